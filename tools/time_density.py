"""Cost of the scalar density quantities against the kinetic energy on the C4 workload (GPU box):

    python tools/time_density.py [--N 2048] [--np 100000000] [--reps 7] [--quantities energy,density,log_density]

spctrm(q) of a particle-backed field (2048^3, 1e8 particles, warm: the particle sort is reused by every call), interleaved;
per call the GPU time of the library's own timing API (vps_timing: the sum over all kernel kinds, and the pencil launch
`fft_z` alone) and the wall time, medians over the repetitions.  The density launch runs one accumulation round and one
transform where the energy launch runs four rounds and one transform, so the expectation is density <= energy.  The script
only uses quantity names: `--quantities energy` runs unchanged on a checkout without the density quantities (the parent's
energy figure).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "large-velocity-power-spectrum_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vpower import device, interp, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--np", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quantities", default="energy,density,log_density")
    a = ap.parse_args()
    N, reps, names = a.N, a.reps, a.quantities.split(",")
    K = device.default_kernels()
    out = {"N": N, "np": a.np, "reps": reps}
    pos, vel, dens = synth.particles_device(K, synth.BASE_SEED + 4, a.np)
    box = interp.BoxField._from_particles((pos, vel, dens), N, 1.0)
    for q in names:                             # warm: kernels loaded, sort made, workspaces allocated
        box.spctrm(q)
    t = {q: {"wall": [], "gpu": [], "fft_z": [], "deposit_launches": []} for q in names}
    for _ in range(reps):
        for q in names:
            torch.cuda.synchronize()
            K.timing(True)
            t0 = time.perf_counter()
            box.spctrm(q)
            torch.cuda.synchronize()
            t[q]["wall"].append(1e3 * (time.perf_counter() - t0))
            tim = K.timing_get()
            K.timing(False)
            t[q]["gpu"].append(sum(ms for _, ms in tim.values()))
            t[q]["fft_z"].append(tim["fft_z"][1])
            t[q]["deposit_launches"].append(tim["deposit"][0])
    for q, v in t.items():
        out[q] = {"gpu_ms_median": float(np.median(v["gpu"])), "fft_z_ms_median": float(np.median(v["fft_z"])),
                  "wall_ms_median": float(np.median(v["wall"])), "gpu_ms_min": float(np.min(v["gpu"])),
                  "gpu_ms_max": float(np.max(v["gpu"])), "sort_reused": all(n == 0 for n in v["deposit_launches"])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
