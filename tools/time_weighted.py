"""Cost of the density-weighted velocity against the plain velocity on the C4 workload (GPU box):

    python tools/time_weighted.py [--N 2048] [--np 100000000] [--reps 5] [--quantities velocity,rho13_velocity]

spctrm(q) and helmholtz_spctrm(q) of a particle-backed field (2048^3, 1e8 particles, warm: the particle sort is reused by every
call), wall ms per call, all interleaved.  The expectation is "equal within run-to-run noise" (same rounds, same bytes; one
log / multiply / exp per record more); the comparison that counts is against `--quantities velocity` of the PARENT commit on
the same box -- the script only uses quantity names, so it runs unchanged on a checkout without the weighted quantity.
Prints one JSON line."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quantities", default="velocity,rho13_velocity")
    a = ap.parse_args()
    N, reps, names = a.N, a.reps, a.quantities.split(",")
    K = device.default_kernels()
    out = {"N": N, "np": a.np, "reps": reps}
    pos, vel, dens = synth.particles_device(K, synth.BASE_SEED + 4, a.np)
    box = interp.BoxField._from_particles((pos, vel, dens), N, 1.0)
    runs = []
    for q in names:
        runs.append(("spctrm(%s)" % q, lambda q=q: box.spctrm(q)))
        runs.append(("helmholtz_spctrm(%s)" % q, lambda q=q: box.helmholtz_spctrm(q)))
    for _, fn in runs:                          # warm: kernels loaded, sort made, workspaces allocated
        fn()
    t = {name: [] for name, _ in runs}
    for _ in range(reps):
        for name, fn in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append(1e3 * (time.perf_counter() - t0))
    for name, v in t.items():
        out[name + "_ms"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
