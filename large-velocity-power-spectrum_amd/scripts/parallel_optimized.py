#!/usr/bin/env python3
"""GPU drop-in for the reference driver scripts/parallel_optimized.py.

    python parallel_optimized.py -i snapshot.hdf5 -o outdir -N 1024 -f
    python -m torch.distributed.run --nproc-per-node 8 parallel_optimized.py -i ... -N 2048 -f

Same flags (parallel_optimized.py:42-61), same preprocessing (:280-291), same output
`<out>/Pk.txt` = np.savetxt of the (nbins,4) float32 table [k, P, Psum, Nsample] (:473),
same module-level helper names (`planner`, `FFTW_power`, `FFTW_vector_power`, `pair_power`,
`hist_sample`).  Differences: the nearest-neighbour search is EXACT (Annoy's answers are
approximate and unpinned), and the O(N^3 m^3) fold across MPI ranks is replaced by one
slab-decomposed N^3 FFT (identical spectrum), so `-M` and `-b` are
accepted and ignored and any number of ranks dividing N/2 works (not only cubes).
"""
import argparse
import datetime
import os
import sys
import warnings

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))

SNAPSHOT = "snapshot_550.hdf5"
SAVEDIR = "../output/"
NBUFFER = 5000
NTOT = 1000
MAXNBOX = 500
LTOT = 1
remove_bulk_velocity = True
GRIDDINGS = ("nn", "ngp", "cic", "tsc")
SECOND_MOMENT = ("total_energy", "subgrid_energy", "dispersion",      # vpower.device.SECOND_MOMENT_QUANTITIES: deposits only
                 "subgrid_stress", "dispersion_tensor")


def build_parser():
    p = argparse.ArgumentParser(description="Compute the velocity power spectrum on MI355X GPUs.",
                                usage="python %(prog)s [options]  (torchrun for several GPUs)")
    p.add_argument("-i", "--input", nargs="?", type=str, default=SNAPSHOT, help="Path to the snapshot file.")
    p.add_argument("-o", "--output", nargs="?", type=str, default=SAVEDIR, help="Directory to save the power spectrum.")
    p.add_argument("-N", "--ntot", nargs="?", type=int, default=NTOT, help="Total resolution.")
    p.add_argument("-M", "--maxnbox", nargs="?", type=int, default=MAXNBOX, help="Accepted for compatibility; unused.")
    p.add_argument("-l", "--ltot", nargs="?", type=int, default=LTOT, help="Total length of the box.")
    p.add_argument("-b", "--nbuffer", nargs="?", type=int, default=NBUFFER, help="Accepted for compatibility; unused.")
    p.add_argument("-f", action="store_true", help="Skip confirmation and start the computation.")
    p.add_argument("--helmholtz", action="store_true",
                   help="Also write the compressive and solenoidal parts of the spectrum (Helmholtz decomposition) to "
                        "Pk_compressive.txt and Pk_solenoidal.txt, in Pk.txt's format.")
    p.add_argument("--quantity", type=str, default="velocity", metavar="NAME",
                   help="What to take the spectrum of: velocity (default: the reference's raw nearest-neighbour velocity, Pk.txt "
                        "unchanged), momentum, energy, weighted_velocity, rho13_velocity, rho12_velocity, density, log_density, "
                        "total_energy, subgrid_energy, dispersion, subgrid_stress, dispersion_tensor (vpower.device.resolve_quantity; "
                        "the last five are the kinetic energy of a cell's particles, its part the gridded mean velocity does not "
                        "resolve, the velocity dispersion, and the full contraction of the sub-grid stress tensor and of the "
                        "velocity-dispersion tensor: --gridding ngp, cic or tsc only).  Every quantity but velocity needs "
                        "PartType0/Density in the snapshot.")
    p.add_argument("--density-weight", type=float, default=None, metavar="ALPHA",
                   help="Exponent alpha of --quantity weighted_velocity (rho^alpha v) or density (rho^alpha; default 1).")
    p.add_argument("--gridding", type=str, default="nn", choices=GRIDDINGS,
                   help="How the particles reach the grid: nn (default: the reference's nearest-neighbour resampling, Pk.txt "
                        "unchanged), or a mass-assignment deposit of [rho v, rho] -- ngp, cic, tsc -- with the quantity formed per "
                        "cell (velocity = sum rho v / sum rho).  Every deposit needs PartType0/Density, --quantity velocity included.")
    p.add_argument("--deconvolve", action="store_true",
                   help="Divide |F(k)|^2 by the window of the --gridding assignment (ngp, cic, tsc; refused with nn).")
    return p


def check_gridding(parser, args):
    """--deconvolve needs a mass-assignment window: refused (parser.error) with the nearest-neighbour gridding."""
    if args.deconvolve and args.gridding == "nn":
        parser.error("--deconvolve divides by the window of a mass assignment: pass --gridding ngp, cic or tsc")
    if args.quantity in SECOND_MOMENT and args.gridding == "nn":
        parser.error("--quantity %s is made of the second moment of a cell's particles, and one nearest particle has none: "
                     "pass --gridding ngp, cic or tsc" % args.quantity)
    return args


def resolve_cli_quantity(args):
    """(name, code) of --quantity / --density-weight through vpower.device.resolve_quantity; --helmholtz keeps refusing scalar
    quantities.  Raises what resolve_quantity raises."""
    from vpower import device
    return device.resolve_quantity(args.quantity, args.density_weight,
                                   supported=device.VECTOR_QUANTITIES if args.helmholtz else None)


def planner(n_total_res, l_total_length, n_box_affordable, n_total_threads):
    """The reference's fold planner (parallel_optimized.py:70-88), kept for callers that
    inspect it; the GPU path does not fold."""
    ntpa = round(n_total_threads ** (1 / 3))
    assert ntpa ** 3 == n_total_threads, \
        "Number of threads must be a cube of an integer. Support for any number is not yet implemented."
    ntpa = int(ntpa)
    loops_per_axis = 1
    n_full = n_total_res / ntpa
    assert n_full.is_integer(), "Divided Nbox must be an integer."
    n_box = n_full
    while n_box > n_box_affordable or not n_box.is_integer():
        loops_per_axis += 1
        n_box = n_full / loops_per_axis
    n_box = int(n_box)
    return loops_per_axis ** 3, ntpa, n_box, n_box / n_total_res * l_total_length


def FFTW_power(f, Lbox, Nsize):
    """0.5*|const*FFT3(f)|^2, float32 (parallel_optimized.py:124-141)."""
    from vpower import interp
    return interp._scalar_power(f, Lbox, Nsize).astype(np.float32)


def FFTW_vector_power(fx, fy, fz, Lbox, Nsize):
    """parallel_optimized.py:92-120."""
    from vpower import interp
    return interp._vector_power(fx, fy, fz, Lbox, Nsize).astype(np.float32)


def pair_power(Pk, Lbox, Nbox, shift=np.array([0, 0, 0])):
    """(n,2) [|k|, P]; each axis shifted by -shift[i] where shift[i] != 0
    (parallel_optimized.py:145-172)."""
    from vpower import device
    k = device.default_kernels()
    ks = device.k_axis(Lbox, Nbox)
    axes = [ks - shift[i] if shift[i] != 0 else ks for i in range(3)]
    return np.column_stack((k.pair_k(*axes).cpu().numpy(), np.ravel(Pk)))


def hist_sample(Pk_pair, kmin, kmax, spacing):
    """(nbins,4) [centre, P, Psum, Nsample] with np.linspace edges and
    n_bins=int((kmax-kmin)/spacing)+1; P is NaN in empty bins (parallel_optimized.py:176-190)."""
    from vpower import device
    k = device.default_kernels()
    centers, edges = device.bin_edges(kmin, kmax, spacing, "script")
    pair = np.asarray(Pk_pair, dtype=np.float64)
    psum, ns = k.hist_pairs(k.to_device(pair[:, 0]), k.to_device(pair[:, 1]), edges)
    psum, ns = psum.cpu().numpy(), ns.cpu().numpy().astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = psum / ns
    return np.column_stack((centers, P, psum, ns))


def load_particles(path, with_density=False):
    """coords, mass, velocity of PartType0 (parallel_optimized.py:272-276); `.npz` accepted.  with_density: and the particle
    densities (PartType0/Density; `Density` in an .npz) as a fourth array."""
    if path.endswith(".npz"):
        z = np.load(path)
        out = (z["Coordinates"], z["Masses"], z["Velocities"])
        return out + (z["Density"],) if with_density else out
    import h5py
    with h5py.File(path, "r") as f:
        out = (f["PartType0/Coordinates"][:], f["PartType0/Masses"][:], f["PartType0/Velocities"][:])
        return out + (f["PartType0/Density"][:],) if with_density else out


def _script_table(tab):
    tab[:, 1] *= 4 * np.pi * tab[:, 0] ** 2
    tab = np.array(tab, dtype=np.float32)                       # :436
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tab[:, 1] = tab[:, 2] / tab[:, 3] * (4 * np.pi * tab[:, 0] ** 2)   # :463
    return tab


def velocity_spectrum(coords, mass, velocity, ntot, ltot, comm=None, kernels=None, helmholtz=False, quantity=None, density=None,
                      gridding="nn", deconvolve=False):
    """The body of main() after loading: preprocessing, exact NN at x=i*LCELL (float32
    lattice, :343-346), raw velocity gather (:351), P(k) (:409-463).  Returns the float32
    (nbins,4) table that rank 0 saves; helmholtz=True: the tuple (total, compressive, solenoidal) of such tables
    (vpower.device.PowerPipeline.accumulate_helmholtz; total is the table of helmholtz=False).
    quantity: a code of vpower.device.resolve_quantity other than plain velocity, with `density` per particle: the fields of
    that quantity from the nearest particle's [rho v, rho] (vps_nn_resample_quantity) instead of the raw velocity.
    gridding "ngp" / "cic" / "tsc" instead of the default "nn": every rank deposits [rho v, rho] of the replicated particles on
    its x-slab by that mass assignment, the quantity (the velocity included: sum rho v / sum rho) formed per cell, so `density`
    is needed whatever the quantity; deconvolve=True then divides |F(k)|^2 by the assignment's window."""
    import torch
    from vpower import device
    if gridding not in GRIDDINGS:
        raise ValueError("gridding must be one of %s, not %r" % (", ".join(GRIDDINGS), gridding))
    if deconvolve and gridding == "nn":
        raise ValueError("deconvolve needs a mass-assignment gridding (ngp, cic, tsc), not the nearest-neighbour resampling")
    if gridding != "nn" and density is None:
        raise Exception("every deposit gridding needs the particle densities (the velocity is sum rho v / sum rho)")
    if gridding == "nn" and quantity is not None and device.needs_second_moment(quantity):
        raise ValueError("the second-moment quantities (%s) need a mass-assignment gridding " % ", ".join(SECOND_MOMENT) +
                         "(ngp, cic, tsc): one nearest particle has no dispersion")
    if helmholtz and quantity is not None and device.is_tensor(quantity):
        raise ValueError("the Helmholtz decomposition takes the three components of a vector quantity, not the six fields of "
                         "subgrid_stress / dispersion_tensor (quantity %d)" % int(quantity))
    k = kernels if kernels is not None else device.default_kernels()
    pipe = device.PowerPipeline(ntot, ltot, kernels=k, comm=comm, flavour="script", deconvolve=gridding if deconvolve else None)
    lcell = ltot / ntot
    ax = np.array([i * lcell for i in range(ntot)], dtype=np.float32).astype(np.float64)
    # preprocessing of :280-291 on the device, in the snapshot's coordinate dtype
    c = np.asarray(coords)
    pos = k.to_device(c if c.dtype == np.float32 else c.astype(np.float64))
    vel = k.to_device(np.asarray(velocity), torch.float32)
    k.preprocess(pos, vel, k.to_device(np.asarray(mass), torch.float32), True, remove_bulk_velocity)
    # Annoy holds float32 coordinates (add_item, :308): search them as float32
    pos = pos.to(torch.float32)
    if gridding != "nn":
        grid = k.deposit_field(pos, vel, k.to_device(np.asarray(density), torch.float32), ntot, ltot, pipe.x0, pipe.nx,
                               quantity if quantity is not None else device.VELOCITY, assignment=gridding)
    elif quantity is not None and int(quantity) != device.VELOCITY:
        if density is None:
            raise Exception("every quantity but the velocity needs the particle densities")
        rhov = k.density_velocity_vector(vel, k.to_device(np.asarray(density), torch.float32))
        grid, _ = k.nn_resample_quantity(pos, rhov, (ax, ax, ax), pipe.x0, pipe.nx, lcell, quantity)
    else:
        grid, _ = k.nn_resample(pos, vel, (ax, ax, ax), pipe.x0, pipe.nx)
    if helmholtz:
        tabs = pipe.finish_helmholtz(*pipe.accumulate_helmholtz([grid[0], grid[1], grid[2]]))
        return tuple(_script_table(t) for t in tabs)
    # (a tensor quantity's six fields: two groups of three, the off-diagonal group scaled by sqrt(2) -- the full contraction)
    psum, ns = pipe.accumulate(device.contraction_fields([grid[i] for i in range(grid.shape[0])],
                                                         quantity if quantity is not None else device.VELOCITY))
    return _script_table(pipe.finish(psum, ns))


def main(argv=None):
    parser = build_parser()
    args = check_gridding(parser, parser.parse_args(argv))
    qname, qcode = resolve_cli_quantity(args)
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if torch.cuda.is_available():
        torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))
    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl" if torch.cuda.is_available() else "gloo")
    outputfile = os.path.join(args.output, "Pk.txt")
    assert os.path.isdir(args.output), "Output directory does not exist."
    assert os.path.isfile(args.input), "Snapshot file does not exist."
    if rank == 0:
        print(f"[{datetime.datetime.now()}] Plan: one {args.ntot}^3 FFT on {world} GPU(s), no folding.", flush=True)
        if not args.f:
            print("Accept plan? (y/n)", flush=True)
            if input() != "y":
                print("Plan rejected.", flush=True)
                ok = False
            else:
                ok = True
        else:
            ok = True
    else:
        ok = True
    if world > 1:
        flag = torch.tensor([1 if ok else 0])
        if torch.cuda.is_available():
            flag = flag.cuda()
        dist.broadcast(flag, 0)
        ok = bool(flag.item())
    if not ok:
        return 0
    print(f"[{datetime.datetime.now()}] Load snapshot: {args.input}", flush=True) if rank == 0 else None
    if qname == "velocity" and args.gridding == "nn":
        coords, mass, velocity = load_particles(args.input)
        tab = velocity_spectrum(coords, mass, velocity, args.ntot, args.ltot, helmholtz=args.helmholtz)
    else:
        coords, mass, velocity, density = load_particles(args.input, with_density=True)
        tab = velocity_spectrum(coords, mass, velocity, args.ntot, args.ltot, helmholtz=args.helmholtz, quantity=qcode,
                                density=density, gridding=args.gridding, deconvolve=args.deconvolve)
    if rank == 0:
        if args.helmholtz:
            tab, comp, sol = tab
            for name, t in (("Pk_compressive.txt", comp), ("Pk_solenoidal.txt", sol)):
                np.savetxt(os.path.join(args.output, name), t)
                print(f"[{datetime.datetime.now()}] Saved: {os.path.join(args.output, name)}", flush=True)
        np.savetxt(outputfile, tab)
        print(f"[{datetime.datetime.now()}] Saved: {outputfile}", flush=True)
    if world > 1:
        dist.barrier()
    return 0


if __name__ == "__main__":
    assert main() == 0, "Program stopped before completion."
