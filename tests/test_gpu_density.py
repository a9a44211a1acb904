"""GPU tests of the scalar density quantities s = rho^alpha ('density', VPS_DENSITY) and s = ln rho ('log_density',
VPS_LOG_DENSITY) on every gridding route, against the float64 reference of tests/density_ref.py (pinned by
tests/test_density_cpu.py).

The bar of every leg is the project's own (tests/test_gpu_parity.py, tests/test_gpu_weighted.py): shell counts bit exact, Psum
within PSUM_RTOL = 2e-5 per live shell, fields within 1e-5 of their max, thin-slab images within 1e-5 of their rms.  The
particle densities are drawn log-uniformly over eight decades (weighted_ref.particles), where log2 rho is far from 0 and the
power and the logarithm show their error.  Every leg prints its worst deviation (pytest -s) before it asserts."""
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import vps_oracle as orc  # noqa: E402

import density_ref as dref  # noqa: E402
import weighted_ref as wref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSUM_RTOL = 2e-5
FIELD_RTOL = 1e-5
IMAGE_RTOL = 1e-5
WHICH = (1.0, 0.5, -0.5, "log")          # the plain density, two powers, the logarithm


@pytest.fixture(scope="module")
def K():
    from vpower import device
    return device.default_kernels()


def _free(K):
    K._work.clear()
    torch.cuda.empty_cache()


def _name(which):
    return "log_density" if which == "log" else "density alpha=%+.3f" % which


def _code(which):
    from vpower import device
    return device.LOG_DENSITY if which == "log" else device.Density(which)


def _spctrm(box, which, **kw):
    if which == "log":
        return box.spctrm("log_density", **kw)
    return box.spctrm("density", **kw) if which == 1.0 else box.spctrm("density", density_weight=which, **kw)


def _check(leg, got, ref, rtol=PSUM_RTOL):
    """got: a PowerSpectrum or an (nbins, 4) table; ref: (nbins, 4).  Counts exact, Psum within rtol per live shell."""
    gs, gn = (got.Psum, got.Nsample) if hasattr(got, "Psum") else (got[:, 2], got[:, 3])
    live = ref[:, 3] > 0
    dev = float(np.max(np.abs(gs[live] - ref[live, 2]) / np.abs(ref[live, 2])))
    print("density leg %-62s worst per-shell deviation %.3e (bar %.1e)" % (leg, dev, rtol))
    assert np.array_equal(np.asarray(gn, dtype=np.int64), ref[:, 3].astype(np.int64)), leg
    assert dev < rtol, (leg, dev)
    return dev


def _gas(pos, vel, dens, L):
    from vpower import interp
    return interp.GasParticles(pos, np.ones(len(pos), np.float32), dens, vel, L)


# --------------------------------------------------------------------------------- 1. fused route, whole grid ----
@pytest.mark.parametrize("N,Np", [(64, 300_000), (250, 2_000_000), (512, 6_000_000)])
def test_fused_route_whole_grid_against_reference(K, N, Np):
    """BoxField.spctrm of a particle-backed field: the DENSITY instantiation of the pencil kernel at 64 and 512 (N = 250 has no
    pencil plan and goes through the un-fused grid); a fifth of the cells empty, one over-full pencil (the p.side[] tail).
    At N = 64 also: 'density' called twice agrees with itself to the order of the LDS adds (identical counts, Psum to 2e-6)."""
    L = 1.0
    pos, vel, dens = dref.fused_inputs(N, Np, L)
    grid = wref.ngp_vec_grid(pos, vel, dens, N, L)
    assert np.mean(grid[..., 3] == 0) > 0.15
    rho = grid[..., 3].copy()
    del grid
    assert K.fused_supported(N, 5) == K.fused_supported(N, 6) == K.fused_supported(N, 2)
    box = _gas(pos, vel, dens, L).deposit_to_field(N)
    for which in WHICH:
        _check("fused N=%d %s" % (N, _name(which)), _spctrm(box, which), dref.table(dref.field(rho, which), L, N))
    if N == 64:
        a, b = box.spctrm("density"), box.spctrm("density", density_weight=1.0)
        assert np.array_equal(a.Nsample, b.Nsample) and np.allclose(a.Psum, b.Psum, rtol=2e-6, atol=0)
    _free(K)


# ------------------------------------------------------------------------------------- 2. thin-slab images ----
@pytest.mark.parametrize("N,nx,x0,which", [(1024, 16, 512, 0.5), (2048, 16, 1200, "log"), (2048, 16, 2032, 1.0),
                                            (4096, 16, 4080, -0.5), (4096, 16, 2064, "log")])
def test_fused_thin_slab_images_against_reference(K, N, nx, x0, which):
    """vps_deposit_fft_zy at the line lengths 1024, 2048, 4096 (the pencil instantiations whole grids do not reach) on a thin
    x-slab: the ONE z/y image against numpy's transform of the reference slab."""
    L = 1.0
    rng = np.random.default_rng(N + x0)
    Np = 600_000
    pos = rng.random((Np, 3), dtype=np.float32)
    pos[: Np // 2, 0] = (x0 + rng.random(Np // 2, dtype=np.float32) * nx) / N
    pos[: Np // 8, 1:] *= 0.05                                      # a crowded corner: pencils that outgrow their registers
    vel = rng.standard_normal((Np, 3), dtype=np.float32)
    dens = wref.eight_decade_densities(rng, Np)
    spec, nyq = K.deposit_fft_zy(K.to_device(pos), K.to_device(vel), K.to_device(dens), N, L, x0, nx, _code(which))
    assert spec.shape[0] == 1 and nyq.shape[0] == 1
    f = dref.field(dref.slab_rho(pos, dens, N, L, x0, nx), which)
    ref = np.fft.fft(np.fft.rfft(f, axis=2), axis=1)                # [x, ky, kz <= N/2]
    scale = np.sqrt(np.mean(np.abs(ref) ** 2))
    err = np.max(np.abs(spec[0].cpu().numpy().transpose(2, 1, 0) - ref[:, :, : N // 2])) / scale
    errn = np.max(np.abs(nyq[0].cpu().numpy().T - ref[:, :, N // 2])) / scale
    print("density leg thin slab N=%d x0=%d %s: image deviation %.3e, Nyquist %.3e of rms (bar %.0e)"
          % (N, x0, _name(which), err, errn, IMAGE_RTOL))
    assert err < IMAGE_RTOL and errn < IMAGE_RTOL, (err, errn)
    _free(K)


# -------------------------------------------------- 3. / 4. un-fused deposit, grid algebra, neighbour search ----
@pytest.mark.parametrize("which", WHICH)
def test_unfused_fields_and_spectra_against_reference(K, which):
    from vpower import device, interp
    N, L, Np = 64, 2.0, 200_000
    pos, vel, dens = wref.particles(7, Np, N, L)
    q = _code(which)
    dpos, dvel, drho = K.to_device(pos), K.to_device(vel), K.to_device(dens)
    grid = wref.ngp_vec_grid(pos, vel, dens, N, L)
    ref_f = dref.field(grid, which)
    scale = np.max(np.abs(ref_f))
    ref = dref.table(ref_f, L, N)
    pipe = device.PowerPipeline(N, L, kernels=K, comm=device.SlabComm(enabled=False))

    def field_ok(leg, got, rf=ref_f, sc=scale):
        err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - rf))) / sc
        print("density leg %-62s worst field deviation %.3e of max (bar %.0e)" % (leg, err, FIELD_RTOL))
        assert err < FIELD_RTOL, (leg, err)

    # vps_deposit_field: the brick epilogue, one channel
    f = K.deposit_field(dpos, dvel, drho, N, L, 0, N, q)
    assert f.shape[0] == 1
    field_ok("deposit_field %s" % _name(which), f[0])
    _check("deposit_field spectrum %s" % _name(which), pipe.spectrum([f[0]]), ref)
    # vps_field_algebra_out on a HOST-built BoxField (vx, vy, vz, mass): rho = mass / Lcell^3
    v, m = orc.vm_from_vec_grid(grid, L / N, zero_empty=True)
    box = interp.BoxField(v, m, L / N)
    g = K.field_algebra_out(box._device_chans(K), q, device.FLAG_INPUT_IS_VM, L / N)
    assert g.shape[0] == 1
    field_ok("field_algebra_out (gridded) %s" % _name(which), g[0])
    sp = _spctrm(box, which)
    _check("BoxField(host).spctrm %s" % _name(which), sp, ref)
    if which == 1.0:      # identity: spctrm('density') of a gridded field is the spectrum of mass / Lcell^3
        direct = pipe.spectrum([K.to_device((m / (L / N) ** 3).astype(np.float32))])
        live = direct[:, 3] > 0
        dev = float(np.max(np.abs(sp.Psum[live] - direct[live, 2]) / direct[live, 2]))
        print("density leg identity spctrm('density') vs spectrum([mass / Lcell^3]): %.3e (bar %.1e)" % (dev, PSUM_RTOL))
        assert np.array_equal(sp.Nsample, direct[:, 3]) and dev < PSUM_RTOL
    # ... and the in-place form on [rho v, rho] channels: the result is channel 0
    ch = K.to_device(np.ascontiguousarray(np.moveaxis(grid, -1, 0)).astype(np.float32))
    K.field_algebra(ch, q, 0, L / N)
    field_ok("field_algebra (in place) %s" % _name(which), ch[0])
    # the un-binned power grid
    P = box.log_density_power() if which == "log" else box.density_power(which)
    Pref = orc.scalar_power(ref_f, L, N)
    assert P.shape == (N, N, N) and abs(P.sum() / Pref.sum() - 1) < PSUM_RTOL
    # vps_nn_resample_quantity: the nearest particle's density
    Nn, Npn = 32, 20_000
    ref_n = dref.field(dref.nn_rho(pos[:Npn], dens[:Npn], Nn, L), which)
    gpn = _gas(pos[:Npn], vel[:Npn], dens[:Npn], L)
    ax = orc.lattice_axes_library(L, Nn)
    fn, _ = K.nn_resample_quantity(gpn._device_pos(K), gpn._device_payload(K), (ax, ax, ax), 0, Nn, L / Nn, q)
    assert fn.shape[0] == 1
    field_ok("nn_resample_quantity %s" % _name(which), fn[0], ref_n, np.max(np.abs(ref_n)))
    _check("ann_interp_to_field.spctrm %s" % _name(which), _spctrm(gpn.ann_interp_to_field(Nn), which), dref.table(ref_n, L, Nn))
    # a SECOND quantity of a neighbour-backed field is served from its four grids (vps_field_algebra_out, gridded input)
    boxn = gpn.ann_interp_to_field(Nn)
    boxn.spctrm("velocity")
    _check("neighbour-backed field, second quantity %s" % _name(which), _spctrm(boxn, which), dref.table(ref_n, L, Nn))
    _free(K)


# ----------------------------------------------------------------------------- 5. CIC with deconvolution ----
def test_cic_assignment_with_deconvolution(K):
    N, L, Np = 256, 1.0, 1_500_000
    pos, vel, dens = wref.particles(17, Np, N, L, empty_fraction=0.0)
    rho = wref.ngp_vec_grid(pos, vel, dens, N, L, assignment="cic")[..., 3].copy()
    box = _gas(pos, vel, dens, L).deposit_to_field(N, assignment="cic")
    for which in (1.0, "log", 0.5):
        _check("CIC N=256 deconvolve %s" % _name(which), _spctrm(box, which, deconvolve=True),
               dref.table(dref.field(rho, which), L, N, window="cic"))
    _free(K)


# ------------------------------------------------------------------------------ 6. context state, residency ----
def test_second_quantity_reuses_the_sort_and_alpha_is_never_stale(K):
    from vpower import device
    N, L, Np = 128, 1.0, 1_000_000
    pos, vel, dens = wref.particles(19, Np, N, L)
    box = _gas(pos, vel, dens, L).deposit_to_field(N)
    first = box.spctrm("velocity")
    n0 = K.h2d_copies
    K.timing(True)
    second = box.spctrm("log_density")
    tim = K.timing_get()
    K.timing(False)
    assert K.h2d_copies == n0, "no upload for a second quantity"
    assert tim["deposit"][0] == 0 and tim["fft_z"][0] == 1, "the bucket sort is reused: only the pencil launch runs"
    grid = wref.ngp_vec_grid(pos, vel, dens, N, L)
    _check("second quantity (sort reused) log_density", second, dref.table(dref.field(grid, "log"), L, N))
    assert np.array_equal(first.Nsample, second.Nsample)
    # Density(a) and WeightedVelocity(b) share ONE exponent slot of the context: interleaved on two fields with different
    # exponents, every call carries its own
    pos2, vel2, dens2 = wref.particles(23, Np // 2, N, L)
    box2 = _gas(pos2, vel2, dens2, L).deposit_to_field(N)
    grid2 = wref.ngp_vec_grid(pos2, vel2, dens2, N, L)
    grids = {1: grid, 2: grid2}
    refs = {}
    for which, kind, a in ((1, "d", 0.5), (2, "w", 1.0 / 3.0), (1, "w", -0.5), (2, "d", -0.5), (1, "d", 1.0), (2, "w", 0.5),
                           (1, "d", 0.5), (2, "d", 2.0)):
        key = (which, kind, a)
        if key not in refs:
            refs[key] = (dref.table(dref.density_field(grids[which], a), L, N) if kind == "d"
                         else wref.table(wref.fields_from_vec_grid(grids[which], a), L, N))
        b = box if which == 1 else box2
        got = b.spctrm("density", density_weight=a) if kind == "d" else b.spctrm("weighted_velocity", density_weight=a)
        _check("interleaved field %d %s alpha=%+.3f" % (which, "density" if kind == "d" else "weighted", a), got, refs[key])
    assert device.Density(0.5) != device.WeightedVelocity(0.5)
    _free(K)


# ------------------------------------------------------------------------------------------------ 7. slabs ----
def _nan_buffer(K, n):
    return torch.full((n,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=K.device)


@pytest.mark.parametrize("which", [0.5, "log"])
def test_emulated_slab_exchange_through_the_production_chunk_calls(K, which):
    """vps_deposit_fft_z per sender slab (ONE z image) -> vps_fft_y chunk by chunk (packed rows) -> the all-to-all played by
    slicing -> vps_fft_x_bin_chunk of the one component on every receiver, against the float64 reference of the whole grid."""
    from vpower import device
    N, G, C_, Np, L = 512, 4, 2, 6_000_000, 1.0
    pos, vel, dens = wref.particles(29, Np, N, L)
    dpos, dvel, drho = K.to_device(pos), K.to_device(vel), K.to_device(dens)
    nx = N // G
    zimgs = [K.deposit_fft_z(dpos, dvel, drho, N, L, g * nx, nx, _code(which)) for g in range(G)]
    assert all(z.shape[0] == 1 for z in zimgs)
    pipe = device.PowerPipeline(N, L, kernels=K, comm=device.SlabComm(enabled=False))
    pipe.prepare()
    psum, ns = pipe.new_accumulators()
    for c in range(C_):
        with K.binning_only():
            packed = K.y_packed(N)
            blk = K.chunk_block(N, nx, G, C_, c, packed)
            sends = [K.fft_y_chunk(z[0], N, nx, G, C_, c, out=_nan_buffer(K, G * blk)) for z in zimgs]
        for h in range(G):
            recv = torch.cat([sends[g][h * blk:(h + 1) * blk] for g in range(G)])
            K.fft_x_bin_chunk([recv], N, nx, G, C_, c, h, packed, psum, ns)
            del recv
        del sends
    tab = pipe.finish(psum, ns)
    del zimgs
    _free(K)
    rho = wref.ngp_vec_grid(pos, vel, dens, N, L)[..., 3].copy()
    _check("emulated slabs N=%d G=%d chunks=%d %s" % (N, G, C_, _name(which)), tab, dref.table(dref.field(rho, which), L, N))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _paths():
    for p in (ROOT, os.path.join(ROOT, "large-velocity-power-spectrum_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _gloo_worker(rank, world, port, N, Np, out_dir):
    _paths()
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vpower import device
        import weighted_ref
        K = device.default_kernels(0)
        pos, vel, dens = weighted_ref.particles(31, Np, N, 1.0)
        d = [K.to_device(a) for a in (pos, vel, dens)]
        pipe = device.PowerPipeline(N, 1.0, kernels=K, comm=device.SlabComm())
        assert pipe.comm.world == world and pipe.x0 == rank * (N // world)
        # a scalar quantity (one z image) between two vector ones in the quantity pipeline
        qs = (device.VELOCITY, device.Density(0.5), device.WeightedVelocity(1.0 / 3.0), device.LOG_DENSITY)
        prod = [(lambda q=q: list(K.deposit_fft_z(d[0], d[1], d[2], N, 1.0, pipe.x0, pipe.nx, q))) for q in qs]
        accs = [pipe.new_accumulators() for _ in qs]
        if pipe.chunked:
            pipe.pipelined_quantities(prod, accs)
        else:
            for p_, a in zip(prod, accs):
                pipe.accumulate_zimages(p_(), a[0], a[1])
        tabs = [pipe.finish(*a) for a in accs]
        # ... and through the un-fused slab grid
        f = K.deposit_field(d[0], d[1], d[2], N, 1.0, pipe.x0, pipe.nx, device.Density(1.0))
        tabs.append(pipe.spectrum([f[0]]))
        np.save(os.path.join(out_dir, f"dtab_{rank}.npy"), np.stack(tabs))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_share_the_gpu(tmp_path):
    import torch.multiprocessing as mp
    world, N, Np = 2, 64, 200_000
    mp.spawn(_gloo_worker, args=(world, _free_port(), N, Np, str(tmp_path)), nprocs=world, join=True)
    pos, vel, dens = wref.particles(31, Np, N, 1.0)
    grid = wref.ngp_vec_grid(pos, vel, dens, N, 1.0)
    refs = [wref.table(wref.fields_from_vec_grid(grid, 0.0), 1.0, N), dref.table(dref.field(grid, 0.5), 1.0, N),
            wref.table(wref.fields_from_vec_grid(grid, 1.0 / 3.0), 1.0, N), dref.table(dref.field(grid, "log"), 1.0, N),
            dref.table(dref.field(grid, 1.0), 1.0, N)]
    for r in range(world):
        tabs = np.load(tmp_path / f"dtab_{r}.npy")
        assert len(tabs) == len(refs)
        for i, (tab, ref) in enumerate(zip(tabs, refs)):
            _check("gloo rank %d table %d" % (r, i), tab, ref)


def _field_worker(rank, world, port, N, Np, out_dir):
    _paths()
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vpower import device
        import weighted_ref
        K = device.default_kernels(0)
        pos, vel, dens = weighted_ref.particles(47, Np, N, 1.0)
        d = [K.to_device(a) for a in (pos, vel, dens)]
        comm = device.FieldComm()
        assert (comm.world, comm.rank, comm.field_world, comm.field_rank) == (1, 0, world, rank)
        quantities = ("density", "velocity", "log_density")
        units = device.FieldComm.units(quantities)
        assert units == [("density", None), ("velocity", 0), ("velocity", 1), ("velocity", 2), ("log_density", None)]
        mine = comm.mine(quantities)
        pipe = device.PowerPipeline(N, 1.0, kernels=K, comm=comm)
        assert pipe.nx == N and not pipe.chunked
        pipe.prepare()
        tabs = []
        for qn in quantities:                   # every rank takes part in every quantity's reductions, with its own fields only
            psum, ns = pipe.new_accumulators()
            comps = [c for (u, c) in mine if u == qn]
            if comps:
                _, code = device.resolve_quantity(qn)
                scalar = comps == [None]
                with K.binning_only():
                    spec, nyq = K.deposit_fft_zy(d[0], d[1], d[2], N, 1.0, 0, N, code, component=None if scalar else tuple(comps))
                assert spec.shape[0] == len(comps)
                pipe.accumulate_spectra(spec, nyq, psum, ns)
            tabs.append(pipe.finish(psum, ns))
        np.save(os.path.join(out_dir, f"dftab_{rank}.npy"), np.stack(tabs))
        np.save(os.path.join(out_dir, f"dmine_{rank}.npy"), np.array([[-1 if c is None else c, quantities.index(u)] for u, c in mine]))
    finally:
        dist.destroy_process_group()


def test_field_parallel_gloo_ranks_deal_the_scalars_out_as_one_unit(tmp_path):
    import torch.multiprocessing as mp
    world, N, Np = 2, 64, 200_000
    mp.spawn(_field_worker, args=(world, _free_port(), N, Np, str(tmp_path)), nprocs=world, join=True)
    pos, vel, dens = wref.particles(47, Np, N, 1.0)
    grid = wref.ngp_vec_grid(pos, vel, dens, N, 1.0)
    refs = [dref.table(dref.field(grid, 1.0), 1.0, N), wref.table(wref.fields_from_vec_grid(grid, 0.0), 1.0, N),
            dref.table(dref.field(grid, "log"), 1.0, N)]
    dealt = []
    for r in range(world):
        dealt += [tuple(x) for x in np.load(tmp_path / f"dmine_{r}.npy")]
        for i, (tab, ref) in enumerate(zip(np.load(tmp_path / f"dftab_{r}.npy"), refs)):
            _check("field ranks %d/%d quantity %d" % (r, world, i), tab, ref)
    assert sorted(dealt) == sorted([(-1, 0), (0, 1), (1, 1), (2, 1), (-1, 2)])    # every field once


# ------------------------------------------------------------------------------------------ 8. C ABI refusals ----
def test_c_abi_refusals_leave_the_context_usable():
    from vpower import _ffi, device
    K2 = device.HipKernels()               # a context of its own: no exponent was ever set on it
    lib, ctx = K2.lib, K2.ctx
    N, L, Np = 64, 1.0, 100_000
    DENS, LOGD = 5, 6
    pos, vel, dens = wref.particles(41, Np, N, L)
    d = [K2.to_device(a) for a in (pos, vel, dens)]
    spec = K2.empty((1, N // 2, N, N), torch.complex64)
    nyq = K2.empty((1, N, N), torch.complex64)
    work = K2.workspace("fused", lib.vps_deposit_fft_zy_workspace_bytes_shared(Np, N, N))
    out = K2.empty((1, N, N, N), torch.float32)
    chans = K2.zeros((4, N, N, N), torch.float32)
    K2._stream()
    assert lib.vps_deposit_fft_zy_supported(ctx, N, DENS) == 1 and lib.vps_deposit_fft_zy_supported(ctx, N, LOGD) == 1
    assert lib.vps_deposit_fft_zy_supported(ctx, N, 7) == 0

    def fused(q, flags=0):
        return lib.vps_deposit_fft_zy(ctx, K2._ptr(d[0]), 0, K2._ptr(d[1]), K2._ptr(d[2]), Np, N, L, 0, N, q, flags,
                                      K2._ptr(spec), K2._ptr(nyq), K2._ptr(work))

    def unfused(q, flags=0):
        w = K2.workspace("deposit", lib.vps_deposit_workspace_bytes(Np, 4, N, N))
        return lib.vps_deposit_field(ctx, K2._ptr(d[0]), 0, K2._ptr(d[1]), K2._ptr(d[2]), Np, N, L, 0, N, q, flags, K2._ptr(out), K2._ptr(w))

    def fused_z(q, slab, flags=0):
        zimg = K2.empty((1, K2.zimage_elems(N, N)), torch.complex64)
        if slab:
            w = K2.workspace("fused_z", lib.vps_deposit_fft_z_workspace_bytes_slab(Np, Np, N, N))
            return lib.vps_deposit_fft_z_slab(ctx, K2._ptr(d[0]), 0, K2._ptr(d[1]), K2._ptr(d[2]), Np, Np, N, L, 0, N, q, flags,
                                              K2._ptr(zimg), K2._ptr(w))
        w = K2.workspace("fused_z", lib.vps_deposit_fft_z_workspace_bytes(Np, N, N))
        return lib.vps_deposit_fft_z(ctx, K2._ptr(d[0]), 0, K2._ptr(d[1]), K2._ptr(d[2]), Np, N, L, 0, N, q, flags,
                                     K2._ptr(zimg), K2._ptr(w))

    Nn = 16
    ax = np.ascontiguousarray(orc.lattice_axes_library(L, Nn))
    rhov = K2.density_velocity_vector(d[1], d[2])

    def nn(q, flags=0):
        o = K2.empty((1, Nn, Nn, Nn), torch.float32)
        w = K2.workspace("nn", lib.vps_nn_workspace_bytes(Np, 0, Nn ** 3))
        return lib.vps_nn_resample_quantity(ctx, K2._ptr(d[0]), 0, K2._ptr(rhov), Np, _ffi.as_dp(ax), Nn, _ffi.as_dp(ax), Nn,
                                            _ffi.as_dp(ax), Nn, 0, Nn, L / Nn, q, flags, K2._ptr(o), None, K2._ptr(w))

    def algebra(q, flags=0):
        return lib.vps_field_algebra_out(ctx, q, flags, L / N, K2._ptr(chans), N ** 3, K2._ptr(out))

    K2.timing(True)
    # VPS_DENSITY before any exponent is set, on every entry point
    for call in (lambda: fused_z(DENS, False), lambda: fused_z(DENS, True), lambda: nn(DENS), lambda: fused(DENS),
                 lambda: unfused(DENS), lambda: algebra(DENS)):
        assert call() == -1 and b"vps_set_density_weight" in lib.vps_last_error(ctx)
    assert lib.vps_set_density_weight(ctx, float("nan")) == -1 and fused(DENS) == -1          # a refused alpha sets nothing
    assert lib.vps_set_density_weight(ctx, 0.5) == 0
    # the three flags, with either code
    for q in (DENS, LOGD):
        for flag, word in ((device.FLAG_SHARE_ENERGY, b"SHARE_ENERGY"), (device.FLAG_REFERENCE_MOMENTUM_BUG, b"MOMENTUM_BUG"),
                           (1 << 4, b"COMPONENTS"), (3 << 4, b"COMPONENTS")):
            for call in (fused, unfused, nn, algebra, lambda q_, f_: fused_z(q_, False, f_), lambda q_, f_: fused_z(q_, True, f_)):
                assert call(q, flag) == -1, (q, flag)
                assert word in lib.vps_last_error(ctx), lib.vps_last_error(ctx)
    assert all(n == 0 for n, _ in K2.timing_get().values()), "a refused call enqueues nothing"
    K2.timing(False)
    # the next valid calls are right
    assert all(c(q) == 0 for q in (DENS, LOGD) for c in (fused, unfused, nn, algebra))
    assert all(fused_z(q, s) == 0 for q in (DENS, LOGD) for s in (False, True))
    pipe = device.PowerPipeline(N, L, kernels=K2, comm=device.SlabComm(enabled=False))
    grid = wref.ngp_vec_grid(pos, vel, dens, N, L)
    assert fused(DENS) == 0 and unfused(DENS) == 0
    ref = dref.table(dref.field(grid, 0.5), L, N)
    _check("C ABI fused VPS_DENSITY after the refusals", pipe.finish(*pipe.accumulate_spectra(spec, nyq)), ref)
    _check("C ABI deposit_field VPS_DENSITY after the refusals", pipe.spectrum([out[0]]), ref)
    assert fused(LOGD) == 0
    _check("C ABI fused VPS_LOG_DENSITY after the refusals", pipe.finish(*pipe.accumulate_spectra(spec, nyq)),
           dref.table(dref.field(grid, "log"), L, N))
    # the wrapper refuses the bare code without its exponent
    with pytest.raises(Exception, match="exponent"):
        K2.deposit_field(d[0], d[1], d[2], N, L, 0, N, device.DENSITY)
    K2.close()
