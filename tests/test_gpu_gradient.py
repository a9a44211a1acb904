"""The velocity-gradient fields of vps_field_algebra_out (VPS_DIVERGENCE, VPS_VORTICITY, VPS_STRAIN_RATE: the stencil kernel of
csrc/gradient.hip) against the references of tests/gradient_ref.py: bit equal on exact inputs at sizes below a tile, off the
tile edges and with 8-byte rows; impulses on every periodic face; random fields within a derived bar; on guarded memory; behind
a busy side stream; their refusals; and the public surface, BoxField.divergence / vorticity / strain_rate / subgrid_flux.
Every case fails on a library without the codes ("vps_field_algebra: quantity 12").
Run on an MI355X:  python -m pytest tests/test_gpu_gradient.py -q -m gpu -s"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import gradient_ref as gr  # noqa: E402
import guarded as gd  # noqa: E402
import stream_probe as sp  # noqa: E402

WHATS = list(gr.CODES)
CACHE = {}


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()
    CACHE.clear()


def _chans(K, u, mass=float("nan")):
    """[4, N, N, N] device channels of the velocity u; the mass channel is not read by the gradient codes: NaN would show."""
    N = u.shape[1]
    ch = torch.empty((4, N, N, N), dtype=torch.float32, device=K.device)
    ch[:3] = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(K.device)
    ch[3] = mass
    return ch


# ------------------------------------------------------------------ exact inputs ----
@pytest.mark.parametrize("N,lc", [(16, 0.25), (96, 2.0), (128, 0.5), (250, 0.125)])
def test_bit_equal_on_integer_velocities(K, N, lc):
    """Integer velocities |u| <= 1024 and a power-of-two Lcell: h is a power of two, every difference, product and sum is exact in
    float32, so the kernel and numpy agree bit for bit whatever the order of anything.  16 is smaller than a tile, 96 is no
    multiple of the 64-cell tile edge, 128 is marched in two x chunks, 250 has N % 4 = 2 (8-byte rows), a remainder tile on both
    tile axes and three x chunks."""
    u = gr.integer_velocity(N, seed=N)
    ch = _chans(K, u)
    ref = gr.fields32_all(u, lc)
    for what in WHATS:
        got = K.velocity_gradient(ch, N, lc, what)
        assert got.shape == (gr.NCH[what], N, N, N) and got.dtype == torch.float32
        got = got.cpu().numpy()
        assert np.array_equal(got, ref[what]), "%s N=%d: %d elements differ" % (what, N, int(np.sum(got != ref[what])))
        assert np.abs(ref[what]).max() > 0
    assert bool(torch.isnan(ch[3]).all()) and np.array_equal(ch[:3].cpu().numpy(), u)          # the input is only read


@pytest.mark.parametrize("N,interior", [(16, (5, 9, 3)), (128, (64, 16, 64)), (250, (84, 16, 32))])
def test_impulses_on_every_face(K, N, interior):
    """One nonzero u_c at (0,0,0), at (N-1,N-1,N-1) and at an interior cell that is the first of a tile on both tile axes and the
    first plane of an x chunk: the output is nonzero at the wrapped neighbours along the axes the quantity differentiates, with
    exactly +-h A (the strain's off-diagonals: half), and nowhere else -- the wrap of each of the six faces, the halo rows and
    columns of the LDS tile and the planes beyond a chunk's ends, each by name."""
    lc, A = 0.25, 3.0
    ch = torch.zeros((4, N, N, N), dtype=torch.float32, device=K.device)
    for p in ((0, 0, 0), (N - 1, N - 1, N - 1), interior):
        for c in range(3):
            ch[(c,) + p] = A
            for what in WHATS:
                got = K.velocity_gradient(ch, N, lc, what)
                idx = got.nonzero()
                vals = got[tuple(idx.t())].cpu().numpy()
                found = {tuple(int(i) for i in row): v for row, v in zip(idx.cpu().numpy(), vals)}
                assert found == gr.impulse_expect(what, c, p, A, lc, N), (what, c, p, found)
            ch[(c,) + p] = 0.0


# ------------------------------------------------------------------ random fields ----
@pytest.mark.parametrize("N", [32, 96])
def test_random_fields_within_the_derived_bar(K, N):
    """Every channel within 16 * 2^-24 * max|u| / Lcell of the float64 reference.  With e = 2^-24 (one float32 rounding,
    relative), M = max|u| and h = 1 / (2 Lcell): one derivative (u+ - u-) * h has three roundings -- the difference, h itself
    (rounded once on the host) and the product -- of a term no larger than 2 M h, so its error is at most 3 e 2 M h (1 + O(e)).
    A channel sums at most three derivatives (the divergence; the vorticity two, the strain's off-diagonals two and an exact
    halving): 3 * 6 e M h for the terms, and two additions of partial sums no larger than 6 M h each: 12 e M h.  Together
    30 e M h = 15 e M / Lcell < 16 e M / Lcell."""
    rng = np.random.default_rng(N)
    u = (rng.standard_normal((3, N, N, N)) + np.array([2.0, -1.0, 0.5])[:, None, None, None]).astype(np.float32)
    lc = 0.37
    ch = _chans(K, u)
    bar = gr.error_bar(u, lc)
    for what in WHATS:
        got = K.velocity_gradient(ch, N, lc, what).double().cpu().numpy()
        ref = gr.fields64(u, lc, what)
        worst = float(np.abs(got - ref).max() / bar)
        print("%s N=%d: worst error %.3f of the bar (16 * 2^-24 * max|u| / Lcell = %.3e)" % (what, N, worst, bar))
        assert np.isfinite(got).all() and worst <= 1.0, (what, N, worst)


# ------------------------------------------------------------------ guarded memory ----
@pytest.mark.parametrize("N", [16, 250])
def test_guarded_exact_size_buffers(K, N):
    """The four input channels are exactly 16 N^3 bytes and the output exactly 4 NCH N^3 poisoned bytes, each between 1 MiB
    guards (tests/guarded.py): no guard is touched, no output element keeps the poison, and the fields are the exact ones."""
    lc = 0.5
    u = gr.integer_velocity(N, seed=1000 + N)
    ref = gr.fields32_all(u, lc)
    G = gd.guarded_kernels()
    try:
        ch = G.empty((4, N, N, N), torch.float32)
        ch[:3] = torch.from_numpy(u).to(G.device)
        ch[3] = 1.0
        for what in WHATS:
            got = G.velocity_gradient(ch, N, lc, what)
            torch.cuda.synchronize()
            rep = G.check()
            assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
            out = gd.report_of(rep, got)
            assert out.nbytes == 4 * gr.NCH[what] * N ** 3 and len(out.poison) == 0, (what, out)
            assert np.array_equal(got.cpu().numpy(), ref[what]), what
            if what == WHATS[0]:                   # (the first check() also covers the arena of the input channels)
                assert gd.report_of(rep, ch).nbytes == 16 * N ** 3
    finally:
        G.release()
        G.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ stream contract ----
@pytest.mark.parametrize("what", WHATS)
def test_side_stream_behind_the_blocker(K, what):
    """velocity_gradient on a side stream behind the blocker of tests/stream_probe.py, the true channels swapped in on that
    stream: the call returns with the blocker pending and gives the bits of the reference of the TRUE data."""
    N, lc = 64, 0.5
    if "blocker" not in CACHE:
        CACHE["blocker"] = sp.Blocker(K.device)
    us = [gr.integer_velocity(N, seed=s) for s in (11, 12)]                  # true, decoy
    refs = [[gr.fields32(u, lc, what)] for u in us]
    true, decoy = _chans(K, us[0], 1.0), _chans(K, us[1], 1.0)
    bufs = [decoy.clone()]
    case = sp.Case("velocity_gradient-%s" % what, bufs, [true], lambda: [K.velocity_gradient(bufs[0], N, lc, what)],
                   refs[0], refs[1], ["exact"])
    sp.run_case(case, CACHE["blocker"])


# ------------------------------------------------------------------ refusals ----
def test_refusals_name_the_quantity_and_enqueue_nothing(K):
    from vpower import _ffi
    from vpower import device as D
    lib = K.lib
    N, L, n = 32, 1.0, 1000
    lc = 0.5
    rng = np.random.default_rng(0)
    pos = K.to_device(rng.random((n, 3)).astype(np.float32))
    vel = K.to_device(rng.standard_normal((n, 3)).astype(np.float32))
    rho = K.to_device((rng.random(n) + 0.5).astype(np.float32))
    rhov = K.density_velocity_vector(vel, rho)
    u = gr.integer_velocity(N, seed=3)
    chans = _chans(K, u, 1.0)
    chans0 = chans.clone()
    nan = float("nan")
    big = torch.full((10, N, N, N), nan, dtype=torch.float32, device=K.device)     # out = big[:6]; big[4:] for the overlaps
    out = big[:6]
    spec = torch.full((3, N // 2, N, N, 2), nan, dtype=torch.float32, device=K.device)
    nyq = torch.full((3, N, N, 2), nan, dtype=torch.float32, device=K.device)
    zimg = torch.full((4 * K.zimage_elems(N, N), 2), nan, dtype=torch.float32, device=K.device)
    work = K.workspace("refusals", max(lib.vps_deposit_assign_workspace_bytes(n, 4, N, 3), lib.vps_deposit_fft_zy_workspace_bytes_shared(n, N, N),
                                       lib.vps_nn_workspace_bytes(n, 0, N ** 3), lib.vps_deposit_workspace_bytes(n, 4, N, N)))
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731
    ax = np.ascontiguousarray((np.arange(N) + 0.5) / N)
    names = {D.DIVERGENCE: "VPS_DIVERGENCE", D.VORTICITY: "VPS_VORTICITY", D.STRAIN_RATE: "VPS_STRAIN_RATE"}
    assert sorted(names) == [12, 13, 14]
    VM = D.FLAG_INPUT_IS_VM
    K._stream()

    def refused(rc, q, code=-1):
        msg = lib.vps_last_error(K.ctx).decode()
        assert rc == code and "quantity %d" % q in msg and names[q] in msg, (q, rc, msg)
        torch.cuda.synchronize()
        for buf in (big, spec, nyq, zimg):
            assert bool(torch.isnan(buf).all()), "a refused call wrote something"
        assert torch.equal(chans, chans0)

    for q, name in names.items():
        nch = D.NCOMP[q]
        assert lib.vps_deposit_fft_zy_supported(K.ctx, N, q) == 0 and lib.vps_deposit_fft_zy_supported(K.ctx, 64, q) == 0
        # the in-place form, a null out_dev
        refused(lib.vps_field_algebra(K.ctx, q, VM, lc, p(chans), N ** 3), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, p(chans), N ** 3, None), q)
        # overlapping buffers: the output starting inside the channels, and the channels starting inside the output
        refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, p(chans), N ** 3, p(chans, 4 * 3 * N ** 3)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, p(big, 4 * (nch - 1) * N ** 3), N ** 3, p(big)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, p(chans), N ** 3, p(chans)), q)
        # without VPS_FLAG_INPUT_IS_VM, and with any other flag next to it
        for flags in (0, D.FLAG_REFERENCE_MOMENTUM_BUG, VM | D.FLAG_REFERENCE_MOMENTUM_BUG, VM | D.FLAG_REUSE_SORT, VM | D.FLAG_SHARE_ENERGY,
                      VM | 0x10, VM | 0x70, VM | D.FLAG_ASSIGN("cic"), VM | D.FLAG_ASSIGN("tsc"), VM | 0x300, 0x300, VM | 0x400):
            refused(lib.vps_field_algebra_out(K.ctx, q, flags, lc, p(chans), N ** 3, p(out)), q)
        # an ncell that is no cube (a multiple of 4 or not), a cube below N = 4, a cube of an odd N, zero, negative
        for ncell in (N ** 3 - 4, N ** 3 + 4, N ** 3 - 1, 2 * N * N, 8, 27, 125, 31 ** 3, 0, -64):
            refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, p(chans), ncell, p(out)), q)
        # a null chans_dev; buffers off the 16-byte boundary (either one); an Lcell that gives no finite h
        refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, None, N ** 3, p(out)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, p(chans, 8), N ** 3, p(out)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM, lc, p(chans), N ** 3, p(out, 4)), q)
        for bad_lc in (0.0, -0.5, float("nan"), float("inf"), 1e-320, 1e300):
            refused(lib.vps_field_algebra_out(K.ctx, q, VM, bad_lc, p(chans), N ** 3, p(out)), q)
        # every other entry point that takes a quantity
        refused(lib.vps_nn_resample_quantity(K.ctx, p(pos), 0, p(rhov), n, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N,
                                             0, N, L / N, q, 0, p(out), None, p(work)), q)
        refused(lib.vps_deposit_fft_zy(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(spec), p(nyq), p(work)), q)
        refused(lib.vps_deposit_fft_z(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        refused(lib.vps_deposit_fft_z_slab(K.ctx, p(pos), 0, p(vel), p(rho), n, n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        for flags in (0, VM, D.FLAG_ASSIGN("cic"), D.FLAG_ASSIGN("tsc")):
            refused(lib.vps_deposit_field(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, flags, p(out), p(work)), q)
        # ... and the context is usable: an exact call right after gives the right answer (N = 4 is the smallest grid taken)
        what = name[4:].lower()
        got = K.velocity_gradient(chans, N, lc, what)
        assert np.array_equal(got.cpu().numpy(), gr.fields32(u, lc, what))
        u4 = gr.integer_velocity(4, seed=4)
        assert np.array_equal(K.velocity_gradient(_chans(K, u4), 4, lc, what).cpu().numpy(), gr.fields32(u4, lc, what))
    # the existing refusals stay: the value 0x300 on the deposit, and the names stay unknown to the spectrum routes
    rc = lib.vps_deposit_field(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, D.VELOCITY, 0x300, p(out), p(work))
    assert rc == -1 and "VPS_FLAG_ASSIGN" in lib.vps_last_error(K.ctx).decode()
    rc = lib.vps_field_algebra_out(K.ctx, 15, VM, lc, p(chans), N ** 3, p(out))
    assert rc == -1 and "quantity 15" in lib.vps_last_error(K.ctx).decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all())
    for name in list(names.values()) + ["subgrid_flux"]:
        with pytest.raises(Exception, match="Unrecognized"):
            D.resolve_quantity(name[4:].lower() if name.startswith("VPS_") else name)
    with pytest.raises(ValueError, match="contiguous"):
        K.velocity_gradient(chans, N, lc, "vorticity", out=big[:6, :, :, ::2])


# ------------------------------------------------------------------ public surface ----
def _lattice_particles(N, L, seed, vel_of=None):
    """Eight particles per cell on the quarter-cell lattice (offsets 0.25 and 0.75 of a cell on every axis), unit density,
    velocities that are small integers (or vel_of(pos)): every NGP / CIC / TSC weight is dyadic, so every sum of the deposit is
    exact in float32 and the gridded fields do not depend on the order of the LDS adds."""
    lc = L / N
    g = (np.arange(2 * N) * 0.5 + 0.25) * lc
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(seed)
    vel = rng.integers(-3, 4, pos.shape).astype(np.float32) if vel_of is None else vel_of(pos).astype(np.float32)
    perm = rng.permutation(len(pos))
    return pos[perm], vel[perm], np.ones(len(pos), dtype=np.float32)


def _box_u(box):
    return np.ascontiguousarray(np.moveaxis(box.get_v(), 3, 0))


def _check_fields(box, label):
    """divergence / vorticity / strain_rate of a field against the float64 reference of its own get_v(), at the random-field bar."""
    got = {"divergence": box.divergence()[None], "vorticity": box.vorticity(), "strain_rate": box.strain_rate()}
    u = _box_u(box)
    bar = gr.error_bar(u, box.Lcell)
    for what, g in got.items():
        assert g.shape == (gr.NCH[what],) + (box.Nsize,) * 3 and g.dtype == np.float32, (label, what, g.shape, g.dtype)
        ref = gr.fields64(u, box.Lcell, what)
        worst = float(np.abs(g - ref).max() / bar)
        print("%s %s: worst error %.3f of the bar" % (label, what, worst))
        assert worst <= 1.0 and np.abs(ref).max() > 0, (label, what, worst)


def test_fields_of_every_kind_of_box(K):
    from vpower import interp
    rng = np.random.default_rng(5)
    N, n, L = 32, 60_000, 2.0
    pos = (rng.random((n, 3)) * L).astype(np.float32)
    vel = (rng.standard_normal((n, 3)) + np.array([1.0, -2.0, 0.5])).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    v = rng.standard_normal((N, N, N, 3)).astype(np.float32).astype(np.float64)
    _check_fields(interp.BoxField(v, np.ones((N, N, N)), L / N), "host-built")
    _check_fields(gp.ann_interp_to_field(N), "neighbour-backed")
    _check_fields(gp.deposit_to_field(N), "particle-backed ngp")
    for a in ("cic", "tsc"):
        _check_fields(gp.deposit_to_field(N, assignment=a, method="fused"), "particle-backed %s" % a)
        _check_fields(gp.deposit_to_field(N, assignment=a, method="direct"), "gridded %s" % a)


@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
def test_subgrid_flux_is_the_contraction_of_the_librarys_own_stress_and_strain(K, assignment):
    """Pi against -tau_ij S_ij in float64 of subgrid_stress() and strain_rate() of the same field, per cell within
    8 * 2^-24 * sum_ij |tau_ij S_ij| (one rounding per product, five per sum, the doubling exact: six).  The particles are exact
    inputs (every deposit sum exact), so the two deposits of tau give the same bits and the bar applies as it stands; Pi is the
    same bits between two calls."""
    from vpower import interp
    N, L = 32, 4.0
    pos, vel, rho = _lattice_particles(N, L, seed=7)
    gp = interp.GasParticles(pos, rho * (L / N) ** 3, rho, vel, L)
    box = gp.deposit_to_field(N) if assignment == "ngp" else gp.deposit_to_field(N, assignment=assignment, method="fused")
    flux = box.subgrid_flux()
    again = box.subgrid_flux()
    tau, S = box.subgrid_stress(), box.strain_rate()
    assert flux.shape == (N, N, N) and flux.dtype == np.float32 and np.isfinite(flux).all()
    assert np.array_equal(flux, again)
    ref, scale = gr.flux64(tau, S)
    worst = float(np.max(np.abs(flux - ref) / np.where(scale > 0, 8 * 2.0 ** -24 * scale, 1.0)))
    print("%s: Pi worst error %.3f of the bar; mean Pi %.6g, rms %.6g" % (assignment, worst, flux.mean(), flux.std()))
    assert worst <= 1.0 and np.all(flux[scale == 0] == 0) and np.abs(ref).max() > 0
    # S is the strain of the velocity gridded by the same assignment: the field's own
    u = _box_u(box)
    assert np.abs(S - gr.fields64(u, box.Lcell, "strain_rate")).max() <= gr.error_bar(u, box.Lcell)


def test_subgrid_flux_needs_the_particles(K):
    from vpower import interp
    rng = np.random.default_rng(2)
    n, L, N = 5000, 1.0, 16
    pos, vel = rng.random((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    host = interp.BoxField(np.ones((N, N, N, 3)), np.ones((N, N, N)), L / N)
    for box in (host, gp.ann_interp_to_field(N), gp.deposit_to_field(N, assignment="cic", method="direct")):
        with pytest.raises(Exception, match="subgrid_flux"):
            box.subgrid_flux()
    box = gp.deposit_to_field(N)
    box.divergence()                                   # the derivative fields keep the particles ...
    assert box.subgrid_flux().shape == (N, N, N)
    box.get_v()                                        # ... building the host grids lets go of them, as for subgrid_stress
    with pytest.raises(Exception, match="subgrid_flux"):
        box.subgrid_flux()
    assert box.divergence().shape == (N, N, N)


def test_shear_wave_from_particles(K):
    """CIC field of particles with v = (sin 2 pi y / L, 0, 0), eight per cell on the quarter-cell lattice.  The sine is
    quantised to multiples of 2^-6, so that every sum of the deposit is exact and the gridded u_x is the same number in every
    (x, z) column: what is tested is the derivative kernel and the plumbing, not the rounding of the deposit.  The divergence is
    zero to the random-field bar, d_y u_x is the sampled wave's, and the mean of Pi is finite and the same between two calls
    (tau_xy = 0 where v_y = 0 and S_xx = 0: this flow hands nothing down, Pi = 0)."""
    from vpower import interp
    N, L = 32, 2.0
    pos, vel, rho = _lattice_particles(N, L, seed=9, vel_of=lambda p: np.stack(
        (np.round(np.sin(2 * np.pi * p[:, 1].astype(np.float64) / L) * 64) / 64, 0 * p[:, 1], 0 * p[:, 1]), axis=1))
    gp = interp.GasParticles(pos, rho * (L / N) ** 3, rho, vel, L)
    box = gp.deposit_to_field(N, assignment="cic", method="fused")
    flux = [box.subgrid_flux(), box.subgrid_flux()]
    div, S = box.divergence(), box.strain_rate()
    u = _box_u(box)
    bar = gr.error_bar(u, box.Lcell)
    print("shear wave: max |div| %.3e (bar %.3e), max |S_xy| %.3e, mean Pi %r and %r" % (np.abs(div).max(), bar, np.abs(S[3]).max(),
                                                                                          float(flux[0].mean()), float(flux[1].mean())))
    assert np.abs(div).max() <= bar
    assert np.abs(S[3]).max() > 0.5 * np.sin(2 * np.pi / N) / box.Lcell * 0.5 and np.abs(u[0]).max() > 0.9
    assert np.isfinite(flux[0]).all() and np.isfinite(float(flux[0].mean())) and float(flux[0].mean()) == float(flux[1].mean())
    assert np.array_equal(flux[0], flux[1])
