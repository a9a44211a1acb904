"""Two-point correlation and structure functions on the MI355X: vps_fft_x modes 5 - 7 line by line, the whole pipeline on exact
and on random fields, the refusals and the stream contract.  Run:  python -m pytest tests/test_gpu_correlation.py -q -m gpu
Every case fails on a library without the modes ("mode must be 0..4").  References: tests/correlation_ref.py (float64 numpy).

Bars
  SHELL_BAR      2e-5: the project's shell-sum bar, |S - S_ref| <= 2e-5 sum w |Re F| per shell.  The normaliser is the shell's
                 ABSOLUTE sum: cancellation in a signed sum cannot hide an error.
  FIELD_BAR      1e-5 of the largest reference value: the bar tests/test_gpu_guarded.py holds mode 2 (vps_power_grid) to.
  XI_EXACT_BAR   2e-5 xi(0) per shell for the analytic cases: the shell-sum bar again, against xi(0) because a shell mean of a
                 signed function can vanish.  Two float32 transforms in a row each add an error of a few 1e-7 of the largest
                 value (tests/test_gpu_parity.py: FFT_RTOL 3e-6 per mode), and the largest value of the second one is xi(0) N^3.
  XI_BAR         random fields, |xi - xi_ref| / xi(0) per shell against the float64 reference fed the same float32 fields:
                 four times the worst value measured on an MI355X over the routes and sizes of test_random_fields (the margin
                 covers the summation-order freedom of the LDS atomics).  structure_function: the same bar against 2 xi(0).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import correlation_ref as cref

gpu = pytest.mark.gpu
pytestmark = gpu

L = 1.0
SHELL_BAR = 2e-5
FIELD_BAR = 1e-5
XI_EXACT_BAR = 2e-5
XI_BAR_MEASURED = 1.7e-7      # worst |xi - xi_ref| / xi(0) seen on an MI355X over test_random_fields
XI_BAR = 4 * XI_BAR_MEASURED
ALL_N = [16, 32, 96, 250, 1024, 1536, 2000, 2048, 4096]
SMALL_N = [16, 32, 96, 250]
CASES = {"plane": lambda N: (0, N, 3), "nyquist": lambda N: (0, N, N // 2), "partial": lambda N: (N // 2 + 1, N // 4, 3)}
CACHE = {}


@pytest.fixture(scope="module")
def K():
    import torch
    from vpower import device
    k = device.HipKernels()
    yield k
    k.close()
    CACHE.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def G():
    import torch
    import guarded
    g = guarded.guarded_kernels()
    yield g
    g.release()
    g.close()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def options(opts):
    from vpower import _ffi
    with contextlib.ExitStack() as stack:
        for k, v in opts.items():
            stack.enter_context(_ffi.option(k, v))
        yield
    for k in opts:
        assert k not in _ffi.OPTIONS, k


def _lines(K, N, seed=0):
    """Random complex64 lines of one plane [N][N], their float64 transform and the device copy; one N (and seed) at a time."""
    key = ("lines", N, seed)
    if key not in CACHE:
        for k in [k for k in CACHE if k[0] in ("lines", "r")]:
            del CACHE[k]
        rng = np.random.default_rng(1000 * seed + N)
        h = (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))).astype(np.complex64)
        CACHE[key] = (K.to_device(h), cref.line_transform(h))
    return CACHE[key]


def _edges(N, table):
    Lcell = L / N
    return cref.default_edges(L, N) if table == "default" else cref.band_edges(L, N, 2.5 * Lcell, 0.4 * L, Lcell)


def _set_tables(K, N, table):
    from vpower import device as D
    Lcell = L / N
    edges = D.radial_edges(L, N) if table == "default" else D.radial_edges(L, N, rmin=2.5 * Lcell, rmax=0.4 * L, rres=Lcell)
    assert np.array_equal(edges, _edges(N, table))
    K.set_binning(*D.binning_tables(D.r_axis(L, N), edges))
    K.set_window(N, None)
    return edges


def _expected_mode(table, opts):
    """default edges lie on integer multiples of Lcell: integer shells are declined; the band's edges are half-integers."""
    if opts.get("no_fast_binning"):
        return 0
    return 2 if (table == "band" and not opts.get("no_int_binning")) else 1


# ------------------------------------------------------------------------------ modes 6 / 7, line level ----
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("N", ALL_N)
def test_signed_binning_lines(K, N, case):
    import torch
    dev, F = _lines(K, N)
    line0, nl, kz0 = CASES[case](N)
    r = cref.line_r(L, N, nl, line0, kz0)
    worst = 0.0
    for table in ("default", "band"):
        edges = _edges(N, table)
        nb = len(edges) - 1
        s_ref, c_ref, a_ref = cref.line_shells(F[:nl], r, N, nl, line0, kz0, edges)
        assert c_ref.sum() > 0 or (case == "nyquist" and table == "band")      # (the band ends at 0.4 L: no lag of the plane L/2 falls into it)
        for opts in ([{}] + ([{"no_fast_binning": 1}, {"no_pair_binning": 1}, {"no_int_binning": 1}] if N <= 250 else [])):
            with options(opts):
                _set_tables(K, N, table)
                assert K.binning_mode() == _expected_mode(table, opts), (table, opts, K.binning_mode())
                ps6, ns6 = K.zeros((nb,), torch.float64), K.zeros((nb,), torch.int64)
                K.fft_x_mode(dev[:nl], N, nl, line0, kz0, 6, psum=ps6, nsample=ns6)
                ps7, ns7 = K.zeros((nb,), torch.float64), torch.full((nb,), 12345, dtype=torch.int64, device=K.device)
                K.fft_x_mode(dev[:nl], N, nl, line0, kz0, 7, psum=ps7, nsample=ns7)
                K.fft_x_mode(dev[:nl], N, nl, line0, kz0, 7, psum=ps7, nsample=None)      # (mode 7 takes no count accumulator)
            assert np.array_equal(ns6.cpu().numpy(), c_ref), (N, case, table, opts)
            assert bool((ns7 == 12345).all()), "mode 7 touched nsample_dev"
            for got, mult in ((ps6, 1.0), (ps7, 2.0)):
                err = np.abs(got.cpu().numpy() - mult * s_ref)
                nz = a_ref > 0
                assert np.all(err[~nz] == 0)
                ratio = float(np.max(err[nz] / (mult * a_ref[nz]), initial=0.0))
                worst = max(worst, ratio)
                assert ratio <= SHELL_BAR, (N, case, table, opts, ratio)
    print("modes 6/7 N=%d %s: worst |S - S_ref| / sum w|Re F| = %.3g" % (N, case, worst))


# ------------------------------------------------------------------------------ mode 5, line level ----
def _mirror(plane):
    """plane[(N - ky) % N][(N - kx) % N]"""
    import torch
    return torch.roll(torch.flip(plane, (0, 1)), (1, 1), (0, 1))


def _mode5(Kx, lines, N, nl, line0, kz0, base_ptr):
    Kx._stream()
    Kx._chk(Kx.lib.vps_fft_x(Kx.ctx, N, nl, line0, kz0, Kx._ptr(lines), 1, 0, 5, None, None, C.c_void_p(base_ptr)))


@pytest.mark.parametrize("N", ALL_N)
def test_power_into_the_full_grid(G, N):
    """Whole grids up to 250; beyond, a window of the three planes N/2 - 1, N/2, N/2 + 1 (the plane N/2 - 1 and its partner
    N/2 + 1 around the Nyquist plane), addressed through a base pointer 'N/2 - 1 planes in front of it' -- the mode touches
    the planes kz and N - kz of a call and nothing else, and the 1 MiB guards on both sides of the window would show it.
    The output is a guarded ZERO buffer, not a poisoned one: the mode accumulates, and a stray store inside the buffer shows
    as a non-zero element where the reference holds none."""
    import torch
    dev, F = _lines(G, N)
    whole = N <= 250
    first = 0 if whole else N // 2 - 1
    nplanes = N if whole else 3
    kzp = 3 if whole else N // 2 - 1
    with G.sequence():
        grid = G.zeros((nplanes, N, N), torch.float32)
        base = grid.data_ptr() - first * N * N * 4
        calls = [(0, N, kzp), (0, N, N // 2), (N // 2 + 1, N // 4, (5 if whole else kzp))] + ([(0, N, 0)] if whole else [])
        ref = {p: np.zeros((N, N)) for p in range(first, first + nplanes)}
        for line0, nl, kz0 in calls:
            _mode5(G, dev[:nl], N, nl, line0, kz0, base)
            for p, v in cref.line_power_full(F[:nl], N, nl, line0, kz0, [q for q in (kz0, N - kz0) if q in ref]).items():
                ref[p] += v
        once = grid.clone()
        # a second component accumulates: the same whole plane again
        _mode5(G, dev, N, N, 0, kzp, base)
        for p, v in cref.line_power_full(F, N, N, 0, kzp, [kzp, N - kzp]).items():
            ref[p] += v
        torch.cuda.synchronize()
    import guarded
    assert guarded.guard_findings(G.check()) == []
    got = grid.cpu().numpy().astype(np.float64)
    scale = max(float(v.max()) for v in ref.values())
    worst = max(float(np.max(np.abs(got[p - first] - ref[p]))) for p in ref) / scale
    print("mode 5 N=%d: worst |P - P_ref| / max P_ref = %.3g" % (N, worst))
    assert worst <= FIELD_BAR
    touched = [p for p in ref if ref[p].any()]
    for p in ref:
        if p not in touched:
            assert not got[p - first].any(), "plane %d was written" % p
    # plane kz and its partner N - kz: bit for bit the same values at k and -k
    a, b = kzp - first, (N - kzp) - first
    assert torch.equal(grid[b], _mirror(grid[a])) and torch.equal(once[b], _mirror(once[a]))
    # the Nyquist plane (and kz = 0) carries every mode once: what one call added is |F|^2, not twice it, and no mirror moved
    nyq = once[N // 2 - first].cpu().numpy().astype(np.float64)
    nyq_ref = cref.line_power_full(F, N, N, 0, N // 2, [N // 2])[N // 2]
    assert np.max(np.abs(nyq - nyq_ref)) <= FIELD_BAR * scale
    assert float(grid.sum(dtype=torch.float64)) > float(once.sum(dtype=torch.float64))


# ------------------------------------------------------------------------------ whole pipeline, exact cases ----
def _pipeline(K, fields, N, subtract_mean=True, **kw):
    from vpower import device as D
    from vpower.spctrm import CorrelationFunction
    pipe = D.CorrelationPipeline(N, L, kernels=K, **kw)
    tab, xi0 = pipe.correlation([K.to_device(np.ascontiguousarray(f, dtype=np.float32)) for f in fields], subtract_mean=subtract_mean)
    return CorrelationFunction(tab, xi0), pipe


@pytest.mark.parametrize("N", SMALL_N)
def test_plane_wave(K, N):
    i = np.arange(N)
    ph = (1 * i[:, None, None] + 2 * i[None, :, None] + 3 * i[None, None, :]) % N
    f = np.cos(2 * np.pi * ph / N)
    cf, pipe = _pipeline(K, [f], N)
    planes = np.arange(N // 2 + 1)
    xi_an = 0.5 * np.cos(2 * np.pi * ph[: N // 2 + 1] / N)
    sm, cnt, _ = cref.shells(cref.lattice_r(L, N, planes), xi_an, cref.hermitian_weight(N, planes)[:, None, None], pipe.edges)
    assert np.array_equal(cf.Nsample, cnt) and cnt[0] == 1
    err = np.max(np.abs(cf.xi - sm / cnt)) / 0.5
    print("plane wave N=%d: worst |xi - xi_analytic| / xi(0) = %.3g, xi0 - 1/2 = %.3g" % (N, err, cf.xi0 - 0.5))
    assert err <= XI_EXACT_BAR and abs(cf.xi0 - 0.5) <= XI_EXACT_BAR * 0.5
    s2 = cf.structure_function()
    assert s2[0, 1] == 0.0 and cf.xi[0] == cf.xi0
    assert np.max(np.abs(s2[:, 1] - 2 * (0.5 - sm / cnt))) <= XI_EXACT_BAR * 1.0


@pytest.mark.parametrize("N", SMALL_N)
def test_constant_field_and_single_cell(K, N):
    c = 2.5
    f = np.full((N, N, N), c)
    on, _ = _pipeline(K, [f], N, subtract_mean=True)
    off, _ = _pipeline(K, [f], N, subtract_mean=False)
    print("constant N=%d: max |xi| (mean removed) = %.3g, max |xi - c^2| / c^2 (mean kept) = %.3g"
          % (N, np.max(np.abs(on.xi)), np.max(np.abs(off.xi - c * c)) / (c * c)))
    assert np.max(np.abs(on.xi)) <= XI_EXACT_BAR * c * c and abs(on.xi0) <= XI_EXACT_BAR * c * c
    assert np.max(np.abs(off.xi - c * c)) <= XI_EXACT_BAR * c * c and abs(off.xi0 - c * c) <= XI_EXACT_BAR * c * c
    assert on.structure_function()[0, 1] == 0.0 and off.structure_function()[0, 1] == 0.0
    # one non-zero cell: xi = a^2 / N^3 at r = 0 and nothing elsewhere; edges that reach beyond sqrt(3) L / 2 count every lag
    a = 3.0
    g = np.zeros((N, N, N))
    g[1, N // 2, N - 1] = a
    Lcell = L / N
    cell, pipe = _pipeline(K, [g], N, subtract_mean=False, rmax=np.sqrt(3) * L / 2 + Lcell)
    xi0 = a * a / N ** 3
    assert cell.Nsample[0] == 1 and cell.Nsample.sum() == N ** 3
    planes = np.arange(N // 2 + 1)
    cnt = cref.shells(cref.lattice_r(L, N, planes), np.zeros((len(planes), N, N)), cref.hermitian_weight(N, planes)[:, None, None], pipe.edges)[1]
    assert np.array_equal(cell.Nsample, cnt)
    print("single cell N=%d: xi0 / (a^2 / N^3) - 1 = %.3g, max |xi(r > 0)| / xi(0) = %.3g"
          % (N, cell.xi0 / xi0 - 1, np.max(np.abs(cell.xi[1:])) / xi0))
    assert abs(cell.xi0 - xi0) <= XI_EXACT_BAR * xi0 and cell.xi[0] == cell.xi0
    assert np.max(np.abs(cell.xi[1:])) <= XI_EXACT_BAR * xi0
    assert cell.structure_function()[0, 1] == 0.0


# ------------------------------------------------------------------------------ whole pipeline, random fields ----
def _particles():
    if "gp" not in CACHE:
        from vpower import interp, synth
        pos, vel, mass, dens = synth.particles(7, 300_000, L)
        CACHE["gp"] = interp.GasParticles(pos, mass, dens, vel, L)
    return CACHE["gp"]


def _box(route, N):
    from vpower import interp
    gp = _particles()
    if route == "host":
        b = gp.deposit_to_field(N)
        return interp.BoxField(b.get_v().astype(np.float32), b.mass.astype(np.float32), b.Lcell), "velocity"
    if route == "ngp":
        return gp.deposit_to_field(N), "velocity"
    if route == "cic":
        return gp.deposit_to_field(N, assignment="cic", method="fused"), "velocity"
    if route == "nn":
        return gp.ann_interp_to_field(N), "velocity"
    return gp.deposit_to_field(N), "dispersion"


@pytest.mark.parametrize("route", ["host", "ngp", "cic", "nn", "dispersion"])
@pytest.mark.parametrize("N", [32, 96])
def test_random_fields(monkeypatch, N, route):
    """BoxField.correlation / structure_function of the velocity of synth particles by every route, against the float64 reference
    fed the very float32 fields the route handed to the pipeline (recorded on the way in)."""
    from vpower import device as D
    seen = []
    inner = D.CorrelationPipeline.correlation

    def recording(self, fields, subtract_mean=True):
        seen.append([f.cpu().numpy() for f in fields])
        return inner(self, fields, subtract_mean=subtract_mean)
    monkeypatch.setattr(D.CorrelationPipeline, "correlation", recording)
    worst = 0.0
    for mean in (True, False):
        box, quantity = _box(route, N)
        cf = box.correlation(quantity, subtract_mean=mean)
        xr, cnt, xi0 = cref.correlation(seen[-1], box.Lbox, subtract_mean=mean)
        assert len(seen[-1]) == (1 if route == "dispersion" else 3)
        assert np.array_equal(cf.Nsample, cnt) and len(cf) == N // 2
        e = max(float(np.max(np.abs(cf.xi - xr))), abs(cf.xi0 - xi0)) / xi0
        worst = max(worst, e)
        s2 = cf.structure_function()
        e2 = float(np.max(np.abs(s2[:, 1] - 2 * (xi0 - xr)))) / (2 * xi0)
        worst = max(worst, e2)
        assert s2[0, 1] == 0.0
    if route == "host":        # the public shorthand: the same table as correlation(...).structure_function()
        s2 = box.structure_function(quantity)
        assert s2.shape == (N // 2, 3) and s2[0, 1] == 0.0 and np.array_equal(s2[:, 2], cnt)
        worst = max(worst, float(np.max(np.abs(s2[:, 1] - 2 * (xi0 - xr)))) / (2 * xi0))
    print("random N=%d %s: worst |xi - xi_ref| / xi(0) (and S2 / 2 xi(0)) = %.3g" % (N, route, worst))
    assert worst <= XI_BAR, (N, route, worst)


# ------------------------------------------------------------------------------ refusals ----
def test_refusals_leave_the_context_usable(K):
    import torch
    from vpower import device as D, interp
    N = 32
    dev, F = _lines(K, N)
    edges = _set_tables(K, N, "default")
    nb = len(edges) - 1
    ps, ns = K.zeros((nb,), torch.float64), K.zeros((nb,), torch.int64)
    out = K.zeros((N, N, N), torch.float32)

    def call(mode, nseg=1, psum=ps, nsample=ns, o=None, kz0=3):
        K._stream()
        rc = K.lib.vps_fft_x(K.ctx, N, N, 0, kz0, K._ptr(dev), nseg, 0, mode, K._ptr(psum), K._ptr(nsample), K._ptr(o))
        return rc, K.lib.vps_last_error(K.ctx).decode()

    def usable():
        p2, n2 = K.zeros((nb,), torch.float64), K.zeros((nb,), torch.int64)
        K.fft_x_mode(dev, N, N, 0, 3, 6, psum=p2, nsample=n2)
        assert int(n2.sum()) == 2 * (cref.line_r(L, N, N, 0, 3) <= edges[-1]).sum()

    rc, msg = call(8)
    assert rc == -1 and "0..7" in msg
    usable()
    rc, msg = call(5, nseg=2, o=out)
    assert rc == -1 and "nseg" in msg
    assert not bool(out.any())
    rc, msg = call(5, o=out, kz0=N // 2 + 1)
    assert rc == -1 and not bool(out.any())
    rc, msg = call(5, o=None)
    assert rc == -1
    for mode in (6, 7):
        rc, msg = call(mode, nseg=2)
        assert rc == -1 and "nseg" in msg
        K.set_window(N, D.window_inv2_axis(N, "cic"))
        rc, msg = call(mode)
        K.set_window(N, None)
        assert rc == -1 and "window" in msg
    rc, msg = call(6, nsample=None)
    assert rc == -1 and "accumulator" in msg
    rc, msg = call(7, psum=None)
    assert rc == -1 and "accumulator" in msg
    assert not bool(ps.any()) and not bool(ns.any())
    usable()
    # the public surface: the refusals of spctrm, by name
    v = np.zeros((16, 16, 16, 3), dtype=np.float32)
    box = interp.BoxField(v, np.ones((16, 16, 16), dtype=np.float32), L / 16)
    with pytest.raises(Exception, match="dispersion"):
        box.correlation("dispersion")
    with pytest.raises(ValueError, match="density_weight"):
        box.correlation("energy", density_weight=0.5)
    with pytest.raises(Exception, match="Unrecognized"):
        box.structure_function("vorticity")

    class TwoRanks:
        world, rank = 2, 0
    with pytest.raises(Exception, match="x-slabs"):
        D.CorrelationPipeline(32, L, kernels=K, comm=TwoRanks())
    usable()


# ------------------------------------------------------------------------------ stream ----
def test_modes_enqueue_on_a_side_stream(K):
    """Modes 5 - 7 behind a busy blocker on a side stream: the calls return while it is pending, and what is read after a
    synchronisation matches the null stream's result (counts and the mode-5 grid bit for bit)."""
    import torch
    N = 96
    dev, F = _lines(K, N)
    edges = _set_tables(K, N, "default")
    nb = len(edges) - 1
    sleep = getattr(torch.cuda, "_sleep", None)
    assert sleep is not None

    def timed(units):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        sleep(int(units))
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)
    timed(10_000_000)
    units = int(10_000_000 * 200.0 / max(timed(10_000_000), 1e-3))      # a blocker of about 200 ms

    def run():
        ps6, ns6 = K.zeros((nb,), torch.float64), K.zeros((nb,), torch.int64)
        ps7 = K.zeros((nb,), torch.float64)
        grid = K.zeros((N, N, N), torch.float32)
        K.fft_x_mode(dev, N, N, 0, 3, 6, psum=ps6, nsample=ns6)
        K.fft_x_mode(dev, N, N, 0, 3, 7, psum=ps7)
        K.fft_x_mode(dev, N, N, 0, 3, 5, out=grid)
        return ps6, ns6, ps7, grid
    null = run()                                   # (also the warm-up: tables, twiddles and partial sums exist)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=K.device)
    with torch.cuda.stream(side):
        sleep(units)
        behind = torch.cuda.Event()
        behind.record(side)
        got = run()
        assert not behind.query(), "a mode waited for the stream (or the blocker was too short)"
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(got[1], null[1]) and int(got[1].sum()) > 0
    assert torch.equal(got[3], null[3]) and bool(got[3].any())
    s_ref, c_ref, a_ref = cref.line_shells(F, cref.line_r(L, N, N, 0, 3), N, N, 0, 3, edges)
    assert np.array_equal(got[1].cpu().numpy(), c_ref)
    for g in (got[0], got[2]):
        assert np.all(np.abs(g.cpu().numpy() - s_ref) <= SHELL_BAR * a_ref)
