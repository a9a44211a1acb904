"""Shell parity of every binning route under custom k ranges (kmin, kmax, kres of PowerPipeline, BoxField.spctrm and
BoxField.helmholtz_spctrm) against the exact separable references, as tests/test_gpu_spectrum_matrix.py and
tests/test_gpu_helmholtz.py hold the default range.

Everything the binning passes skip or pack is a function of the k range: the row cut of a binning-only scope, the tile skip of
the paired x pass, the packed slots of the chunked exchange, the float first guess with its clamps, the choice between
integer and float64 shells and the LDS carve-up.  The rows of gpu_checks.K_RANGES reach each of them (a deep cut, a band above
the fundamental, a first edge at exactly 0, bin counts from 2 to ~N); tests/test_separable_reference.py pins the references at
these thresholds to the oracle and asserts, without a GPU, that every (N, row) used here has the geometry it is there for.
Legs:
  a. whole grid, every row x every x-pass variant: the binning mode the documented rule gives (derived on the host, never read
     back), counts bit for bit, Psum within PSUM_RTOL, empty bins exactly 0;
  b. the Helmholtz decomposition of the same rows;
  c. CIC and TSC window tables with `deep` and `band`;
  d. the slab exchange emulated on one GPU, every receiver, NaN-prefilled send buffers, after the packed geometry has been
     restated on the host (block sizes, mixed / dead / unequal / full slots);
  e. the user-facing routes at N = 128 against the float64 oracle (parallel_optimized.py has no k-range flags: not a route);
  f. the limits: 8193 bins and an x pass beyond the LDS are refused cleanly."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import helmholtz_ref as hr  # noqa: E402
from oracle import gpu_checks as chk  # noqa: E402
from oracle import vps_oracle as orc  # noqa: E402
from test_gpu_helmholtz import _check as _check_helmholtz  # noqa: E402
from test_gpu_spectrum_matrix import PSUM_RTOL, RANK, VARIANTS, _check_table, _free, _nan_buffer  # noqa: E402

WHOLE_1024_VARIANTS = ("default", "no_fast_binning")
HELMHOLTZ_VARIANTS = ("default", "no_int_binning", "no_fast_binning")
WINDOW_VARIANTS = ("default", "no_fast_binning")
HELMHOLTZ_SLABS = ((256, 8, 2), (1024, 16, 2))


@pytest.fixture(scope="module")
def K():
    from vpower import device
    k = device.default_kernels()
    torch.cuda.reset_peak_memory_stats()
    yield k
    print("\ntest_gpu_krange_matrix: peak device memory %.1f GB" % (torch.cuda.max_memory_allocated() / 1e9))


def _factors(N, ncomp, salt):
    return [chk.separable_factors(N, RANK, seed=3000 * N + 10 * salt + i) for i in range(ncomp)]


_FIELDS = {}


def _fields(K, N, ncomp, salt):
    """The float32 fields of _factors(N, ncomp, salt), kept for the rows of one N (one entry: the next N frees them)."""
    key = (N, ncomp, salt)
    if key not in _FIELDS:
        _FIELDS.clear()
        _free(K)
        comps = _factors(N, ncomp, salt)
        _FIELDS[key] = (comps, [chk.separable_slab(K.device, f, 0, N) for f in comps])
    return _FIELDS[key]


def _pipeline(K, N, name, deconvolve=None):
    from vpower import device
    L = chk.k_range_box(name, N)
    flavour, kmin, kmax, kres = chk.k_range(name, N, L)
    return device.PowerPipeline(N, L, kernels=K, comm=device.SlabComm(enabled=False), flavour=flavour, kmin=kmin, kmax=kmax,
                                kres=kres, deconvolve=deconvolve)


def _mode(pipe, opts):
    """The mode vps_set_binning must select for the pipeline's tables under `opts`: the documented rule, on the host."""
    if opts.get("no_fast_binning"):
        return 0
    mode = chk.expected_binning_mode(pipe.N, pipe.k2, pipe.thr, pipe.edges)
    return min(mode, 1) if opts.get("no_int_binning") else mode


def _variants(names=None):
    return [v for v in VARIANTS if names is None or v[0] in names]


def _run(K, pipe, opts, call):
    """pipe.prepare() under `opts`, the binning mode asserted, then call(); the options are restored."""
    from vpower import _ffi
    try:
        for k_, v_ in opts.items():
            _ffi.set_option(k_, v_)
        pipe.prepare()
        assert K.binning_mode() == _mode(pipe, opts), (opts, K.binning_mode(), _mode(pipe, opts))
        return call()
    finally:
        for k_ in opts:
            _ffi.set_option(k_, None)


def _empty_bins_are_zero(tab, counts, what):
    empty = counts == 0
    assert np.all(tab[empty, 2] == 0.0) and np.all(tab[empty, 3] == 0.0), what


# ------------------------------------------------------------------ a. whole grid, every row x every x-pass variant ----
@pytest.mark.parametrize("N,name", [(N, name) for N, names in chk.K_WHOLE.items() for name in names])
def test_whole_grid_every_row_every_variant(K, N, name):
    comps, fields = _fields(K, N, 3 if N <= 256 else 1, 0)
    pipe = _pipeline(K, N, name)
    counts = chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr)
    ref_ps, ref_ns = chk.separable_shell_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
    assert np.array_equal(ref_ns, counts) and counts.sum() > 0
    for vname, opts, _ in _variants(WHOLE_1024_VARIANTS if N == 1024 else None):
        tab = _run(K, pipe, opts, lambda: pipe.finish(*pipe.accumulate(fields)))
        _check_table(tab, ref_ps, counts, (N, name, vname))
        _empty_bins_are_zero(tab, counts, (N, name, vname))


# ------------------------------------------------------------------------------------------------- b. Helmholtz ----
@pytest.mark.parametrize("N,name", [(N, name) for N, names in chk.K_HELMHOLTZ.items() for name in names])
def test_helmholtz_every_row(K, N, name):
    comps, fields = _fields(K, N, 3, 1)
    pipe = _pipeline(K, N, name)
    ref = hr.separable_helmholtz_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
    counts = chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr)
    assert np.array_equal(ref[2], counts)
    if name == "zero":
        # bin 0 = [0, kf) holds the k = 0 mode alone.  Its k' is 0, so under the documented rule (P_comp = 0 where k' = 0,
        # PowerPipeline.finish_helmholtz) its compressive share is exactly 0 and all of its power is solenoidal
        assert pipe.thr[0] == 0.0 and counts[0] == 1 and ref[1][0] == 0.0 and ref[0][0] > 0.0
    for vname, opts, _ in _variants(HELMHOLTZ_VARIANTS):
        tabs = _run(K, pipe, opts, lambda: pipe.finish_helmholtz(*pipe.accumulate_helmholtz(fields)))
        _check_helmholtz(tabs, ref, (N, name, vname))
        for t in tabs[:2]:
            _empty_bins_are_zero(t, counts, (N, name, vname))
        if name == "zero":
            assert tabs[1][0, 2] == 0.0 and tabs[2][0, 2] == tabs[0][0, 2]


# ---------------------------------------------------------------------------------------------------- c. window ----
@pytest.mark.parametrize("N,name", [(N, name) for N, names in chk.K_WINDOW.items() for name in names])
def test_window_tables_every_row(K, N, name):
    comps, fields = _fields(K, N, 3 if N <= 256 else 1, 0)
    for assignment in ("cic", "tsc"):
        pipe = _pipeline(K, N, name, deconvolve=assignment)
        counts = chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr)
        ref_ps, ref_ns = chk.separable_shell_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr, win=pipe.window)
        assert np.array_equal(ref_ns, counts)
        for vname, opts, _ in _variants(WINDOW_VARIANTS):
            tab = _run(K, pipe, opts, lambda: pipe.finish(*pipe.accumulate(fields)))
            _check_table(tab, ref_ps, counts, (N, name, assignment, vname))
        if N == 256 and assignment == "cic":
            ref = hr.separable_helmholtz_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr, win=pipe.window)
            tabs = _run(K, pipe, {}, lambda: pipe.finish_helmholtz(*pipe.accumulate_helmholtz(fields)))
            _check_helmholtz(tabs, ref, (N, name, assignment, "helmholtz"))
    pipe = _pipeline(K, N, name)
    pipe.prepare()                    # (the window table is part of the context: leave it switched off)


# ------------------------------------- d. slab decomposition emulated on one GPU, production calls, packed geometry ----
def _assert_packed_geometry(K, pipe, name, N, G, C):
    """The cut restated on the host (gpu_checks.row_cut) and what the row is in this leg for; inside a binning_only scope."""
    nx = N // G
    kcut = chk.row_cut(N, pipe.k2, pipe.thr)
    assert K.y_packed(N)
    for c in range(C):
        assert K.chunk_block(N, nx, G, C, c, True) == chk.packed_block(kcut, N, nx, G, C, c), (name, N, G, C, c)
    mix = chk.slot_mix(kcut, N, G, C)
    if name == "corner":
        assert mix["full"] == mix["slots"]
    if name == "band" or (name == "deep" and (N, G, C) != (128, 4, 2)):
        assert mix["mixed"] >= 1
    if name in ("deep", "band"):
        assert mix["dead"] >= 1
    if name == "zero":
        assert mix["unequal"] >= 1


def _exchange(K, pipe, name, comps, N, G, C, helmholtz):
    """vps_fft_z per sender slab -> vps_fft_y chunk by chunk into NaN-filled send buffers, packed rows inside binning_only()
    -> the all-to-all played by slicing -> the chunk x pass on every receiver.  -> the finished table(s)."""
    nx = N // G
    pipe.prepare()
    with K.binning_only():
        _assert_packed_geometry(K, pipe, name, N, G, C)
    zimgs = []
    for f in comps:
        zimgs.append([])
        for g in range(G):
            slab = chk.separable_slab(K.device, f, g * nx, nx)
            zimgs[-1].append(K.fft_z(slab, N, nx))
            del slab
    acc = pipe.new_accumulators(helmholtz=helmholtz)
    for c in range(C):
        with K.binning_only():
            packed = K.y_packed(N)
            blk = K.chunk_block(N, nx, G, C, c, packed)
            sends = [[K.fft_y_chunk(z, N, nx, G, C, c, out=_nan_buffer(K, G * blk)) for z in zc] for zc in zimgs]
        assert packed
        for h in range(G):
            recv = [torch.cat([s[g][h * blk:(h + 1) * blk] for g in range(G)]) for s in sends]
            if helmholtz:
                K.fft_x_bin_chunk_helmholtz(recv, N, nx, G, C, c, h, packed, acc[0], acc[1], acc[2])
            else:
                K.fft_x_bin_chunk(recv, N, nx, G, C, c, h, packed, acc[0], acc[1])
            del recv
        del sends
    del zimgs
    return pipe.finish_helmholtz(*acc) if helmholtz else pipe.finish(*acc)


@pytest.mark.parametrize("N,G,C", chk.K_SLABS)
@pytest.mark.parametrize("name", chk.K_SLAB_ROWS)
def test_emulated_slab_exchange_every_receiver(K, name, N, G, C):
    _FIELDS.clear()
    comps = _factors(N, 1, 2)
    pipe = _pipeline(K, N, name)
    counts = chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr)
    ref_ps, ref_ns = chk.separable_shell_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
    assert np.array_equal(ref_ns, counts)
    tab = _exchange(K, pipe, name, comps, N, G, C, False)
    _check_table(tab, ref_ps, counts, (name, N, G, C))
    _empty_bins_are_zero(tab, counts, (name, N, G, C))
    _free(K)


@pytest.mark.parametrize("N,G,C", HELMHOLTZ_SLABS)
@pytest.mark.parametrize("name", ("deep", "band"))
def test_emulated_slab_exchange_helmholtz(K, name, N, G, C):
    _FIELDS.clear()
    comps = _factors(N, 3, 3)
    pipe = _pipeline(K, N, name)
    ref = hr.separable_helmholtz_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
    assert np.array_equal(ref[2], chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr))
    _check_helmholtz(_exchange(K, pipe, name, comps, N, G, C, True), ref, (name, N, G, C))
    _free(K)


# --------------------------------------------------------------------------- e. user-facing routes at N = 128 ----
ROUTE_N = 128


@pytest.fixture(scope="module")
def routes():
    """float64 power grids of the three routes' float64 gridding references (the ones tests/test_gpu_parity.py and
    tests/test_gpu_helmholtz.py use), computed once: {key: P grid}, plus the objects the routes start from."""
    from helpers import synth
    from vpower import interp
    N, L = ROUTE_N, chk.k_range_box("deep", ROUTE_N)
    assert all(chk.k_range_box(name, N) == L for name in chk.K_ROUTE_ROWS)
    out = {"L": L}
    pos, vel, mass, dens = synth(128, 300000, L)
    out["gp"] = interp.GasParticles(pos, mass, dens, vel, L)
    vec = orc.density_velocity_vector(vel.astype(np.float64), dens.astype(np.float64))
    v, m = orc.vm_from_vec_grid(orc.deposit_to_grid_fast(vec, pos, N, L), L / N, zero_empty=True)
    out["velocity"] = orc.vector_power(v[..., 0], v[..., 1], v[..., 2], L, N)
    out["energy"] = orc.scalar_power(orc.kinetic_energy_field(v[..., 0], v[..., 1], v[..., 2], m), L, N)
    pos, vel, mass, dens = synth(57, 3000, L)
    out["gp_nn"] = interp.GasParticles(pos, mass, dens, vel, L)
    ax = orc.lattice_axes_library(L, N)
    grid, _ = orc.ann_interpolate(pos, (ax, ax, ax), orc.density_velocity_vector(vel.astype(np.float64), dens.astype(np.float64)), N)
    v, m = orc.vm_from_vec_grid(grid, L / N)
    out["nn_momentum"] = orc.vector_power(*orc.momentum_fields(v[..., 0], v[..., 1], v[..., 2], m), L, N)
    rng = np.random.default_rng(N)
    v = rng.standard_normal((N, N, N, 3)).astype(np.float32).astype(np.float64)
    m = np.exp(0.3 * rng.standard_normal((N, N, N))).astype(np.float32).astype(np.float64)
    out["box"] = interp.BoxField(v, m, L / N)
    out["helm_tot"], out["helm_comp"] = hr.helmholtz_power(v[..., 0], v[..., 1], v[..., 2], L, N)
    return out


@pytest.mark.parametrize("name", chk.K_ROUTE_ROWS)
def test_user_facing_routes_take_the_k_range(K, routes, name):
    """kmin, kmax, kres of the row through GasParticles.deposit_to_field(N).spctrm (the fused pencil route),
    ann_interp_to_field(N).spctrm and a grid-backed BoxField.helmholtz_spctrm, against orc.spectrum_table of the float64
    power grids: k and Nsample equal, Psum within the bar each route has in its own test file (2e-5 everywhere; the Helmholtz
    tables with the floor 2e-5 of the total per shell, tests/test_gpu_helmholtz.py)."""
    N, L = ROUTE_N, routes["L"]
    _, kmin, kmax, kres = chk.k_range(name, N, L)
    kw = dict(kmin=kmin, kmax=kmax, kres=kres)

    def ref_of(P):
        return orc.spectrum_table(P, L, N, "library", kmin, kmax, kres)

    def agree(sp, ref, what, floor=None):
        assert np.array_equal(np.asarray(sp.k), ref[:, 0]), what
        assert np.array_equal(np.asarray(sp.Nsample), ref[:, 3]), what
        err = np.abs(np.asarray(sp.Psum) - ref[:, 2])
        bar = PSUM_RTOL * np.abs(ref[:, 2]) + (0 if floor is None else PSUM_RTOL * floor)
        print(what, "worst Psum error / bar: %.3g" % np.max(err / np.maximum(bar, 1e-300)))
        assert np.all(err <= bar), (what, np.nonzero(err > bar)[0][:8])

    for q in ("velocity", "energy"):
        box = routes["gp"].deposit_to_field(N)
        sp = box.spctrm(q, **kw)
        assert box._src is not None and box._chans is None          # the fused route: no grid was made
        agree(sp, ref_of(routes[q]), (name, "fused", q))
    agree(routes["gp_nn"].ann_interp_to_field(N).spctrm("momentum", **kw), ref_of(routes["nn_momentum"]), (name, "nn", "momentum"))
    tabs = routes["box"].helmholtz_spctrm("velocity", **kw)
    r_tot, r_comp = ref_of(routes["helm_tot"]), ref_of(routes["helm_comp"])
    agree(tabs[0], r_tot, (name, "helmholtz", "total"))
    agree(tabs[1], r_comp, (name, "helmholtz", "compressive"), floor=r_tot[:, 2])
    r_sol = r_tot.copy()
    r_sol[:, 2] = r_tot[:, 2] - r_comp[:, 2]
    agree(tabs[2], r_sol, (name, "helmholtz", "solenoidal"), floor=r_tot[:, 2])
    _free(K)


# --------------------------------------------------------------------------------------- f. limits, refused cleanly ----
def _script_range_with_bins(N, L, nbins):
    """A script-flavour k range of exactly `nbins` bins (n_bins = int((kmax - kmin) / kres) + 1) from kf to Nyquist."""
    kf = 2 * np.pi / L
    kmin, kmax = kf, (N // 2) * kf
    kres = (kmax - kmin) / (nbins - 0.5)
    assert int((kmax - kmin) / kres) + 1 == nbins
    return kmin, kmax, kres


def _bounded_rank1_factors(N, seed):
    """One separable term whose three 1-D spectra have EVERY magnitude in [0.5, 1.5] (conjugate pairs built as pairs): the
    |F|^2 of all modes lie within a factor 9^3 < 2^10 of each other."""
    rng = np.random.default_rng(seed)
    h = N // 2
    out = []
    for _ in range(3):
        spec = np.zeros(N, dtype=np.complex128)
        spec[1:h] = rng.uniform(0.5, 1.5, h - 1) * np.exp(2j * np.pi * rng.random(h - 1))
        spec[h + 1:] = np.conj(spec[1:h][::-1])
        spec[0], spec[h] = rng.uniform(0.5, 1.5, 2) * rng.choice([-1.0, 1.0], 2)
        out.append(np.fft.ifft(spec).real.copy()[None, :])
    return tuple(out)


def test_more_than_8192_bins_are_refused_and_leave_the_tables_alone(K):
    """8193 bins: prepare() raises VpsError naming the limit and nothing is enqueued; a pipeline prepared before still gives
    its earlier table afterwards, bit for bit -- through the x pass alone, which reads the tables set last, and through the
    pipeline.  Bit for bit is a fair demand of this field: every addend of a shell sum is a float32 (24 bits), the addends lie
    within 2^11 of each other (_bounded_rank1_factors, the Hermitian weight 2) and a shell of N = 64 has fewer than 2^14 modes,
    so the float64 sums are exact (49 < 53 bits) in whatever order the atomics add them."""
    from vpower import device, _ffi
    N, L = 64, 1.0
    f = _bounded_rank1_factors(N, seed=64)
    field = chk.separable_slab(K.device, f, 0, N)
    pipe = device.PowerPipeline(N, L, kernels=K, comm=device.SlabComm(enabled=False), flavour="script")
    before = pipe.finish(*pipe.accumulate([field]))
    ref_ps, ref_ns = chk.separable_shell_sums(K.device, [f], N, L, pipe.k2, pipe.thr)
    assert ref_ns.max() < 1 << 14
    _check_table(before, ref_ps, ref_ns, "before")
    kmin, kmax, kres = _script_range_with_bins(N, L, 8193)
    bad = device.PowerPipeline(N, L, kernels=K, comm=device.SlabComm(enabled=False), flavour="script", kmin=kmin, kmax=kmax, kres=kres)
    assert bad.nbins == 8193
    K.timing(True)
    try:
        with pytest.raises(_ffi.VpsError, match="8192"):
            bad.prepare()
        K.sync()
        assert all(n == 0 for n, _ in K.timing_get().values())
    finally:
        K.timing(False)
    spec, nyq = K.fft_zy(field, N, N)
    psum, ns = pipe.new_accumulators()
    K.fft_x_bin_multi([spec], N, N // 2 * N, 0, 0, 1, N // 2 * N * N, psum, ns)      # no set_binning since the refusal
    K.fft_x_bin_multi([nyq], N, N, 0, N // 2, 1, N * N, psum, ns)
    assert np.array_equal(pipe.finish(psum, ns), before, equal_nan=True)
    assert np.array_equal(pipe.finish(*pipe.accumulate([field])), before, equal_nan=True)
    _free(K)


def test_x_pass_beyond_the_lds_is_refused_and_leaves_the_accumulators_alone(K):
    """8192 bins under no_int_binning: the float64 threshold table, the shell sums and the counts alone need
    (8192 + 2) * 8 + 8192 * 8 + 8192 * 4 B of LDS (launch_x in fft_xpass.h) before any line buffer -- more than the device has.
    The x pass raises "needs ... LDS", the accumulators keep their contents, and a default-range spectrum on the same context
    afterwards is correct."""
    from vpower import device, _ffi
    N, L, nbins = 64, 1.0, 8192
    assert (nbins + 2) * 8 + nbins * 8 + nbins * 4 > K.device_info()["lds_per_cu"]
    comps = _factors(N, 3, 4)
    fields = [chk.separable_slab(K.device, f, 0, N) for f in comps]
    kmin, kmax, kres = _script_range_with_bins(N, L, nbins)
    pipe = device.PowerPipeline(N, L, kernels=K, comm=device.SlabComm(enabled=False), flavour="script", kmin=kmin, kmax=kmax, kres=kres)
    assert pipe.nbins == nbins
    psum, ns = pipe.new_accumulators()
    psum.fill_(3.0)
    ns.fill_(7)
    try:
        _ffi.set_option("no_int_binning", 1)
        with pytest.raises(_ffi.VpsError, match="needs .* LDS"):
            pipe.accumulate(fields, psum, ns)
        K.sync()
    finally:
        _ffi.set_option("no_int_binning", None)
    assert bool((psum == 3.0).all()) and bool((ns == 7).all())
    pipe = device.PowerPipeline(N, L, kernels=K, comm=device.SlabComm(enabled=False))
    ref_ps, ref_ns = chk.separable_shell_sums(K.device, comps, N, L, pipe.k2, pipe.thr)
    tab = pipe.finish(*pipe.accumulate(fields))
    _check_table(tab, ref_ps, ref_ns, "after the refusal")
    _free(K)
