"""The stream contract of include/vps_hip.h ("Streams"): every entry point behind a busy side stream (tests/stream_probe.py).
Run on an MI355X:  python -m pytest tests/test_gpu_streams.py -q -m gpu        (leg a runs without a GPU)

Every other GPU test, bench.py and smoke() stay on the null stream, which orders everything for free.  Here each call is made
inside `with torch.cuda.stream(S)` on a non-blocking pool stream, behind a blocker, on input buffers that held a decoy until S
overwrote them (stream_probe.run_case): a launch, memset or copy on the wrong stream, a wrapper that forgets self._stream(), a
table overwritten under a pending launch or a host array read after the call returned gives valid but wrong numbers.

Blocker: torch.cuda._sleep, calibrated once per module with events to stream_probe.BLOCKER_MS = 200 ms.  It must outlast the host
side of the longest non-blocking leg.  Measured on an MI355X (ROCm 7.2.0, torch 2.10 built for HIP 7.0): 199.7 ms for 4.8e8 units; the longest non-blocking call
behind it (fft_zy at 1024 with its torch allocations in one run, the Helmholtz chunk pipeline of three 128^3 fields in another)
returns after 0.45 to 2.1 ms of host time, the blocking ones after 199 to 202 ms.  Step 3 of the probe fails a leg with "blocker too short" should that ever stop holding.

Legs
  a  test_tables_cover_every_symbol (no GPU): stream_probe's three tables against vpower/_ffi.py and against the legs here.
  b  test_leg[...]: one case per device-work method of HipKernels.  Launch sites chosen by the host and the leg that reaches them:
       two-level sort, LDS-staged ........ deposit_c1 / c3 / c4, deposit_field, fused_* (deposit_plan: two_level = 1, staged = 1)
       sort_atomic = 1 ................... deposit_c4-sort_atomic (two_level = 0)
       sort_staged = 0 ................... deposit_c4-unstaged (staged = 0)
       bricks ............................ deposit_*, deposit_field;   pencils: fused_*, deposit_fft_z[_slab] (plan bx = 1, bz = N)
       pencil kernel, one-launch form .... fused_whole, fused_thin_slab, fused_components, fused_share_energy
       narrow y pass (fft_transpose_pass)  every leg below 1024;   wide y pass (fft_transpose_pass_wide): fft_zy_wide_1024
                                           (chosen by the line length alone, fft_transpose.h: wide_transpose; no plan query reports it)
       d_xpart regrowth .................. switch_xpart (its first x pass grows the partial sums of a fresh context)
       ypack rebuild ..................... fft_y_chunk_packed-rebuild (another chunk count than the warm-up's: blocking)
       NN column / scatter search ........ nn_*-column / nn_*-scatter (nn_last_search)
     NOT covered: the split pencil kernel of 4096-cell lines (energy; reachable only at N = 4096) and the one-level sort of more
     buckets than the two-level sort covers (2048^3 bricks) -- production shapes that would take a leg far beyond a few seconds.
  c  test_tables_change_under_a_pending_launch: set_binning A -> x pass -> set_binning B -> x pass; set_window CIC -> TSC -> None.
  d  test_host_arguments_are_free_on_return: k2 / thr, the window, the NN axes, hist edges, pair_k axes overwritten with the
     decoy's values right after the call returned (the z-image pointer list of spectrum_zimages: in leg h's child).
  e  test_switching_streams_*: the sort workspace (share_energy, reuse token) and d_xpart across two streams (vps_set_stream's event).
  f  test_public_surface: GasParticles / BoxField / deposit_to_grid on a side stream against the oracle and the null stream.
  g  test_timing_on_a_side_stream: launch counts per kind equal the null stream's, intervals finite and >= 0.
  h  test_library_exchange_on_a_side_stream: vps_spectrum_zimages (own communication stream, events) with ctx->stream = S, in a child.
"""
import os
import sys

import numpy as np
import pytest

import stream_probe as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
N0, NP0 = 64, 100003          # particle legs: 64^3, 1e5 particles (no multiple of a block)
TRUE, DECOY = 101, 202        # seeds
CACHE = {}


# ------------------------------------------------------------------------------------------- a: the tables ----
SPECIAL_LEGS = {"switch_sort_workspace": "test_switching_streams_sort_workspace", "switch_xpart": "test_switching_streams_xpart",
                "tables_binning": "test_tables_change_under_a_pending_launch", "tables_window": "test_tables_change_under_a_pending_launch",
                "timing": "test_timing_on_a_side_stream", "library_exchange": "test_library_exchange_on_a_side_stream",
                "destroy_with_work_pending": "test_destroy_with_work_pending", "memory_helpers": "test_memory_helpers",
                "host_arguments": "test_host_arguments_are_free_on_return", "public_surface": "test_public_surface"}


# the special legs that assert `not E_blk.query()` right behind the pure enqueues they stand for
ASSERTS_BLOCKER_PENDING = ("switch_sort_workspace", "memory_helpers", "library_exchange")


def test_tables_cover_every_symbol():
    """Every vps_* symbol of _ffi.SYMBOLS is in exactly one table, and every symbol of NONBLOCKING / BLOCKING names a leg that exists."""
    from vpower import _ffi
    names = [s[0] for s in _ffi.SYMBOLS]
    assert len(set(names)) == len(names)
    tables = {"NONBLOCKING": set(sp.NONBLOCKING), "BLOCKING": set(sp.BLOCKING), "HOST_ONLY": set(sp.HOST_ONLY)}
    assert len(sp.HOST_ONLY) == len(tables["HOST_ONLY"])
    for n in names:
        where = [t for t, members in tables.items() if n in members]
        assert len(where) == 1, "%s is in %r: every symbol belongs to exactly one table" % (n, where)
    listed = set().union(*tables.values())
    assert listed == set(names), "listed but not in _ffi.SYMBOLS: %r" % sorted(listed - set(names))
    legs = set(LEGS) | set(SPECIAL_LEGS)
    for name, fn in SPECIAL_LEGS.items():
        assert callable(globals().get(fn)), (name, fn)
    for sym, leg in list(sp.NONBLOCKING.items()) + [(s, v[0]) for s, v in sp.BLOCKING.items()]:
        assert leg in legs, "%s names the leg %r, which does not exist" % (sym, leg)
    for sym in sp.NONBLOCKING:          # a symbol listed as a pure enqueue is run by a case that asserts it
        if sp.NONBLOCKING[sym] in LEGS:
            assert not LEGS[sp.NONBLOCKING[sym]][1], (sym, "its leg is marked blocking")
        else:
            assert sp.NONBLOCKING[sym] in ASSERTS_BLOCKER_PENDING, (sym, "its leg does not assert that the blocker is still pending")
    for sym, (leg, _) in sp.BLOCKING.items():
        if leg in LEGS:
            assert LEGS[leg][1], (sym, "its leg is not marked blocking")


# ------------------------------------------------------------------------------------------- fixtures ----
@pytest.fixture(scope="module")
def K():
    import torch
    from vpower import device
    k = device.HipKernels()           # a context of its own: its stream, tables and partial sums are this module's
    yield k
    k.close()
    CACHE.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def blocker(K):
    b = sp.Blocker(K.device)
    print("blocker: %d units, %.1f ms measured" % (b.units, b.measured_ms))
    assert 0.5 * sp.BLOCKER_MS <= b.measured_ms <= 500.0, b.measured_ms
    yield b
    if b.enqueue_ms:
        worst = max(b.enqueue_ms, key=lambda e: e[1])
        print("longest non-blocking enqueue: %s, %.2f ms of host time against a blocker of %.0f ms" % (worst[0], worst[1], b.measured_ms))


def _tg():
    import route_refs
    return route_refs


def _parts(K, seed, N=N0, n=NP0):
    import torch
    key = ("parts", N, n, seed)
    if key not in CACHE:
        CACHE[key] = _tg().P(K, n, N, torch.float32, "uniform", seed)
    return CACHE[key]


def _cached(key, make):
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def _particle_case(K, name, call_on, ref_of, kinds, N=N0, n=NP0, **kw):
    """A case on (pos, vel, rho): call_on(pos, vel, rho) -> outputs, ref_of(P) -> references (cached per seed)."""
    T, D = _parts(K, TRUE, N, n), _parts(K, DECOY, N, n)
    bufs = [D.pos.clone(), D.vel.clone(), D.rho.clone()]
    refs = [_cached(("ref", name, s), lambda p=p: ref_of(p)) for s, p in ((TRUE, T), (DECOY, D))]
    return sp.Case(name, bufs, [T.pos, T.vel, T.rho], lambda: call_on(*bufs), refs[0], refs[1], kinds, **kw)


# ------------------------------------------------------------------------------------------- b: the cases ----
def leg_cell_index(K):
    return _particle_case(K, "cell_index", lambda p, v, r: [K.cell_index(p, N0, 1.0)], lambda P: [P.cells], ["exact"])


def leg_density_velocity_vector(K):
    import torch
    return _particle_case(K, "density_velocity_vector", lambda p, v, r: [K.density_velocity_vector(v, r)],
                          lambda P: [torch.cat([P.rho[:, None] * P.vel, P.rho[:, None]], dim=1)], ["exact"])


def leg_totals(K):
    def ref(P):
        m, v = P.rho.double(), P.vel.double()
        return [np.array([float(m.sum())] + [float((m * v[:, c]).sum()) for c in range(3)] + [float((m * (v * v).sum(dim=1)).sum())])]
    return _particle_case(K, "totals", lambda p, v, r: [K.particle_totals(v, r)], ref, ["exact"], blocking=True)


def leg_preprocess(K):
    def ref(P):
        pos, vel, m = P.pos.cpu().numpy(), P.vel.cpu().numpy(), P.rho.cpu().numpy().astype(np.float64)
        mn = pos.min(axis=0)
        bulk = np.array([float((m * vel[:, a]).sum() / m.sum()) for a in range(3)])      # integer data: the sums are exact
        return [mn.astype(np.float64), bulk, pos - mn, vel - bulk.astype(np.float32)]

    def call(p, v, r):
        mn, bv = K.preprocess(p, v, r)
        return [mn, bv, p, v]
    T = _parts(K, TRUE)
    bulk = ref(T)[1]
    ulp = np.abs(np.spacing(bulk.astype(np.float32))).astype(np.float64)           # tests/test_gpu_small_kernels.py: one float32 ulp
    return _particle_case(K, "preprocess", call, ref, ["exact", ("abs", ulp), "exact", ("abs", 2.0 ** -22)], blocking=True)


def _deposit_case(K, C, opts=None, expect=None, tag=""):
    from oracle import gpu_checks as chk
    import torch
    name = "deposit_c%d%s" % (C, tag)
    T, D = _parts(K, TRUE), _parts(K, DECOY)
    with sp.options(opts or {}):
        plan = K.deposit_plan(NP0, C, N0, 0, N0)
    want = dict(two_level=1, staged=1) if expect is None else expect
    assert {k: plan[k] for k in want} == want, plan
    bufs = [D.pos.clone(), D.payload(C).float().contiguous()]

    def ref(P):
        return [torch.stack([w.float() for w in chk.exact_slab_reference(P.cells, None, None, N0, 0, N0, payload=P.payload(C))]).view(C, N0, N0, N0)]

    def call():
        with sp.options(opts or {}):
            return [K.deposit(bufs[0], bufs[1], N0, 1.0, 0, N0)]
    refs = [_cached(("ref", "deposit", C, s), lambda p=p: ref(p)) for s, p in ((TRUE, T), (DECOY, D))]
    return sp.Case(name, bufs, [T.pos, T.payload(C).float().contiguous()], call, refs[0], refs[1], ["exact"])


def _field_ref(P, N, x0, nx, name):
    tg = _tg()
    return tg.reference_fields(tg.vec_grid(P, N, x0, nx), 1.0 / N, name)


def leg_deposit_field(K):
    from vpower import device as D
    plan = K.deposit_plan(NP0, 4, N0, 0, N0)
    assert plan["two_level"] == 1 and plan["bx"] > 1, plan          # bricks, not the pencils (bx = 1) of the fused route
    return _particle_case(K, "deposit_field", lambda p, v, r: list(K.deposit_field(p, v, r, N0, 1.0, 0, N0, D.MOMENTUM)),
                          lambda P: _field_ref(P, N0, 0, N0, "momentum"), ["field"] * 3)


def _image_refs(K, P, N, x0, nx, name):
    """[spec_0.., nyq_0..] complex128 references of the fused route's images."""
    tg = _tg()
    r = tg.fused_refs(K, P, N, x0, nx, [name])[name]
    return [a for a, _ in r] + [b for _, b in r]


def _fused_case(K, name, x0, nx, component=None):
    from vpower import device as D
    plan = K.deposit_plan(NP0, 4, N0, x0, nx, pencil=True)
    assert plan["bx"] == 1 and plan["bz"] == N0 and plan["two_level"] == 1, plan
    comps = (0, 1, 2) if component is None else component

    def ref(P):
        r = _cached(("img", x0, nx, id(P)), lambda: _image_refs(K, P, N0, x0, nx, "momentum"))
        return [r[c] for c in comps] + [r[3 + c] for c in comps]

    def call(p, v, r):
        spec, nyq = K.deposit_fft_zy(p, v, r, N0, 1.0, x0, nx, D.MOMENTUM, component=component)
        return list(spec) + list(nyq)
    return _particle_case(K, name, call, ref, ["image"] * (2 * len(comps)))


def leg_fused_share_energy(K):
    """momentum with share_energy, then energy with the reuse token: the energy call only runs its y pass on what the first left."""
    from vpower import device as D
    tg = _tg()

    def ref(P):
        return _cached(("img", 0, N0, id(P)), lambda: _image_refs(K, P, N0, 0, N0, "momentum")) + \
            _cached(("imgE", id(P)), lambda: _image_refs(K, P, N0, 0, N0, "energy"))

    def call(p, v, r):
        with tg.reuse_flags(K) as taken:
            s1, n1 = K.deposit_fft_zy(p, v, r, N0, 1.0, 0, N0, D.MOMENTUM, share_energy=True)
            s2, n2 = K.deposit_fft_zy(p, v, r, N0, 1.0, 0, N0, D.ENERGY, reuse_sort=K.fused_token(), share_energy=True)
        assert taken == [0, D.FLAG_REUSE_SORT], taken
        return list(s1) + list(n1) + list(s2) + list(n2)
    return _particle_case(K, "fused_share_energy", call, ref, ["image"] * 8)


def _zimage_refs(K, P, N, x0, nx, name):
    import torch
    tg = _tg()
    return [tg.z_reference(torch.as_tensor(np.ascontiguousarray(f), device=K.device), N) for f in _field_ref(P, N, x0, nx, name)]


def leg_deposit_fft_z(K):
    from vpower import device as D
    return _particle_case(K, "deposit_fft_z", lambda p, v, r: list(K.deposit_fft_z(p, v, r, N0, 1.0, 0, N0, D.MOMENTUM)),
                          lambda P: _zimage_refs(K, P, N0, 0, N0, "momentum"), ["image"] * 3)


def leg_deposit_fft_z_slab(K):
    """count_in_slab + the slab-sized workspace (rows [48, 64))."""
    from vpower import device as D
    x0, nx = 48, 16

    def ref(P):
        inside = int(((P.cells[:, 0] >= x0) & (P.cells[:, 0] < x0 + nx)).sum())
        return [np.array([inside])] + _zimage_refs(K, P, N0, x0, nx, "momentum")

    def call(p, v, r):
        inside = K.count_in_slab(p, N0, 1.0, x0, nx)
        z = K.deposit_fft_z(p, v, r, N0, 1.0, x0, nx, D.MOMENTUM, slab_particles=inside)
        return [np.array([inside])] + list(z)
    return _particle_case(K, "deposit_fft_z_slab", call, ref, ["exact"] + ["image"] * 3, blocking=True, indep=(0,))


def _assign_data(K, seed):
    """20 000 real-valued particles in a 32^3 box of length 2 (the shape of test_gpu_assign_direct's public-surface leg)."""
    def make():
        rng = np.random.default_rng(seed)
        pos = (rng.random((20000, 3)) * 2.0).astype(np.float32)
        f = rng.standard_normal((20000, 4)).astype(np.float32)
        return pos, f, K.to_device(pos), K.to_device(f)
    return _cached(("assign", seed), make)


def _assign_case(K, route, assignment):
    from oracle import vps_oracle as orc
    N, L = 32, 2.0
    T, D = _assign_data(K, TRUE), _assign_data(K, DECOY)
    bufs = [D[2].clone(), D[3].clone()]

    def ref(d):
        return [np.moveaxis(orc.deposit_assign(d[1].astype(np.float64), d[0], N, L, assignment), -1, 0)]

    def call():
        if route == "expand":
            pe, fe = K.assign_expand(bufs[0], bufs[1], N, L, assignment)
            return [K.deposit(pe, fe, N, L, 0, N)]
        return [K.deposit_assign(bufs[0], bufs[1], N, L, assignment)]
    refs = [_cached(("ref", "assign", assignment, s), lambda d=d: ref(d)) for s, d in ((TRUE, T), (DECOY, D))]
    bar = ("abs", 2e-5 * float(np.abs(refs[0][0]).max()))          # tests/test_gpu_assign_direct.py: test_public_surface
    name = ("assign_expand_%s" if route == "expand" else "deposit_assign_%s") % assignment
    return sp.Case(name, bufs, [T[2], T[3]], call, refs[0], refs[1], [bar], bitwise=False)


def _nn_data(K, seed):
    """(pos, integer payload [rho v, rho], axes, exact neighbour index): 2e4 particles, 32^3 uniform lattice."""
    tg = _tg()
    return tg.nn_setup(K, 20000, ("uniform", 32), 0, 32, seed)


def _nn_case(K, method, column):
    import torch
    from vpower import device as D
    tg = _tg()
    M = 32
    T, Dd = _nn_data(K, TRUE), _nn_data(K, DECOY)
    bufs = [Dd[0].clone(), Dd[1].clone()]
    axes = T[2]
    opts = {"nn_column": column}
    kind = "column" if column else "scatter"

    def ref(d):
        pos, pay, _, idx = d
        near = pay[idx]
        if method == "nn_resample":
            return [idx.to(torch.int32).reshape(M, M, M), near.t().contiguous().reshape(4, M, M, M)]
        vec = near.double().cpu().numpy().reshape(M, M, M, 4)
        fields = tg.reference_fields(vec, 1.0 / M, "vm" if method == "nn_resample_field" else "momentum")
        return [idx.to(torch.int32).reshape(M, M, M)] + fields

    def call():
        with sp.options(opts):
            if method == "nn_resample":
                out, idx = K.nn_resample(bufs[0], bufs[1], axes, 0, M, want_index=True)
            elif method == "nn_resample_field":
                out, idx = K.nn_resample_field(bufs[0], bufs[1], axes, 0, M, 1.0 / M, want_index=True)
            else:
                out, idx = K.nn_resample_quantity(bufs[0], bufs[1], axes, 0, M, 1.0 / M, D.MOMENTUM, want_index=True)
        assert K.nn_last_search()["kind"] == kind, K.nn_last_search()
        return [idx, out] if method == "nn_resample" else [idx] + list(out)
    refs = [_cached(("ref", method, s), lambda d=d: ref(d)) for s, d in ((TRUE, T), (DECOY, Dd))]
    kinds = ["exact", "exact"] if method == "nn_resample" else ["exact"] + ["field"] * (len(refs[0]) - 1)
    return sp.Case("%s-%s" % (method, kind), bufs, [T[0], T[1]], call, refs[0], refs[1], kinds, blocking=True)


def _chans(K, seed):
    """[rho v, rho] cell totals of the particles as a float32 grid [4, N, N, N] and its float64 form [N, N, N, 4]."""
    def make():
        import torch
        vec = _tg().vec_grid(_parts(K, seed), N0, 0, N0)
        return vec, torch.as_tensor(np.ascontiguousarray(np.moveaxis(vec, -1, 0)), dtype=torch.float32, device=K.device).contiguous()
    return _cached(("chans", seed), make)


def _algebra_case(K, out_of_place):
    from vpower import device as D
    tg = _tg()
    T, Dd = _chans(K, TRUE), _chans(K, DECOY)
    bufs = [Dd[1].clone()]

    def call():
        if out_of_place:
            return list(K.field_algebra_out(bufs[0], D.MOMENTUM, 0, 1.0 / N0))
        K.field_algebra(bufs[0], D.MOMENTUM, 0, 1.0 / N0)
        return list(bufs[0][:3])
    refs = [_cached(("ref", "algebra", s), lambda d=d: tg.reference_fields(d[0], 1.0 / N0, "momentum")) for s, d in ((TRUE, T), (DECOY, Dd))]
    return sp.Case("field_algebra_out" if out_of_place else "field_algebra", bufs, [T[1]], call, refs[0], refs[1], ["field"] * 3)


def _sep(K, N, seed, x0=0, nx=None):
    from oracle import gpu_checks as chk
    nx = N if nx is None else nx
    return _cached(("sep", N, seed, x0, nx), lambda: chk.separable_slab(K.device, chk.separable_factors(N, seed=seed), x0, nx))


def _fft_case(K, name, N, nx, x0, call_on, ref_on, kinds, weighted=False, **kw):
    """A case on one separable field (and a weight): call_on(f, w) -> outputs; ref_on(f64 product) -> references."""
    T, Dd = _sep(K, N, TRUE, x0, nx), _sep(K, N, DECOY, x0, nx)
    w = _sep(K, N, 7, x0, nx) if weighted else None
    bufs = [Dd.clone()]

    def ref(f):
        return ref_on(f.double() * w.double() if weighted else f.double())
    refs = [_cached(("ref", name, s), lambda f=f: ref(f)) for s, f in ((TRUE, T), (DECOY, Dd))]
    return sp.Case(name, bufs, [T], lambda: call_on(bufs[0], w), refs[0], refs[1], kinds, **kw)


def leg_fft_zy(K, N=N0, nx=N0, x0=0, weighted=False, name=None):
    tg = _tg()
    name = name or ("fft_zy_weighted" if weighted else "fft_zy")
    return _fft_case(K, name, N, nx, x0, lambda f, w: list(K.fft_zy(f, N, nx, weight=w)), lambda p: list(tg.zy_reference(p, N, nx)),
                     ["image", "image"], weighted=weighted)


def leg_fft_z(K):
    tg = _tg()
    return _fft_case(K, "fft_z", N0, N0, 0, lambda f, w: [K.fft_z(f, N0, N0, weight=w)], lambda p: [tg.z_reference(p, N0)], ["image"],
                     weighted=True)


def leg_rfft3(K):
    import torch
    return _fft_case(K, "rfft3", N0, N0, 0, lambda f, w: [K.rfft3(f, N0)], lambda p: [torch.fft.rfftn(p).permute(2, 1, 0).contiguous()], ["image"])


def leg_power_grid(K):
    import torch
    return _fft_case(K, "power_grid", N0, N0, 0, lambda f, w: [K.power_grid([f], N0)],
                     lambda p: [torch.fft.rfftn(p).permute(2, 1, 0).abs().square().contiguous()], ["field"])


def leg_fft_x_write(K):
    """z and y passes, then the write-mode x pass: the half spectrum below the Nyquist plane."""
    import torch
    N = N0

    def call(f, w):
        spec, nyq = K.fft_zy(f, N, N)
        out = K.empty((N // 2, N, N), torch.complex64)
        K.fft_x_write(spec, N, N // 2 * N, 1, 0, out)
        return [out]
    return _fft_case(K, "fft_x_write", N, N, 0, call, lambda p: [torch.fft.rfftn(p).permute(2, 1, 0)[: N // 2].contiguous()], ["image"])


def _pipe(K, N, **kw):
    from vpower import device as D
    return D.PowerPipeline(N, 1.0, kernels=K, comm=D.SlabComm(enabled=False), **kw)


def _shell_case(K, name, N, ncomp, run, helmholtz=False, window=None, **kw):
    """A binning case on `ncomp` separable component fields: run(pipe, fields) -> accumulators; the references are
    oracle/gpu_checks.separable_shell_sums (tests/helmholtz_ref.py for the compressive part)."""
    from oracle import gpu_checks as chk
    import helmholtz_ref as hr
    pipe = _pipe(K, N, deconvolve=window)
    seeds = {TRUE: [TRUE + c for c in range(ncomp)], DECOY: [DECOY + c for c in range(ncomp)]}
    T = [_sep(K, N, s) for s in seeds[TRUE]]
    Dd = [_sep(K, N, s) for s in seeds[DECOY]]
    bufs = [f.clone() for f in Dd]

    def ref(ss):
        comps = [chk.separable_factors(N, seed=s) for s in ss]
        if helmholtz:
            r = hr.separable_helmholtz_sums(K.device, comps, N, 1.0, pipe.k2, pipe.thr, win=pipe.window)
            return [np.asarray(r[0]), np.asarray(r[2]), np.asarray(r[1])]
        ps, ns = chk.separable_shell_sums(K.device, comps, N, 1.0, pipe.k2, pipe.thr, win=pipe.window)
        return [ps, ns]

    def call():
        acc = run(pipe, bufs)
        scale = 0.5 * pipe.const ** 2
        return [acc[0] * scale, acc[1]] + ([acc[2] * scale] if helmholtz else [])
    refs = [_cached(("ref", "shell", N, tuple(ss), helmholtz, window), lambda ss=ss: ref(ss)) for ss in (seeds[TRUE], seeds[DECOY])]
    kinds = ["psum", "exact"] + (["psum"] if helmholtz else [])
    return sp.Case(name, bufs, T, call, refs[0], refs[1], kinds, indep=(1,), bitwise=False, **kw)


def _zy_all(K, pipe, fields):
    import torch
    zy = [K.fft_zy(f, pipe.N, pipe.N) for f in fields]
    return torch.stack([z[0] for z in zy]), torch.stack([z[1] for z in zy])


def leg_fft_x_bin(K):
    """One component through vps_fft_x (mode 0)."""
    def run(pipe, fields):
        pipe.prepare()
        psum, ns = pipe.new_accumulators()
        spec, nyq = K.fft_zy(fields[0], pipe.N, pipe.N)
        K.fft_x_bin(spec, pipe.N, pipe.N // 2 * pipe.N, 0, 0, 1, 0, psum, ns)
        K.fft_x_bin(nyq, pipe.N, pipe.N, 0, pipe.N // 2, 1, 0, psum, ns)
        return psum, ns
    return _shell_case(K, "fft_x_bin", N0, 1, run)


def leg_fft_x_bin_multi(K):
    return _shell_case(K, "fft_x_bin_multi", N0, 3, lambda pipe, fields: pipe.accumulate_spectra(*_zy_all(K, pipe, fields)))


def leg_fft_x_bin_helmholtz(K):
    return _shell_case(K, "fft_x_bin_helmholtz", N0, 3, lambda pipe, fields: pipe.accumulate_spectra_helmholtz(*_zy_all(K, pipe, fields)),
                       helmholtz=True)


def _chunk_run(K, helmholtz, nchunks=2):
    def run(pipe, fields):
        pipe.chunked, pipe.nchunks = True, nchunks             # one rank, the chunk pipeline of the slab exchange
        z = [K.fft_z(f, pipe.N, pipe.N) for f in fields]
        pipe.prepare()
        with K.binning_only():
            assert K.y_packed(pipe.N), "128: the chunks carry packed rows"
        return pipe.accumulate_zimages_helmholtz(z) if helmholtz else pipe.accumulate_zimages(z)
    return run


def leg_fft_x_bin_chunk(K):
    """128: packed rows (kcut) in fft_y_chunk, the chunk x pass."""
    return _shell_case(K, "fft_x_bin_chunk", 128, 3, _chunk_run(K, False))


def leg_fft_x_bin_chunk_helmholtz(K):
    return _shell_case(K, "fft_x_bin_chunk_helmholtz", 128, 3, _chunk_run(K, True), helmholtz=True)


def _y_chunk_case(K, packed, rebuild=False):
    """fft_y_chunk of chunk 1 of 2 (the last: Nyquist rows ride behind it), one rank, 128: every stored element against numpy's
    transform (tests/route_refs.py: expected_chunk); the elements a packed slot does not store are left out."""
    import contextlib
    import torch
    from oracle import gpu_checks as chk
    tg = _tg()
    N, C, c = 128, 2, 1
    pipe = _pipe(K, N, **dict(zip(("flavour", "kmin", "kmax", "kres"), chk.k_range("band", N, 1.0))))          # (kmax = 0.6 N/2: the upper chunk keeps some planes)
    kcut = chk.row_cut(N, pipe.k2, pipe.thr) if packed else None
    name = "fft_y_chunk_%s%s" % ("packed" if packed else "unpacked", "-rebuild" if rebuild else "")

    def ref_on(p):
        spec, nyq = tg.zy_reference(p, N, N)
        want, stored = tg.expected_chunk(spec, nyq, N, N, 1, C, c, kcut)
        CACHE[("stored", packed)] = stored
        assert bool(stored.any()) and (not packed or not bool(stored.all())), "the chunk is meant to hold stored and unstored rows"
        return [torch.where(stored, want, torch.zeros_like(want))]

    def call_on(f, w, chunks=C, chunk=c):
        pipe.prepare()
        z = K.fft_z(f, N, N)
        with (K.binning_only() if packed else contextlib.nullcontext()):
            assert bool(K.y_packed(N)) == packed
            out = K.fft_y_chunk(z, N, N, 1, chunks, chunk)
        if chunks != C:
            return [out]
        return [torch.where(CACHE[("stored", packed)], out, torch.zeros_like(out))]
    case = _fft_case(K, name, N, N, 0, call_on, ref_on, ["image"], blocking=rebuild)
    if rebuild:                  # the warm-up leaves the chunk tables of ANOTHER chunk count: the call rebuilds them, behind a drain
        buf = case.bufs[0]
        case.warm = lambda: call_on(buf, None, chunks=4, chunk=0)
        case.reset = lambda: call_on(buf, None, chunks=4, chunk=0)
    return case


def leg_raw_fft_zy_and_power_bin(K):
    """The two entry points no wrapper method calls (vps_fft_zy, vps_power_bin), through the C ABI."""
    import torch
    from oracle import gpu_checks as chk
    tg = _tg()
    N = N0
    pipe = _pipe(K, N)
    T, Dd = _sep(K, N, TRUE), _sep(K, N, DECOY)
    bufs = [Dd.clone()]

    def ref(seed, f):
        ps, ns = chk.separable_shell_sums(K.device, [chk.separable_factors(N, seed=seed)], N, 1.0, pipe.k2, pipe.thr)
        return list(tg.zy_reference(f.double(), N, N)) + [ps, ns]

    def call():
        K._stream()
        pipe.prepare()
        spec, nyq = K.empty((N // 2, N, N), torch.complex64), K.empty((N, N), torch.complex64)
        work = K.workspace("fft", K.lib.vps_fft_workspace_bytes(N, N))
        K._chk(K.lib.vps_fft_zy(K.ctx, N, N, K._ptr(bufs[0]), K._ptr(spec), K._ptr(nyq), K._ptr(work)))
        psum, ns = pipe.new_accumulators()
        pwork = K.workspace("power", K.lib.vps_power_workspace_bytes(N))
        K._chk(K.lib.vps_power_bin(K.ctx, N, K._ptr(bufs[0]), K._ptr(pwork), K._ptr(psum), K._ptr(ns)))
        return [spec, nyq, psum * (0.5 * pipe.const ** 2), ns]
    refs = [_cached(("ref", "raw", s), lambda s=s, f=f: ref(s, f)) for s, f in ((TRUE, T), (DECOY, Dd))]
    return sp.Case("raw_fft_zy_and_power_bin", bufs, [T], call, refs[0], refs[1], ["image", "image", "psum", "exact"], indep=(3,),
                   bitwise=False)


def leg_pair_k(K):
    from oracle import vps_oracle as orc
    N = 48
    axes = {s: [orc.k_axis(2.5, N) * f for f in ((1.0, 1.5, 0.5) if s == TRUE else (2.0, 0.75, 1.25))] for s in (TRUE, DECOY)}

    def ref(ax):
        kx, ky, kz = np.meshgrid(*ax, indexing="ij")
        return [np.sqrt((kx * kx + ky * ky) + kz * kz).ravel()]
    return sp.Case("pair_k", [], [], lambda: [K.pair_k(*axes[TRUE])], ref(axes[TRUE]), ref(axes[DECOY]), ["exact"], blocking=True,
                   warm=lambda: K.pair_k(*axes[DECOY]))


def leg_hist_pairs(K):
    import small_ref as sr
    n = 100003
    edges = np.linspace(0.0, 1.0, 33)

    def make(seed):
        rng = np.random.default_rng(seed)
        k, w = rng.random(n), sr.dyadic_weights(rng, n)
        return k, w, K.to_device(k), K.to_device(w)
    T, Dd = _cached(("hist", TRUE), lambda: make(TRUE)), _cached(("hist", DECOY), lambda: make(DECOY))
    bufs = [Dd[2].clone(), Dd[3].clone()]

    def ref(d):
        return [np.histogram(d[0], bins=edges, weights=d[1])[0], np.histogram(d[0], bins=edges)[0]]
    return sp.Case("hist_pairs", bufs, [T[2], T[3]], lambda: list(K.hist_pairs(bufs[0], bufs[1], edges)), ref(T), ref(Dd),
                   [("rel", 1e-12), "exact"], blocking=True)


# name -> (builder, blocking)
LEGS = {
    "preprocess": (leg_preprocess, True),
    "totals": (leg_totals, True),
    "cell_index": (leg_cell_index, False),
    "density_velocity_vector": (leg_density_velocity_vector, False),
    "deposit_c1": (lambda K: _deposit_case(K, 1), False),
    "deposit_c3": (lambda K: _deposit_case(K, 3), False),
    "deposit_c4": (lambda K: _deposit_case(K, 4), False),
    "deposit_c4-sort_atomic": (lambda K: _deposit_case(K, 4, {"sort_atomic": 1}, dict(two_level=0), "-sort_atomic"), False),
    "deposit_c4-unstaged": (lambda K: _deposit_case(K, 4, {"sort_staged": 0}, dict(two_level=1, staged=0), "-unstaged"), False),
    "deposit_field": (leg_deposit_field, False),
    "fused_whole": (lambda K: _fused_case(K, "fused_whole", 0, N0), False),
    "fused_thin_slab": (lambda K: _fused_case(K, "fused_thin_slab", 48, 16), False),
    "fused_components": (lambda K: _fused_case(K, "fused_components", 0, N0, component=(0, 2)), False),
    "fused_share_energy": (leg_fused_share_energy, False),
    "deposit_fft_z": (leg_deposit_fft_z, False),
    "deposit_fft_z_slab": (leg_deposit_fft_z_slab, True),
    "assign_expand_cic": (lambda K: _assign_case(K, "expand", "cic"), False),
    "assign_expand_tsc": (lambda K: _assign_case(K, "expand", "tsc"), False),
    "deposit_assign_cic": (lambda K: _assign_case(K, "direct", "cic"), False),
    "deposit_assign_tsc": (lambda K: _assign_case(K, "direct", "tsc"), False),
    "nn_resample-column": (lambda K: _nn_case(K, "nn_resample", 1), True),
    "nn_resample-scatter": (lambda K: _nn_case(K, "nn_resample", 0), True),
    "nn_resample_field-column": (lambda K: _nn_case(K, "nn_resample_field", 1), True),
    "nn_resample_field-scatter": (lambda K: _nn_case(K, "nn_resample_field", 0), True),
    "nn_resample_quantity-column": (lambda K: _nn_case(K, "nn_resample_quantity", 1), True),
    "nn_resample_quantity-scatter": (lambda K: _nn_case(K, "nn_resample_quantity", 0), True),
    "field_algebra": (lambda K: _algebra_case(K, False), False),
    "field_algebra_out": (lambda K: _algebra_case(K, True), False),
    "fft_zy": (leg_fft_zy, False),
    "fft_zy_weighted": (lambda K: leg_fft_zy(K, weighted=True), False),
    "fft_zy_wide_1024": (lambda K: leg_fft_zy(K, 1024, 16, 480, name="fft_zy_wide_1024"), False),
    "fft_z": (leg_fft_z, False),
    "fft_y_chunk_packed": (lambda K: _y_chunk_case(K, True), False),
    "fft_y_chunk_unpacked": (lambda K: _y_chunk_case(K, False), False),
    "fft_y_chunk_packed-rebuild": (lambda K: _y_chunk_case(K, True, rebuild=True), True),
    "fft_x_bin": (leg_fft_x_bin, False),
    "fft_x_bin_multi": (leg_fft_x_bin_multi, False),
    "fft_x_bin_chunk": (leg_fft_x_bin_chunk, False),
    "fft_x_bin_helmholtz": (leg_fft_x_bin_helmholtz, False),
    "fft_x_bin_chunk_helmholtz": (leg_fft_x_bin_chunk_helmholtz, False),
    "fft_x_write": (leg_fft_x_write, False),
    "rfft3": (leg_rfft3, False),
    "power_grid": (leg_power_grid, False),
    "raw_fft_zy_and_power_bin": (leg_raw_fft_zy_and_power_bin, False),
    "pair_k": (leg_pair_k, True),
    "hist_pairs": (leg_hist_pairs, True),
}


@gpu
@pytest.mark.parametrize("name", list(LEGS))
def test_leg(K, blocker, name):
    build, blocking = LEGS[name]
    case = build(K)
    assert case.blocking == blocking and case.name == name, (case.name, case.blocking)
    sp.run_case(case, blocker)


# ------------------------------------------------------------------------------------------- c: tables under a pending launch ----
@gpu
def test_tables_change_under_a_pending_launch(K, blocker):
    """An x pass with k range A is enqueued behind the blocker; set_binning(B) and a second x pass follow; then the window goes
    CIC -> TSC -> None with an x pass after each.  Every table matches the reference of ITS tables: no launch sees its successor's."""
    import torch
    from oracle import gpu_checks as chk
    from vpower import device as D
    N = N0
    comps = [chk.separable_factors(N, seed=TRUE)]
    f = _sep(K, N, TRUE)
    pa = _pipe(K, N)
    kb = dict(zip(("flavour", "kmin", "kmax", "kres"), chk.k_range("band", N, 1.0)))
    pb = _pipe(K, N, **kb)
    pw = {w: _pipe(K, N, deconvolve=w) for w in ("cic", "tsc")}
    pipes = [pa, pb, pw["cic"], pw["tsc"], pa]
    refs = [chk.separable_shell_sums(K.device, comps, N, 1.0, p.k2, p.thr, win=p.window) for p in pipes]
    assert sp.error_in_bars(refs[2][0], refs[0][0], "psum") >= sp.GUARD_FACTOR and sp.error_in_bars(refs[3][0], refs[2][0], "psum") >= sp.GUARD_FACTOR
    assert len(refs[1][0]) != len(refs[0][0]) or sp.error_in_bars(refs[1][0], refs[0][0], "psum") >= sp.GUARD_FACTOR
    spec, nyq = K.fft_zy(f, N, N)
    spec, nyq = spec[None].contiguous(), nyq[None].contiguous()
    for p in pipes:                                        # every table once on the null stream: nothing below is a first use
        p.accumulate_spectra(spec, nyq)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=K.device)
    with torch.cuda.stream(side):
        blocker.enqueue()
        accs = [p.accumulate_spectra(spec, nyq) for p in pipes]
        got = [(a[0].cpu().numpy() * (0.5 * p.const ** 2), a[1].cpu().numpy()) for a, p in zip(accs, pipes)]
    side.synchronize()
    for i, ((ps, ns), (rps, rns)) in enumerate(zip(got, refs)):
        assert np.array_equal(ns, rns), "tables %d: shell counts" % i
        miss = sp.error_in_bars(ps, rps, "psum")
        print("tables %d: %.3g bars" % (i, miss))
        assert miss <= 1.0, "tables %d: shell sums miss their own reference by %.3g bars" % (i, miss)
    K.set_window(N, None)


# ------------------------------------------------------------------------------------------- d: host arguments ----
@gpu
def test_host_arguments_are_free_on_return(K, blocker):
    """Every entry point that takes host arrays, behind the blocker, its arrays overwritten with the decoy's values as soon as
    it has returned: set_binning (k2, thr), set_window, the NN axes, hist_pairs edges, pair_k axes.  (The pointer list of
    spectrum_zimages needs a communicator, hence a child process: the last step of test_library_exchange_on_a_side_stream makes
    the raw call with a list of its own and repoints it at the decoy's z images right after the return.)"""
    import torch
    from oracle import gpu_checks as chk
    from oracle import vps_oracle as orc
    N = N0
    comps = [chk.separable_factors(N, seed=TRUE)]
    f = _sep(K, N, TRUE)
    pa = _pipe(K, N, deconvolve="cic")
    pb = _pipe(K, N, deconvolve="tsc", **dict(zip(("flavour", "kmin", "kmax", "kres"), chk.k_range("band", N, 1.0))))
    ref_ps, ref_ns = chk.separable_shell_sums(K.device, comps, N, 1.0, pa.k2, pa.thr, win=pa.window)
    spec, nyq = K.fft_zy(f, N, N)
    nnT, nnD = _nn_data(K, TRUE), _nn_data(K, DECOY)
    ks = orc.k_axis(2.5, 48)
    edges_true = np.linspace(0.0, 1.0, 33)
    hk = K.to_device(np.random.default_rng(5).random(50000))
    # the decoy's values, same shapes: tables of another k range cut / padded to size would not be valid, so the decoy tables are
    # the true ones scaled (monotone thresholds, an even window)
    pb.accumulate_spectra(spec[None].contiguous(), nyq[None].contiguous())
    K.nn_resample(nnD[0], nnD[1], [a * 0.9 for a in nnD[2]], 0, 32, want_index=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=K.device)
    with torch.cuda.stream(side):
        blocker.enqueue()
        k2, thr = pa.k2.copy(), pa.thr.copy()
        K.set_binning(N, k2, thr, float(pa.edges[0]), pa._binning[4])
        k2 *= 1.37
        thr *= 0.61
        win = pa.window.copy()
        K.set_window(N, win)
        win[:] = pb.window
        psum, ns = pa.new_accumulators()
        K.fft_x_bin(spec, N, N // 2 * N, 0, 0, 1, 0, psum, ns)
        K.fft_x_bin(nyq, N, N, 0, N // 2, 1, 0, psum, ns)
        axes = [a.copy() for a in nnT[2]]
        pos, pay = nnD[0].clone(), nnD[1].clone()
        pos.copy_(nnT[0])
        pay.copy_(nnT[1])
        out, idx = K.nn_resample(pos, pay, axes, 0, 32, want_index=True)
        for a in axes:
            a *= 0.9
        ax = [ks.copy(), ks * 1.5, ks * 0.5]
        pk = K.pair_k(*ax)
        for a in ax:
            a *= 2.0
        edges = edges_true.copy()
        hs, hn = K.hist_pairs(hk, None, edges)
        edges *= 0.5
        got = [x.cpu().numpy() for x in (psum, ns, idx, pk, hn)]
    side.synchronize()
    assert np.array_equal(got[1], ref_ns) and sp.error_in_bars(got[0] * (0.5 * pa.const ** 2), ref_ps, "psum") <= 1.0
    assert np.array_equal(got[2].reshape(-1), nnT[3].cpu().numpy()), "the NN axes were read after the call returned"
    kx, ky, kz = np.meshgrid(ks, ks * 1.5, ks * 0.5, indexing="ij")
    assert np.array_equal(got[3], np.sqrt((kx * kx + ky * ky) + kz * kz).ravel()), "the pair_k axes were read after the call returned"
    assert np.array_equal(got[4], np.histogram(hk.cpu().numpy(), bins=edges_true)[0])
    K.set_window(N, None)


# ------------------------------------------------------------------------------------------- e: switching streams ----
@gpu
def test_switching_streams_sort_workspace(K, blocker):
    """momentum with share_energy on S1 behind a blocker, energy with the reuse token on S2 with none: vps_set_stream makes S2 wait
    for what S1 holds.  (Without that the energy call would read the sort and the z image the decoy run left: valid, wrong.)"""
    import torch
    from vpower import device as D
    tg = _tg()
    T, Dd = _parts(K, TRUE), _parts(K, DECOY)
    ref = _cached(("imgE", id(T)), lambda: _image_refs(K, T, N0, 0, N0, "energy"))
    dref = _cached(("imgE", id(Dd)), lambda: _image_refs(K, Dd, N0, 0, N0, "energy"))
    assert sp.error_in_bars(dref[0], ref[0], "image") >= sp.GUARD_FACTOR
    pos, vel, rho = Dd.pos.clone(), Dd.vel.clone(), Dd.rho.clone()
    K.deposit_fft_zy(pos, vel, rho, N0, 1.0, 0, N0, D.MOMENTUM, share_energy=True)          # a valid earlier sort of the decoy
    K.deposit_fft_zy(pos, vel, rho, N0, 1.0, 0, N0, D.ENERGY, reuse_sort=K.fused_token(), share_energy=True)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=K.device), torch.cuda.Stream(device=K.device)
    with tg.reuse_flags(K) as taken:
        with torch.cuda.stream(s1):
            blocker.enqueue()
            behind = torch.cuda.Event()
            behind.record(s1)
            for b, t in zip((pos, vel, rho), (T.pos, T.vel, T.rho)):
                b.copy_(t, non_blocking=True)
            K.deposit_fft_zy(pos, vel, rho, N0, 1.0, 0, N0, D.MOMENTUM, share_energy=True)
            tok = K.fused_token()
        # (the token compares the tensors' version counters, which the copies above have already moved)
        with torch.cuda.stream(s2):
            spec, nyq = K.deposit_fft_zy(pos, vel, rho, N0, 1.0, 0, N0, D.ENERGY, reuse_sort=tok, share_energy=True)
            assert not behind.query(), "blocker too short: the energy call on S2 was made after S1 had already drained"
            got = [spec[0].cpu(), nyq[0].cpu()]
    assert taken == [0, D.FLAG_REUSE_SORT], taken
    torch.cuda.synchronize()
    for g, r, d in zip(got, ref, dref):
        miss = sp.error_in_bars(g, r, "image")
        assert miss <= 1.0, "energy after a stream switch misses its reference by %.3g bars (%.3g from the decoy's)" % (miss, sp.error_in_bars(g, d, "image"))


@gpu
def test_switching_streams_xpart(blocker):
    """A fresh context: its first x pass on S1 behind the blocker (tables uploaded, the partial sums d_xpart grown: the call drains
    the stream).  Then two binning x passes of other fields, the first on S1 behind the blocker, the second on S2 with none: both
    use the one d_xpart, both tables must be right.  (This pair pins the RESULT across a switch, not the need for
    vps_set_stream's event: S1 waits 200 ms and the pass on S2 takes microseconds, so without the event the two would not
    overlap either.  Only test_switching_streams_sort_workspace fails without it.)"""
    import torch
    from oracle import gpu_checks as chk
    from vpower import device as D
    k = D.HipKernels()
    try:
        N = N0
        pipe = D.PowerPipeline(N, 1.0, kernels=k, comm=D.SlabComm(enabled=False))
        fields = [_sep(k, N, s) for s in (TRUE, DECOY)]
        refs = [chk.separable_shell_sums(k.device, [chk.separable_factors(N, seed=s)], N, 1.0, pipe.k2, pipe.thr) for s in (TRUE, DECOY)]
        assert sp.error_in_bars(refs[1][0], refs[0][0], "psum") >= sp.GUARD_FACTOR
        zy = [k.fft_zy(f, N, N) for f in fields]
        zy = [(a.clone()[None], b.clone()[None]) for a, b in zy]
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(device=k.device), torch.cuda.Stream(device=k.device)
        with torch.cuda.stream(s1):            # the first x pass of this context: tables uploaded and d_xpart grown behind the blocker
            blocker.enqueue()
            a0 = pipe.accumulate_spectra(*zy[0])
            g0 = (a0[0].cpu().numpy(), a0[1].cpu().numpy())
        assert np.array_equal(g0[1], refs[0][1]) and sp.error_in_bars(g0[0] * (0.5 * pipe.const ** 2), refs[0][0], "psum") <= 1.0
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            blocker.enqueue()
            a1 = pipe.accumulate_spectra(*zy[0])
        with torch.cuda.stream(s2):
            a2 = pipe.accumulate_spectra(*zy[1])
            g2 = (a2[0].cpu().numpy(), a2[1].cpu().numpy())
        with torch.cuda.stream(s1):
            g1 = (a1[0].cpu().numpy(), a1[1].cpu().numpy())
        torch.cuda.synchronize()
        for i, (g, r) in enumerate(zip((g1, g2), refs)):
            assert np.array_equal(g[1], r[1]), i
            miss = sp.error_in_bars(g[0] * (0.5 * pipe.const ** 2), r[0], "psum")
            assert miss <= 1.0, "x pass %d of two streams sharing d_xpart misses its reference by %.3g bars" % (i, miss)
    finally:
        k.close()


@gpu
def test_destroy_with_work_pending(blocker):
    """vps_destroy drains the stream: a context closed while its launch still waits behind the blocker leaves the right output."""
    import torch
    from vpower import device as D
    k = D.HipKernels()
    T, Dd = _parts(k, TRUE), _parts(k, DECOY)
    vel, rho = Dd.vel.clone(), Dd.rho.clone()
    k.density_velocity_vector(vel, rho)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=k.device)
    with torch.cuda.stream(side):
        blocker.enqueue()
        vel.copy_(T.vel, non_blocking=True)
        rho.copy_(T.rho, non_blocking=True)
        out = k.density_velocity_vector(vel, rho)
        k.close()
        got = out.cpu()
    side.synchronize()
    assert torch.equal(got, torch.cat([T.rho[:, None] * T.vel, T.rho[:, None]], dim=1).cpu())


@gpu
def test_memory_helpers(K, blocker):
    """vps_memset / vps_memcpy_h2d / vps_memcpy_d2h / vps_sync through the C ABI on S: ordered behind the copy that precedes them."""
    import ctypes as C
    import torch
    n = 1 << 16
    true, decoy = torch.full((n,), 7, dtype=torch.uint8, device=K.device), torch.full((n,), 9, dtype=torch.uint8, device=K.device)
    buf = decoy.clone()
    host = np.full(n // 4, 3, dtype=np.uint8)
    back = np.zeros(n, dtype=np.uint8)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=K.device)
    with torch.cuda.stream(side):
        blocker.enqueue()
        behind = torch.cuda.Event()
        behind.record(side)
        buf.copy_(true, non_blocking=True)
        K._stream()
        K._chk(K.lib.vps_memset(K.ctx, C.c_void_p(buf.data_ptr()), 1, n // 2))
        assert not behind.query(), "blocker too short: vps_memset is a pure enqueue"
        K._chk(K.lib.vps_memcpy_h2d(K.ctx, C.c_void_p(buf.data_ptr() + n // 2), host.ctypes.data_as(C.c_void_p), n // 4))
        assert behind.query(), "vps_memcpy_h2d completes the copy from the host buffer before it returns"
        host[:] = 5                                     # free on return
        K._chk(K.lib.vps_memcpy_d2h(K.ctx, back.ctypes.data_as(C.c_void_p), C.c_void_p(buf.data_ptr()), n))
        assert behind.query(), "vps_memcpy_d2h blocks"
        K.sync()
    assert np.array_equal(back, np.concatenate([np.full(n // 2, 1), np.full(n // 4, 3), np.full(n // 4, 7)]).astype(np.uint8))


# ------------------------------------------------------------------------------------------- f: the public surface ----
@gpu
def test_public_surface(blocker):
    """GasParticles(...).deposit_to_field(64).spctrm(q) for velocity, momentum, energy, rho13_velocity and density,
    helmholtz_spctrm, ann_interp_to_field(32).spctrm('momentum') and deposit_to_grid(method="direct"): the true particles on the
    null stream, then a DECOY set of the same shapes on the null stream (the process-wide context's workspaces, tables and z images
    now hold the decoy's), then the true particles on a side stream behind the blocker.  Every side-stream table against its
    float64 oracle table (tests/weighted_ref.py, density_ref.py, helmholtz_ref.py, orc.exact_nn_lattice) at the project's bars,
    and against the null-stream run; the decoy's tables are more than 100 bars away."""
    import torch
    import density_ref as dref
    import helmholtz_ref as hr
    import weighted_ref as wref
    from oracle import vps_oracle as orc
    from vpower import interp
    N, Nn, Np, L = 64, 32, 100003, 1.0
    names = ("velocity", "momentum", "energy", "rho13_velocity", "density")

    def data(seed):
        rng = np.random.default_rng(seed)
        return (rng.random((Np, 3)).astype(np.float32), rng.standard_normal((Np, 3)).astype(np.float32),
                np.exp(0.5 * rng.standard_normal(Np)).astype(np.float32))

    def run(d):
        pos, vel, dens = d
        gp = interp.GasParticles(pos, np.ones(Np, np.float32), dens, vel, L)
        box = gp.deposit_to_field(N)
        out = {q: box.spctrm(q) for q in names}
        out["total"], out["compressive"], out["solenoidal"] = box.helmholtz_spctrm("velocity")
        out["nn"] = gp.ann_interp_to_field(Nn).spctrm("momentum")
        return out, interp.deposit_to_grid(vel[:, 0].copy(), pos, N, L, assignment="cic", method="direct")

    def oracle(d):
        pos, vel, dens = d
        grid = wref.ngp_vec_grid(pos, vel, dens, N, L)
        v, m = orc.vm_from_vec_grid(grid, L / N, zero_empty=True)
        ref = {q: orc.box_spctrm(v[..., 0], v[..., 1], v[..., 2], m, L / N, q) for q in ("velocity", "momentum", "energy")}
        ref["rho13_velocity"] = wref.table(wref.fields_from_vec_grid(grid, 1.0 / 3.0), L, N)
        ref["density"] = dref.table(dref.field(grid, 1.0), L, N)
        ref["total"], ref["compressive"], ref["solenoidal"] = hr.helmholtz_tables(v[..., 0], v[..., 1], v[..., 2], L, N)
        ax = orc.lattice_axes_library(L, Nn)
        vec = orc.density_velocity_vector(vel.astype(np.float64), dens.astype(np.float64))
        near = vec[orc.exact_nn_lattice(pos, ax, ax, ax)].reshape(Nn, Nn, Nn, 4)
        vn, mn = orc.vm_from_vec_grid(near, L / Nn, zero_empty=True)
        ref["nn"] = orc.box_spctrm(vn[..., 0], vn[..., 1], vn[..., 2], mn, L / Nn, "momentum")
        return ref, orc.deposit_assign(vel[:, 0].astype(np.float64), pos, N, L, "cic")
    true, decoy = data(11), data(12)
    ref, ref_grid = oracle(true)
    dref_, dref_grid = oracle(decoy)
    for q in ref:
        if q != "solenoidal":          # (a difference of two sums: its bar below is absolute in the total)
            assert sp.error_in_bars(dref_[q][:, 2], ref[q][:, 2], "psum") >= sp.GUARD_FACTOR, q
    null, null_grid = run(true)
    run(decoy)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        blocker.enqueue()
        got, got_grid = run(true)
    side.synchronize()
    for q in ref:
        assert np.array_equal(got[q].Nsample, ref[q][:, 3]), q
        assert np.array_equal(got[q].Nsample, null[q].Nsample), q
        if q == "solenoidal":          # tests/test_gpu_helmholtz.py: _check
            assert np.all(np.abs(got[q].Psum - ref[q][:, 2]) <= sp.PSUM_RTOL * ref["total"][:, 2]), q
            assert np.all(np.abs(got[q].Psum - null[q].Psum) <= sp.PSUM_RTOL * ref["total"][:, 2]), q
            continue
        miss = sp.error_in_bars(got[q].Psum, ref[q][:, 2], "psum")
        print("public surface %s: %.3g bars from the oracle, %.3g from the decoy's" % (q, miss, sp.error_in_bars(got[q].Psum, dref_[q][:, 2], "psum")))
        assert miss <= 1.0, "%s on a side stream misses the oracle table by %.3g bars" % (q, miss)
        assert np.allclose(got[q].Psum, null[q].Psum, rtol=sp.PSUM_RTOL, atol=0), q
    bar = 2e-5 * np.abs(ref_grid).max()                      # tests/test_gpu_assign_direct.py: test_public_surface
    assert np.abs(dref_grid - ref_grid).max() >= sp.GUARD_FACTOR * bar
    assert np.allclose(got_grid, ref_grid, rtol=0, atol=bar) and np.allclose(got_grid, null_grid, rtol=0, atol=bar)


# ------------------------------------------------------------------------------------------- g: timing ----
@gpu
def test_timing_on_a_side_stream(K, blocker):
    """K.timing(True): the launch counts per kind of a sequence on S equal those of the same sequence on the null stream; every
    interval is finite and >= 0."""
    import torch
    from vpower import device as D
    T = _parts(K, TRUE)
    f = _sep(K, N0, TRUE)
    pipe = _pipe(K, N0)
    nn = _nn_data(K, TRUE)

    def sequence():
        spec, nyq = K.deposit_fft_zy(T.pos, T.vel, T.rho, N0, 1.0, 0, N0, D.MOMENTUM)
        pipe.accumulate_spectra(spec, nyq)
        K.deposit_field(T.pos, T.vel, T.rho, N0, 1.0, 0, N0, D.VM)
        K.rfft3(f, N0)
        K.nn_resample(nn[0], nn[1], nn[2], 0, 32)
    sequence()
    torch.cuda.synchronize()
    K.timing(True)
    try:
        sequence()
        null = K.timing_get()
        side = torch.cuda.Stream(device=K.device)
        with torch.cuda.stream(side):
            K._stream()
            K.timing(True)
            blocker.enqueue()
            sequence()
            got = K.timing_get()
            lists = {name: K.timing_list(name) for name in got}
        side.synchronize()
    finally:
        K.timing(False)
    assert {k: v[0] for k, v in got.items()} == {k: v[0] for k, v in null.items()}, (got, null)
    assert sum(v[0] for v in got.values()) > 10
    for name, (n, ms) in got.items():
        assert np.isfinite(ms) and ms >= 0 and len(lists[name]) == n
        assert np.all(np.isfinite(lists[name])) and np.all(lists[name] >= 0), (name, lists[name])


# ------------------------------------------------------------------------------------------- h: the in-library exchange ----
def _exchange_worker(rank, N, Np, out_dir):
    for p in (ROOT, os.path.join(ROOT, "large-velocity-power-spectrum_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["VPS_A2A_CHUNKS"] = "4"
    torch.cuda.set_device(0)
    from vpower import _ffi, device, synth
    K = device.default_kernels(0)
    comm = device.LibraryComm(K, rank=0, world=1, uid=device.HipKernels.comm_unique_id())
    pipe = device.PowerPipeline(N, 1.0, kernels=K, comm=comm)
    assert pipe.chunked and pipe.nchunks == 4
    pt, pd = synth.particles(37, Np, 1.0), synth.particles(38, Np, 1.0)
    true = [K.to_device(pt[i]) for i in (0, 1, 3)]             # positions, velocities, densities
    decoy = [K.to_device(pd[i]) for i in (0, 1, 3)]
    bufs = [d.clone() for d in decoy]
    blocker = sp.Blocker(K.device)
    tabs = []

    def sequence():
        out = []
        for q in (device.VELOCITY, device.ENERGY):
            z = K.deposit_fft_z(bufs[0], bufs[1], bufs[2], N, 1.0, 0, N, q)
            zs = [z[i] for i in range(z.shape[0])]
            out.append(pipe.finish(*pipe.accumulate_zimages(zs)))
            out.append(pipe.finish(*pipe.accumulate_zimages(zs)))          # buffers and events re-used
        return out
    sequence()                                                            # on the decoy, null stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        blocker.enqueue()
        for b, t in zip(bufs, true):
            b.copy_(t, non_blocking=True)
        tabs += sequence()
        z = K.deposit_fft_z(bufs[0], bufs[1], bufs[2], N, 1.0, 0, N, device.VELOCITY)
        _ffi.set_option("comm_fail_send", 5)
        try:
            failed = False
            try:
                pipe.accumulate_zimages([z[i] for i in range(3)])
            except Exception as e:
                failed = "ncclSend" in str(e) and "group closed" in str(e)
            assert failed, "the injected send failure must surface as an error"
        finally:
            _ffi.set_option("comm_fail_send", None)
        blocker.enqueue()
        tabs.append(pipe.finish(*pipe.accumulate_zimages([z[i] for i in range(3)])))
    side.synchronize()
    # vps_spectrum_zimages through the C ABI with a pointer list the TEST owns: repointed at the decoy's z images as soon as the
    # call has returned (the list is read on the host, before the return), the blocker still pending behind the call and behind
    # vps_allreduce_shells -- both are pure enqueues
    import ctypes as C
    for b, t in zip(bufs, true):
        b.copy_(t)
    zt = K.deposit_fft_z(bufs[0], bufs[1], bufs[2], N, 1.0, 0, N, device.VELOCITY).clone()
    zd = K.deposit_fft_z(decoy[0], decoy[1], decoy[2], N, 1.0, 0, N, device.VELOCITY).clone()
    pipe.prepare()
    work = K.workspace("exchange", K.lib.vps_spectrum_zimages_workspace_bytes(N, N, 1, 4, 3))
    psum, ns = pipe.new_accumulators()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        K._stream()
        blocker.enqueue()
        behind = torch.cuda.Event()
        behind.record(side)
        ptrs = (C.c_void_p * 3)(*[zt[i].data_ptr() for i in range(3)])
        K._chk(K.lib.vps_spectrum_zimages(K.ctx, N, N, ptrs, 3, 4, K._ptr(work), 1, K._ptr(psum), K._ptr(ns)))
        for i in range(3):
            ptrs[i] = zd[i].data_ptr()
        K.allreduce_shells(psum, ns)
        assert not behind.query(), "blocker too short: vps_spectrum_zimages and vps_allreduce_shells are pure enqueues"
        tabs.append(pipe.finish(psum, ns))
    side.synchronize()
    np.save(os.path.join(out_dir, "tab_streams.npy"), np.stack(tabs))
    K.comm_destroy()


@gpu
def test_library_exchange_on_a_side_stream(tmp_path):
    """The velocity and energy sequence of test_library_rccl_exchange_single_rank with ctx->stream = a side stream behind a
    blocker: one-rank LibraryComm, four chunks, every call twice (events re-used), once more after the injected send failure;
    then the raw call with a pointer list of the test's own, overwritten with the decoy's z images right after the return, the
    blocker asserted pending behind it.  A fresh child process, as there."""
    import torch.multiprocessing as mp
    from oracle import vps_oracle as orc
    from vpower import synth
    N, Np = 128, 200000
    mp.spawn(_exchange_worker, args=(N, Np, str(tmp_path)), nprocs=1, join=True)
    tabs = np.load(tmp_path / "tab_streams.npy")
    refs = {}
    for seed in (37, 38):
        pos, vel, mass, dens = synth.particles(seed, Np, 1.0)
        vec = orc.density_velocity_vector(vel.astype(np.float64), dens.astype(np.float64))
        v, m = orc.vm_from_vec_grid(orc.deposit_to_grid_fast(vec, pos, N, 1.0), 1.0 / N, zero_empty=True)
        refs[seed] = {q: orc.box_spctrm(v[..., 0], v[..., 1], v[..., 2], m, 1.0 / N, q) for q in ("velocity", "energy")}
    for q in ("velocity", "energy"):
        assert sp.error_in_bars(refs[38][q][:, 2], refs[37][q][:, 2], "psum") >= sp.GUARD_FACTOR
    assert len(tabs) == 6
    for i, q in enumerate(("velocity", "velocity", "energy", "energy", "velocity", "velocity")):      # (the last: the owned pointer list)
        ref = refs[37][q]
        assert np.array_equal(tabs[i][:, 3], ref[:, 3]), (i, q)
        assert np.allclose(tabs[i][:, 2], ref[:, 2], rtol=sp.PSUM_RTOL, atol=0), (i, q)
