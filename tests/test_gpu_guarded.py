"""The library's entry points on guarded, poisoned, exact-size memory (tests/guarded.py; pinned on the CPU by
tests/test_guarded_cpu.py).  Run on an MI355X:  python -m pytest tests/test_gpu_guarded.py -q -m gpu

Every leg runs its call in three workspace states -- Z (zero-filled), D-same (as a real call of the same shape on OTHER particles
or another field left it) and D-other (as a real call of a larger shape left it, the view cut to the new size) -- on fresh
poisoned outputs each time, and asserts:
  (a) no guard of any buffer handed out during the call changed (the dirt-making calls included: they run on exact-size memory too);
  (b) no element of an output the contract says is written still holds the poison, and (fft_y_chunk in a binning-only scope) the
      elements it says are not written hold exactly the poison (include/vps_hip.h; the predicted set is computed on the host);
  (c) the result matches the route's float64 reference at the route's bar IN EACH STATE: integer payloads bit exact, images 1e-5 of
      the rms, fields 1e-5 of the maximum, neighbour indices exact;
  (d) the three states give bit-equal outputs wherever the route is deterministic on integer data (everything below except the
      velocity and weighted images of the fused route, which add q (1 / rho) in arrival order).
Data is integer-valued (rho in 1..3, v in -3..3: oracle/gpu_checks.py: constructed_particles), so float32 LDS sums are exact whatever
the arrival order.  Every leg asserts the path it took (deposit_plan, nn_plan, nn_last_search) where the route has one.
Legs: raw deposit; deposit_field; field_algebra[_out]; fused deposit_fft_zy (whole grids, last slab, thin slabs, component masks, the
share_energy and reuse_sort sequences); deposit_fft_z[_slab]; un-fused fft_z / fft_zy / rfft3; neighbours; the small producers;
the x pass; fft_y_chunk -- the one route where (b) has a non-empty predicted set -- with the chunk x pass; spectrum_zimages."""
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import density_ref as dref  # noqa: E402
import guarded as gd  # noqa: E402
from route_refs import (  # noqa: E402,F401
    P as _P, vec_grid as _vec_grid, ALPHA, reference_fields as _reference_fields, zy_reference as _zy_reference, z_reference as _z_reference, fused_refs as _fused_refs, reuse_flags as _reuse_flags, expected_chunk as _expected_chunk, NN_REF, nn_setup as _nn_setup)
import weighted_ref as wref  # noqa: E402
from oracle import gpu_checks as chk  # noqa: E402
from oracle import vps_oracle as orc  # noqa: E402

FIELD_BAR = 1e-5       # fields: max error / max |reference|
IMAGE_BAR = 1e-5       # images: max error / rms of the reference
STATES = ("Z", "D-same", "D-other")


@pytest.fixture(scope="module")
def G():
    g = gd.guarded_kernels()
    yield g
    g.release()
    g.close()
    FUSED_CASES.clear()
    NN_REF.clear()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _options(opts):
    from vpower import _ffi
    with contextlib.ExitStack() as stack:
        for k, v in opts.items():
            stack.enter_context(_ffi.option(k, v))
        yield


def _tensors(res):
    return list(res.values()) if isinstance(res, dict) else list(res) if isinstance(res, (tuple, list)) else [res]


def _checked(G, what):
    """(a) and (b) for everything handed out since the last check."""
    torch.cuda.synchronize()
    rep = G.check()
    assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
    left = [(r.name, r.shape, len(r.poison), [tuple(int(i) for i in np.unravel_index(j, r.shape)) for j in r.poison[:4].tolist()],
             tuple(int(i) for i in np.unravel_index(int(r.poison[-1]), r.shape))) for r in rep if r.kind == "empty" and len(r.poison)]
    assert left == [], "%s: elements still hold the poison (buffer, shape, count, first indices, last index): %r" % (what, left)
    return rep


def _states(G, what, run, same, other):
    """run() in the three workspace states -> {state: result}.  same(), other(): the real calls that make the dirt."""
    outs = {}
    for st in STATES:
        G.release()
        G.state = "Z"
        if st != "Z":
            (same if st == "D-same" else other)()
            _checked(G, "%s, the call before %s" % (what, st))
            G.state = "D"
        outs[st] = run()
        _checked(G, "%s, state %s" % (what, st))
    G.state = "Z"
    G.release()
    return outs


def _bit_equal(outs, what):
    """(d)"""
    z = _tensors(outs["Z"])
    for st in STATES[1:]:
        for i, (a, b) in enumerate(zip(z, _tensors(outs[st]))):
            assert torch.equal(a, b), "%s: output %d differs between Z and %s in %d elements" % (what, i, st, int((a != b).sum()))



def _dist(n):
    return "clump" if n >= 64 else "uniform"


# ------------------------------------------------------------------------------------------- raw deposit ----
def _raw_deposit(G, N, C, n, dtype, x0, nx, **expect):
    plan = G.deposit_plan(n, C, N, x0, nx)
    assert {k: plan[k] for k in expect} == expect, plan
    assert plan["nchunks"] == -(-n // 2048), plan
    t, s, o = _P(G, n, N, dtype, "uniform", 1), _P(G, n, N, dtype, _dist(n), 2), _P(G, 3 * n + 5, 96, dtype, "clump", 3)
    pay = t.payload(C)
    f = {id(p): p.payload(C).float().contiguous() for p in (t, s, o)}
    what = "deposit %d^3 rows [%d, %d) C=%d n=%d %s" % (N, x0, x0 + nx, C, n, dtype)
    outs = _states(G, what, lambda: G.deposit(t.pos, f[id(t)], N, 1.0, x0, nx), lambda: G.deposit(s.pos, f[id(s)], N, 1.0, x0, nx),
                   lambda: G.deposit(o.pos, f[id(o)], 96, 1.0, 0, 96))
    want = torch.stack([w.float() for w in chk.exact_slab_reference(t.cells, None, None, N, x0, nx, payload=pay)]).view(C, nx, N, N)
    for st, g in outs.items():
        assert g.shape == want.shape and torch.equal(g, want), "%s, state %s: %d cells differ" % (what, st, int((g != want).sum()))
    _bit_equal(outs, what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("N,x0,nx", [(48, 0, 48), (64, 0, 64), (64, 48, 16)])
def test_raw_deposit(G, N, x0, nx, C, dtype):
    _raw_deposit(G, N, C, 20011, dtype, x0, nx, two_level=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("opts,expect", [({"sort_atomic": 1}, dict(two_level=0)), ({"sort_staged": 0}, dict(two_level=1, staged=0)),
                                         ({"sort_groups": 7}, dict(two_level=1))], ids=["atomic", "unstaged", "groups7"])
def test_raw_deposit_sort_flavours(G, opts, expect, dtype):
    with _options(opts):
        if "sort_groups" in opts:
            assert G.deposit_plan(20011, 3, 64, 0, 64)["ngroups"] <= 7
        _raw_deposit(G, 64, 3, 20011, dtype, 0, 64, **expect)
        _raw_deposit(G, 64, 4, 20011, dtype, 48, 16, **expect)


@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 3 * 2048 + 77])
def test_raw_deposit_particle_counts(G, n):
    """Around one level-1 chunk of the sort (2048 particles)."""
    _raw_deposit(G, 48, 1, n, torch.float32, 0, 48, two_level=1)
    _raw_deposit(G, 64, 4, n, torch.float32, 48, 16, two_level=1)


# ------------------------------------------------------------------------------------------- per-cell fields ----
def _quantities():
    from vpower import device as D
    return {"velocity": (D.VELOCITY, 0), "momentum": (D.MOMENTUM, 0), "momentum_bug": (D.MOMENTUM, D.FLAG_REFERENCE_MOMENTUM_BUG),
            "energy": (D.ENERGY, 0), "vm": (D.VM, 0), "weighted_third": (D.WeightedVelocity(1.0 / 3.0), 0),
            "weighted_half": (D.WeightedVelocity(0.5), 0), "density_1": (D.Density(1.0), 0), "density_third": (D.Density(1.0 / 3.0), 0),
            "density_half": (D.Density(0.5), 0), "log_density": (D.LOG_DENSITY, 0)}


QUANTITY_IDS = ["velocity", "momentum", "momentum_bug", "energy", "vm", "weighted_third", "weighted_half", "density_1",
                "density_third", "density_half", "log_density"]



def _assert_fields(got, ref, what):
    assert got.shape[0] == len(ref), (what, got.shape, len(ref))
    g = got.double().cpu().numpy()
    for c, r in enumerate(ref):
        err, top = float(np.abs(g[c] - r).max()), float(np.abs(r).max())
        assert err <= FIELD_BAR * top, "%s component %d: max error %.3g against %.3g x %.3g" % (what, c, err, FIELD_BAR, top)


@pytest.fixture(scope="module")
def field_particles(G):
    N = 64
    return N, _P(G, 30011, N, torch.float32, "uniform", 11), _P(G, 30011, N, torch.float32, "clump", 12), \
        _P(G, 90038, 96, torch.float32, "clump", 13)


@pytest.fixture(scope="module")
def field_grid(field_particles):
    N, t, _, _ = field_particles
    return _vec_grid(t, N, 0, N)


@pytest.mark.parametrize("name", QUANTITY_IDS)
def test_deposit_field(G, field_particles, field_grid, name):
    N, t, s, o = field_particles
    q, flags = _quantities()[name]
    plan = G.deposit_plan(t.n, 4, N, 0, N)
    assert plan["two_level"] == 1, plan
    what = "deposit_field %s 64^3" % name
    outs = _states(G, what, lambda: G.deposit_field(t.pos, t.vel, t.rho, N, 1.0, 0, N, q, flags),
                   lambda: G.deposit_field(s.pos, s.vel, s.rho, N, 1.0, 0, N, q, flags),
                   lambda: G.deposit_field(o.pos, o.vel, o.rho, 96, 1.0, 0, 96, q, flags))
    ref = _reference_fields(field_grid, 1.0 / N, name)
    for st, g in outs.items():
        _assert_fields(g, ref, "%s, state %s" % (what, st))
    _bit_equal(outs, what)


@pytest.mark.parametrize("vm", [0, 1], ids=["rhov", "input_is_vm"])
@pytest.mark.parametrize("name", QUANTITY_IDS)
def test_field_algebra_and_field_algebra_out(G, field_particles, field_grid, name, vm):
    """No workspace: output poison and guards, the reference, and in place == out of place.  The in-place form runs on a guarded
    copy of the channels; the channels a quantity does not have must stay what they were."""
    from vpower import device as D
    N, t, _, _ = field_particles
    q, flags = _quantities()[name]
    Lcell = 1.0 / N
    G.release()
    G.state = "Z"
    if vm:
        chans = G.deposit_field(t.pos, t.vel, t.rho, N, 1.0, 0, N, D.VM).clone()
        c64 = chans.double().cpu().numpy()
        vec = np.stack([c64[0] * c64[3] / Lcell ** 3, c64[1] * c64[3] / Lcell ** 3, c64[2] * c64[3] / Lcell ** 3, c64[3] / Lcell ** 3], axis=-1)
        flags |= D.FLAG_INPUT_IS_VM
    else:
        chans = G.deposit(t.pos, t.payload(4).float().contiguous(), N, 1.0, 0, N).clone()
        vec = field_grid
    _checked(G, "the channels")
    ref = _reference_fields(vec, Lcell, name)
    keep = chans.clone()
    what = "field_algebra_out %s %s" % (name, "vm" if vm else "rhov")
    out = G.field_algebra_out(chans, q, flags, Lcell)
    _checked(G, what)
    assert torch.equal(chans, keep), "field_algebra_out only reads its input"
    _assert_fields(out, ref, what)
    inplace = G.empty(tuple(chans.shape), torch.float32)
    inplace.copy_(chans)
    G.field_algebra(inplace, q, flags, Lcell)
    _checked(G, "field_algebra (in place) %s" % name)
    n = D.NCOMP[int(q)]
    assert torch.equal(inplace[:n], out) and torch.equal(inplace[n:], keep[n:])
    G.release()


# ------------------------------------------------------------------------------------------- fused deposit + z / y passes ----


def _assert_image(got, ref, what):
    rms = float(ref.abs().square().mean().sqrt())
    err = float((got.to(torch.complex128) - ref).abs().max())
    assert err <= IMAGE_BAR * rms, "%s: max error %.3g against %.3g x rms %.3g" % (what, err, IMAGE_BAR, rms)


FUSED_NAMES = ["velocity", "momentum", "momentum_bug", "energy", "weighted_third", "density_1", "density_half", "log_density"]
ORDER_DEPENDENT = ("velocity", "weighted_third")                           # q (1 / rho) added in arrival order: (c) only
FUSED_SHAPES = [(64, 0, 64), (192, 0, 192), (128, 96, 32)]



class _Fused:
    def __init__(self, G, N, x0, nx, n, clumped=False):
        self.N, self.x0, self.nx = N, x0, nx
        self.t = _P(G, n, N, torch.float32, "clump" if clumped else "uniform", 21)
        self.s = _P(G, n, N, torch.float32, "uniform" if clumped else "clump", 22)
        # D-other: twice the line length -- or, for the thin slabs (4096 is the longest line), twice the rows
        self.No, self.nxo = (N, 2 * nx) if N >= 1024 else (2 * N, max(16, nx // 2))
        self.o = _P(G, 3 * n + 5, self.No, torch.float32, "clump", 23)

    def calls(self, G, q, flags, **kw):
        def call(p, N, x0, nx):
            return lambda: G.deposit_fft_zy(p.pos, p.vel, p.rho, N, 1.0, x0, nx, q, flags, **kw)
        return call(self.t, self.N, self.x0, self.nx), call(self.s, self.N, self.x0, self.nx), call(self.o, self.No, 0, self.nxo)


FUSED_CASES = {}


def _fused_case(G, shape):
    """Particles and float64 reference images of one shape, made once."""
    from vpower import device as D
    if shape not in FUSED_CASES:
        N, x0, nx = shape
        assert G.fused_supported(N, D.MOMENTUM) and G.fused_supported(2 * N, D.MOMENTUM)
        f = _Fused(G, N, x0, nx, 40011 if N == 64 else 150011)
        plan = G.deposit_plan(f.t.n, 4, N, x0, nx, pencil=True)
        assert plan["bx"] == 1 and plan["bz"] == N and plan["two_level"] == 1, plan
        f.refs = _fused_refs(G, f.t, N, x0, nx, FUSED_NAMES)
        FUSED_CASES[shape] = f
    return FUSED_CASES[shape]


@pytest.fixture(params=FUSED_SHAPES, ids=lambda s: "%d-x0=%d-nx=%d" % s)
def fused(G, request):
    return _fused_case(G, request.param)


@pytest.mark.parametrize("name", FUSED_NAMES)
def test_fused_deposit_fft_zy(G, fused, name):
    q, flags = _quantities()[name]
    what = "deposit_fft_zy %s %d rows [%d, %d)" % (name, fused.N, fused.x0, fused.x0 + fused.nx)
    outs = _states(G, what, *fused.calls(G, q, flags))
    for st, (spec, nyq) in outs.items():
        assert spec.shape[0] == len(fused.refs[name])
        for c, (rs, rn) in enumerate(fused.refs[name]):
            _assert_image(spec[c], rs, "%s, state %s, spec %d" % (what, st, c))
            _assert_image(nyq[c], rn, "%s, state %s, nyq %d" % (what, st, c))
    if name not in ORDER_DEPENDENT:
        _bit_equal(outs, what)


@pytest.mark.parametrize("comps", [(0,), (2,), (0, 2)], ids=["x", "z", "xz"])
def test_fused_component_masks(G, comps):
    from vpower import device as D
    fused = _fused_case(G, FUSED_SHAPES[0])
    what = "deposit_fft_zy momentum components %r" % (comps,)
    outs = _states(G, what, *fused.calls(G, D.MOMENTUM, 0, component=comps))
    for st, (spec, nyq) in outs.items():
        assert spec.shape[0] == len(comps) and nyq.shape[0] == len(comps)
        for i, c in enumerate(comps):
            _assert_image(spec[i], fused.refs["momentum"][c][0], "%s, state %s, spec %d" % (what, st, c))
            _assert_image(nyq[i], fused.refs["momentum"][c][1], "%s, state %s, nyq %d" % (what, st, c))
    _bit_equal(outs, what)



def _sequence(G, f, steps):
    """steps: [(quantity, flags, kwargs)] on one workspace, every call after the first with the token of the one before."""
    def run_on(p, N, x0, nx):
        def run():
            res, tok, ptrs = [], None, []
            with G.sequence(), _reuse_flags(G) as taken:
                for q, flags, kw in steps:
                    res += list(G.deposit_fft_zy(p.pos, p.vel, p.rho, N, 1.0, x0, nx, q, flags, reuse_sort=tok, **kw))
                    tok = G.fused_token()
                    ptrs.append(tok[10])                                   # work.data_ptr() inside the token
            from vpower import device as D
            assert taken == [0] + [D.FLAG_REUSE_SORT] * (len(steps) - 1), taken
            assert len(set(ptrs)) == 1, "the sequence must stay on one workspace"
            return res
        return run
    return run_on(f.t, f.N, f.x0, f.nx), run_on(f.s, f.N, f.x0, f.nx), run_on(f.o, f.No, 0, f.nxo)


def test_fused_share_energy_sequence(G, fused):
    """momentum -> energy under share_energy: the energy call only runs its y pass on the z image the momentum launch left."""
    from vpower import device as D
    what = "share_energy %d" % fused.N
    outs = _states(G, what, *_sequence(G, fused, [(D.MOMENTUM, 0, dict(share_energy=True)), (D.ENERGY, 0, dict(share_energy=True))]))
    for st, res in outs.items():
        for c in range(3):
            _assert_image(res[0][c], fused.refs["momentum"][c][0], "%s, state %s, momentum %d" % (what, st, c))
            _assert_image(res[1][c], fused.refs["momentum"][c][1], "%s, state %s, momentum nyq %d" % (what, st, c))
        _assert_image(res[2][0], fused.refs["energy"][0][0], "%s, state %s, energy" % (what, st))
        _assert_image(res[3][0], fused.refs["energy"][0][1], "%s, state %s, energy nyq" % (what, st))
    _bit_equal(outs, what)


def test_fused_reuse_sort_sequence(G, fused):
    """velocity -> momentum -> energy on one sort (the reuse_sort token)."""
    from vpower import device as D
    what = "reuse_sort %d" % fused.N
    outs = _states(G, what, *_sequence(G, fused, [(D.VELOCITY, 0, {}), (D.MOMENTUM, 0, {}), (D.ENERGY, 0, {})]))
    for st, res in outs.items():
        for c in range(3):
            _assert_image(res[0][c], fused.refs["velocity"][c][0], "%s, state %s, velocity %d" % (what, st, c))
            _assert_image(res[2][c], fused.refs["momentum"][c][0], "%s, state %s, momentum %d" % (what, st, c))
            _assert_image(res[1][c], fused.refs["velocity"][c][1], "%s, state %s, velocity nyq %d" % (what, st, c))
            _assert_image(res[3][c], fused.refs["momentum"][c][1], "%s, state %s, momentum nyq %d" % (what, st, c))
        _assert_image(res[4][0], fused.refs["energy"][0][0], "%s, state %s, energy" % (what, st))
        _assert_image(res[5][0], fused.refs["energy"][0][1], "%s, state %s, energy nyq" % (what, st))
    _bit_equal({st: res[2:] for st, res in outs.items()}, what)


THIN_NAMES = ["velocity", "momentum", "energy"]
# 8-row slabs of the long lines (1024: 8-line pencils; 2048: the wide y pass; 4096: the split kernel for energy) and, at 128, a whole
# grid whose TESTED particles are the clumped ones: 44 particles per cell in 2 x 16 pencils, 5600 records a pencil
THIN_SHAPES = [(1024, 504, 8, False), (2048, 1000, 8, False), (4096, 3000, 8, False), (128, 0, 128, True)]


@pytest.mark.parametrize("N,x0,nx,clumped", THIN_SHAPES, ids=lambda v: str(v))
def test_fused_thin_slabs_and_overfull_pencils(G, N, x0, nx, clumped):
    from vpower import device as D
    assert G.fused_supported(N, D.ENERGY)
    f = _Fused(G, N, x0, nx, 600011, clumped)
    plan = G.deposit_plan(f.t.n, 4, N, x0, nx, pencil=True)
    assert plan["bx"] == 1 and plan["bz"] == N and plan["two_level"] == 1, plan
    if clumped:
        per_pencil = torch.bincount(f.t.cells[:, 0].long() * N + f.t.cells[:, 1].long())
        assert int(per_pencil.max()) > 4096, "the clump is meant to fill pencils far beyond one workgroup's registers"
    sums = chk.exact_slab_reference(f.t.cells, f.t.rho, f.t.vel, N, x0, nx)      # (134 million cells at 4096: on the device)
    fields = chk.ngp_fields_float64(sums[0].double(), [a.double() for a in sums[1:]], (1.0 / N) ** 3, THIN_NAMES)
    del sums
    refs = {name: [_zy_reference(c.view(nx, N, N), N, nx) for c in fields[name]] for name in THIN_NAMES}
    del fields
    for name in THIN_NAMES:
        q, flags = _quantities()[name]
        what = "deposit_fft_zy %s %d rows [%d, %d)%s" % (name, N, x0, x0 + nx, " clumped" if clumped else "")
        outs = _states(G, what, *f.calls(G, q, flags))
        for st, (spec, nyq) in outs.items():
            for c, (rs, rn) in enumerate(refs[name]):
                _assert_image(spec[c], rs, "%s, state %s, spec %d" % (what, st, c))
                _assert_image(nyq[c], rn, "%s, state %s, nyq %d" % (what, st, c))
        if name not in ORDER_DEPENDENT:
            _bit_equal(outs, what)
        del outs



@pytest.mark.parametrize("x0", [0, 96])
@pytest.mark.parametrize("bound", ["none", "count_in_slab", "loose"])
def test_fused_deposit_fft_z_and_its_slab_form(G, x0, bound):
    """128, 32 rows, replicated particles.  count_in_slab: the compacted layout (recompute = 1, cap_in > cap: the slack region);
    loose: a bound so close to all particles that the layout falls back to sorting them all (recompute = 0)."""
    from vpower import device as D
    # the compaction pays only where the slab's particles + 2048 blocks of 2048 slots are fewer than half of all particles
    N, nx, n = 128, 32, 20_000_003 if bound == "count_in_slab" else 600011
    t, s, o = _P(G, n, N, torch.float32, "uniform", 31), _P(G, n, N, torch.float32, "clump", 32), _P(G, 3 * n + 5, 256, torch.float32, "clump", 33)

    def slab_particles(p, N_, x0_, nx_):
        inside = G.count_in_slab(p.pos, N_, 1.0, x0_, nx_)
        assert inside == int(((p.cells[:, 0] >= x0_) & (p.cells[:, 0] < x0_ + nx_)).sum())
        return {"none": None, "count_in_slab": inside, "loose": p.n - 1}[bound]
    sp = {id(p): slab_particles(p, *shape) for p, shape in ((t, (N, x0, nx)), (s, (N, x0, nx)), (o, (256, 0, 64)))}
    if bound == "count_in_slab":       # D-same is the same SHAPE: the same bound (the clump lies outside both slabs, so it holds)
        assert sp[id(s)] <= sp[id(t)]
        sp[id(s)] = sp[id(t)]
    plan = G.deposit_plan(n, 4, N, x0, nx, pencil=True, slab_particles=sp[id(t)])
    if bound == "count_in_slab":
        assert plan["recompute"] == 1 and plan["cap_in"] > sp[id(t)], plan
    else:
        assert plan["recompute"] == 0 and plan["cap_in"] == n, plan
    vec = _vec_grid(t, N, x0, nx)
    for name in ("momentum", "energy"):
        q, flags = _quantities()[name]
        refs = [_z_reference(torch.as_tensor(np.ascontiguousarray(f), device=G.device), N) for f in _reference_fields(vec, 1.0 / N, name)]
        what = "deposit_fft_z %s 128 rows [%d, %d), bound %s" % (name, x0, x0 + nx, bound)
        outs = _states(G, what, lambda: G.deposit_fft_z(t.pos, t.vel, t.rho, N, 1.0, x0, nx, q, flags, slab_particles=sp[id(t)]),
                       lambda: G.deposit_fft_z(s.pos, s.vel, s.rho, N, 1.0, x0, nx, q, flags, slab_particles=sp[id(s)]),
                       lambda: G.deposit_fft_z(o.pos, o.vel, o.rho, 256, 1.0, 0, 64, q, flags, slab_particles=sp[id(o)]))
        for st, zimg in outs.items():
            assert zimg.shape == (len(refs), G.zimage_elems(N, nx))
            for c, r in enumerate(refs):
                _assert_image(zimg[c], r, "%s, state %s, component %d" % (what, st, c))
        _bit_equal(outs, what)


# ------------------------------------------------------------------------------------------- un-fused FFT ----
# (N, nx, x0) -> the larger shape of D-other
FFT_SHAPES = {(64, 64, 0): (128, 128), (250, 250, 0): (384, 384), (384, 48, 96): (384, 96), (1024, 16, 480): (1024, 32)}


@pytest.mark.parametrize("weighted", [0, 1], ids=["plain", "weighted"])
@pytest.mark.parametrize("N,nx,x0", list(FFT_SHAPES), ids=lambda v: str(v))
def test_unfused_fft_zy_and_fft_z(G, N, nx, x0, weighted):
    """Rank-3 separable fields (oracle/gpu_checks.py); D-same is another field of the same shape."""
    No, nxo = FFT_SHAPES[(N, nx, x0)]
    f = chk.separable_slab(G.device, chk.separable_factors(N, seed=1), x0, nx)
    w = chk.separable_slab(G.device, chk.separable_factors(N, seed=2), x0, nx) if weighted else None
    fs = chk.separable_slab(G.device, chk.separable_factors(N, seed=3), x0, nx)
    fo = chk.separable_slab(G.device, chk.separable_factors(No, seed=4), 0, nxo)
    prod = f.double() * w.double() if weighted else f.double()
    rs, rn = _zy_reference(prod, N, nx)
    what = "fft_zy %d nx=%d%s" % (N, nx, " weighted" if weighted else "")
    outs = _states(G, what, lambda: G.fft_zy(f, N, nx, weight=w), lambda: G.fft_zy(fs, N, nx, weight=w), lambda: G.fft_zy(fo, No, nxo))
    for st, (spec, nyq) in outs.items():
        _assert_image(spec, rs, "%s, state %s, spec" % (what, st))
        _assert_image(nyq, rn, "%s, state %s, nyq" % (what, st))
    _bit_equal(outs, what)
    del outs, rs, rn
    # the z pass alone (no workspace): B[x][kz][y] for kz < N/2, then the Nyquist plane BN[x][y]
    G.state = "Z"
    zimg = G.fft_z(f, N, nx, weight=w)
    assert [r.kind for r in _checked(G, "fft_z %d" % N)] == ["empty"], "fft_z takes no workspace: one state is all there is"
    Z = torch.fft.rfft(prod, dim=2)                                        # [x, y, kz]
    ref = torch.cat([Z[:, :, : N // 2].permute(0, 2, 1).reshape(-1), Z[:, :, N // 2].reshape(-1)])
    assert zimg.numel() == ref.numel() == G.zimage_elems(N, nx)
    _assert_image(zimg, ref, "fft_z %d nx=%d" % (N, nx))
    G.release()


def test_rfft3(G):
    N = 64
    f = chk.separable_slab(G.device, chk.separable_factors(N, seed=5), 0, N)
    fs = chk.separable_slab(G.device, chk.separable_factors(N, seed=6), 0, N)
    fo = chk.separable_slab(G.device, chk.separable_factors(128, seed=7), 0, 128)
    outs = _states(G, "rfft3 64", lambda: G.rfft3(f, N), lambda: G.rfft3(fs, N), lambda: G.rfft3(fo, 128))
    ref = torch.fft.rfftn(f.double()).permute(2, 1, 0)                     # [kz <= N/2, ky, kx]
    for st, got in outs.items():
        _assert_image(got, ref, "rfft3 64, state %s" % st)
    _bit_equal(outs, "rfft3 64")


# ------------------------------------------------------------------------------------------- neighbours ----



def _nn_leg(G, n, lattice, x0, nx, opts, quantities=()):
    M = lattice[1]
    plan = G.nn_plan(n)
    assert plan["sorted"] == int(n >= 16384) and plan["nchunks"] == -(-n // 4096), plan
    pos, pay, axes, idx = _nn_setup(G, n, lattice, x0, nx, 1)
    ps, pays, _, _ = _nn_setup(G, n, lattice, x0, nx, 2, ref=False)      # the same count from another seed
    po, payo, axo, _ = _nn_setup(G, 3 * n, ("uniform", 40), 0, 40, 3, ref=False)
    kind = chk.nn_search_kind(lattice, opts)
    want = pay[idx].t().contiguous().reshape(4, nx, M, M)
    vec = pay[idx].double().cpu().numpy().reshape(nx, M, M, 4)
    with _options(opts):
        def run():
            out, got = G.nn_resample(pos, pay, axes, x0, nx, want_index=True)
            assert G.nn_last_search()["kind"] == kind, G.nn_last_search()
            return out, got
        what = "nn_resample %d particles %r rows [%d, %d) %r" % (n, lattice, x0, x0 + nx, opts)
        outs = _states(G, what, run, lambda: G.nn_resample(ps, pays, axes, x0, nx, want_index=True),
                       lambda: G.nn_resample(po, payo, axo, 0, 40, want_index=True))
        for st, (out, got) in outs.items():
            bad = int((got.reshape(-1).to(torch.int64) != idx).sum())
            assert bad == 0, "%s, state %s: %d neighbours differ" % (what, st, bad)
            assert torch.equal(out, want), "%s, state %s: the output is not the payload of the nearest particles" % (what, st)
        _bit_equal(outs, what)
        for name in quantities:
            q, flags = _quantities()[name]
            Lcell = 1.0 / M
            whatq = "nn_resample_quantity %s %r" % (name, opts)
            outs = _states(G, whatq, lambda: G.nn_resample_quantity(pos, pay, axes, x0, nx, Lcell, q, flags, want_index=True),
                           lambda: G.nn_resample_quantity(ps, pays, axes, x0, nx, Lcell, q, flags, want_index=True),
                           lambda: G.nn_resample_quantity(po, payo, axo, 0, 40, 1.0 / 40, q, flags, want_index=True))
            ref = _reference_fields(vec, Lcell, name)
            for st, (out, got) in outs.items():
                assert torch.equal(got.reshape(-1).to(torch.int64), idx), (whatq, st)
                _assert_fields(out, ref, "%s, state %s" % (whatq, st))
            _bit_equal(outs, whatq)


@pytest.mark.parametrize("opts", [{"nn_column": 1}, {"nn_column": 0}, {"nn_query_centric": 1}, {"nn_build_atomic": 1}],
                         ids=["column", "scatter", "query_centric", "build_atomic"])
def test_nn_whole_lattice(G, opts):
    """32^3 lattice, 2e4 float32 particles: a 10 % clump, 1000 duplicates at higher indices (oracle/gpu_checks.py)."""
    _nn_leg(G, 20000, ("uniform", 32), 0, 32, opts, quantities=QUANTITY_IDS if opts == {"nn_column": 1} else ("momentum", "density_half"))


def test_nn_jittered_lattice_takes_the_ring_search(G):
    _nn_leg(G, 20000, ("jittered", 32), 0, 32, {})


def test_nn_slab(G):
    _nn_leg(G, 20000, ("uniform", 32), 24, 8, {}, quantities=("vm",))


@pytest.mark.parametrize("n", [16383, 16384, 16385])
def test_nn_switch_into_the_bucket_sort(G, n):
    _nn_leg(G, n, ("uniform", 32), 0, 32, {})
    NN_REF.clear()


# ------------------------------------------------------------------------------------------- small producers ----
@pytest.fixture(scope="module")
def T(G):
    return G.device_info()["num_cu"] * 8 * 256


@pytest.mark.parametrize("count", [1, 65, 257, "T+1"])
def test_small_producers(G, T, count):
    """cell_index, density_velocity_vector, assign_expand (CIC and TSC), hist_pairs: output poison and guards at counts around a
    wave, a workgroup and one trip of the capped grids; the exact ones against the oracle as well."""
    n = T + 1 if count == "T+1" else count
    rng = np.random.default_rng(n)
    N, L = 96, 2.5
    pos = (rng.random((n, 3)) * L).astype(np.float32)
    vel = rng.integers(-3, 4, (n, 3)).astype(np.float32)
    rho = rng.integers(1, 4, n).astype(np.float32)
    dp, dv, dr = G.to_device(pos), G.to_device(vel), G.to_device(rho)
    G.release()
    G.state = "Z"
    ci = G.cell_index(dp, N, L)
    _checked(G, "cell_index %d" % n)
    assert np.array_equal(ci.cpu().numpy(), orc.cell_index(pos, N, L))
    vec = G.density_velocity_vector(dv, dr)
    _checked(G, "density_velocity_vector %d" % n)
    assert np.array_equal(vec.cpu().numpy(), orc.density_velocity_vector(vel, rho))
    for assignment, S in (("cic", 8), ("tsc", 27)):
        pe, fe = G.assign_expand(dp, vec, N, L, assignment)
        _checked(G, "assign_expand %s %d" % (assignment, n))
        assert pe.shape == (n * S, 3) and fe.shape == (n * S, 4)
        tot = fe.double().sum(dim=0).cpu().numpy()
        want = orc.density_velocity_vector(vel, rho).astype(np.float64)
        assert np.all(np.abs(tot - want.sum(axis=0)) <= 27 * 16 * 2.0 ** -24 * np.abs(want).sum(axis=0))
    edges = np.linspace(0.0, 1.0, 33)
    k = rng.random(n)
    wts = rng.integers(1, 1 << 20, n).astype(np.float64) / 1024.0
    psum, ns = G.hist_pairs(G.to_device(k), G.to_device(wts), edges)
    _checked(G, "hist_pairs %d" % n)
    assert np.array_equal(ns.cpu().numpy(), np.histogram(k, bins=edges)[0])
    assert np.allclose(psum.cpu().numpy(), np.histogram(k, bins=edges, weights=wts)[0], rtol=1e-12, atol=0)
    G.release()


def test_pair_k_and_power_grid(G):
    N, L = 48, 2.5
    ks = orc.k_axis(L, N)
    G.release()
    G.state = "Z"
    got = G.pair_k(ks, ks * 1.5, ks[::-1].copy())
    _checked(G, "pair_k")
    kx, ky, kz = np.meshgrid(ks, ks * 1.5, ks[::-1].copy(), indexing="ij")
    assert np.array_equal(got.cpu().numpy(), np.sqrt((kx * kx + ky * ky) + kz * kz).ravel())
    fields = [chk.separable_slab(G.device, chk.separable_factors(64, seed=s), 0, 64) for s in (8, 9)]
    other = [chk.separable_slab(G.device, chk.separable_factors(128, seed=10), 0, 128)]
    outs = _states(G, "power_grid 64", lambda: G.power_grid(fields, 64), lambda: G.power_grid(fields[::-1], 64),
                   lambda: G.power_grid(other, 128))
    ref = sum(torch.fft.rfftn(f.double()).permute(2, 1, 0).abs().square() for f in fields)
    for st, g in outs.items():
        err = float((g.double() - ref).abs().max())
        assert err <= FIELD_BAR * float(ref.max()), ("power_grid", st, err)
    _bit_equal(outs, "power_grid 64")


# ------------------------------------------------------------------------------------------- x pass ----
def test_fft_x_write_at_384(G):
    """The write-mode x pass on the guarded spectrum of fft_zy: every mode of the half spectrum against numpy's rfftn.
    (State Z only: the x pass takes no workspace; the three states of the `fft` key are test_unfused_fft_zy_and_fft_z's.)"""
    N = 384
    f = chk.separable_slab(G.device, chk.separable_factors(N, seed=11), 0, N)
    G.release()
    G.state = "Z"
    spec, nyq = G.fft_zy(f, N, N)
    out = G.empty((N // 2, N, N), torch.complex64)
    G.fft_x_write(spec, N, N // 2 * N, 1, 0, out)
    outn = G.empty((1, N, N), torch.complex64)
    G.fft_x_write(nyq, N, N, 1, 0, outn)
    _checked(G, "fft_x_write 384")
    ref = torch.fft.rfftn(f.double()).permute(2, 1, 0)                     # [kz <= N/2, ky, kx]
    _assert_image(out, ref[: N // 2], "fft_x_write 384")
    _assert_image(outn[0], ref[N // 2], "fft_x_write 384, Nyquist plane")
    G.release()


@pytest.mark.parametrize("N", [64, 128])
def test_binning_x_pass_whole_grid(G, N):
    """fft_x_bin_multi and fft_x_bin_helmholtz (through PowerPipeline.accumulate_spectra[_helmholtz] with the guarded kernels: the
    accumulators come from the guarded zeros) on guarded spectra; both states of `count`.  (State Z only: the x pass takes no
    workspace.)"""
    import helmholtz_ref as hr
    from vpower import device as D
    from test_gpu_helmholtz import _check as check_helmholtz
    comps = [chk.separable_factors(N, seed=20 + c) for c in range(3)]
    fields = [chk.separable_slab(G.device, c, 0, N) for c in comps]
    G.release()
    G.state = "Z"
    pipe = D.PowerPipeline(N, 1.0, kernels=G, comm=D.SlabComm(enabled=False))
    zy = [G.fft_zy(f, N, N) for f in fields]
    spec, nyq = torch.stack([z[0] for z in zy]), torch.stack([z[1] for z in zy])
    _checked(G, "fft_zy of the three components")
    ref_ps, ref_ns = chk.separable_shell_sums(G.device, comps, N, 1.0, pipe.k2, pipe.thr)
    assert np.array_equal(ref_ns, chk.shell_counts_exact(G.device, N, pipe.k2, pipe.thr))
    psum, ns = pipe.accumulate_spectra(spec, nyq)
    rep = _checked(G, "fft_x_bin_multi %d" % N)
    assert any(r.kind == "zeros" for r in rep), "the accumulators must come from the guarded zeros"
    tab = pipe.finish(psum, ns)
    assert np.array_equal(tab[:, 3], ref_ns)
    assert np.allclose(tab[:, 2], ref_ps, rtol=2e-5, atol=0)
    before, p1 = ns.clone(), psum.clone()
    pipe.accumulate_spectra(spec, nyq, psum, ns, count=False)
    torch.cuda.synchronize()
    assert torch.equal(ns, before), "count=False must leave nsample as it was, bit for bit"
    nmax = float(ref_ns.max())
    assert bool(((psum - 2 * p1).abs() <= 2 * nmax * 2.0 ** -53 * (2 * p1).abs()).all())   # the same terms in another order
    tabs = pipe.finish_helmholtz(*pipe.accumulate_spectra_helmholtz(spec, nyq))
    _checked(G, "fft_x_bin_helmholtz %d" % N)
    check_helmholtz(tabs, hr.separable_helmholtz_sums(G.device, comps, N, 1.0, pipe.k2, pipe.thr), ("guarded", N))
    G.release()


# ------------------------------------------------------------------------------------------- the chunked slab exchange ----
def _k_pipeline(G, N, name):
    from vpower import device as D
    L = chk.k_range_box(name, N)
    flavour, kmin, kmax, kres = chk.k_range(name, N, L)
    return D.PowerPipeline(N, L, kernels=G, comm=D.SlabComm(enabled=False), flavour=flavour, kmin=kmin, kmax=kmax, kres=kres)



def _chunk_checked(G, what, out, want, stored, rms):
    """(a) for everything handed out; (b) STRICT for the send buffer `out`: the elements that still hold the poison are exactly
    the ones the contract leaves unwritten; (c) every other element is right."""
    torch.cuda.synchronize()
    rep = G.check()
    assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
    left = torch.zeros(out.numel(), dtype=torch.bool)
    left[gd.report_of(rep, out).poison] = True
    left = left.to(out.device)
    extra, missing = torch.nonzero(left & stored).reshape(-1), torch.nonzero(~left & ~stored).reshape(-1)
    assert extra.numel() == 0 and missing.numel() == 0, (
        "%s: %d elements the contract says are stored still hold the poison (first %r); %d it says are not stored were written "
        "(first %r); buffer of %d" % (what, extra.numel(), extra[:6].tolist(), missing.numel(), missing[:6].tolist(), out.numel()))
    err = float((out.to(torch.complex128) - want)[stored].abs().max()) if bool(stored.any()) else 0.0
    assert err <= IMAGE_BAR * rms, "%s: max error %.3g against %.3g x rms %.3g" % (what, err, IMAGE_BAR, rms)
    return int((~stored).sum())


@pytest.mark.parametrize("scope", ["plain", "binning_only"])
@pytest.mark.parametrize("name", ["deep", "band", "corner"])
@pytest.mark.parametrize("N,R,C", [(128, 4, 2), (250, 5, 5)], ids=["128-4ranks-2chunks", "250-5ranks-5chunks"])
def test_fft_y_chunk_and_the_chunk_x_pass(G, N, R, C, name, scope):
    """Every chunk of every sender slab into a poisoned send buffer, then the chunk form of the binning x pass on every receiver
    (the all-to-all played by slicing), with the accumulators from the guarded zeros; at (128, 4, 2) three components, so that
    the Helmholtz chunk form runs as well.  No workspace on this route: one state."""
    import contextlib as cl
    import helmholtz_ref as hr
    from test_gpu_helmholtz import _check as check_helmholtz
    nx, ncomp = N // R, 3 if N == 128 else 1
    comps = [chk.separable_factors(N, seed=40 + i) for i in range(ncomp)]
    G.release()
    G.state = "Z"
    pipe = _k_pipeline(G, N, name)
    pipe.prepare()
    packed = scope == "binning_only"
    enter = G.binning_only if packed else cl.nullcontext
    kcut = chk.row_cut(N, pipe.k2, pipe.thr) if packed else None
    zimgs, refs = [], []
    for f in comps:
        slabs = [chk.separable_slab(G.device, f, g * nx, nx) for g in range(R)]
        zimgs.append([G.fft_z(s_, N, nx) for s_ in slabs])
        refs.append([_zy_reference(s_.double(), N, nx) for s_ in slabs])
    _checked(G, "fft_z of the sender slabs")
    rms = float(torch.cat([r[0].reshape(-1) for r in refs[0]]).abs().square().mean().sqrt())
    unstored, chunks = 0, []
    for c in range(C):
        with enter():
            assert bool(G.y_packed(N)) == packed
            blk = G.chunk_block(N, nx, R, C, c, packed)
            if packed:
                assert blk == chk.packed_block(kcut, N, nx, R, C, c)
            sends = []
            for i in range(ncomp):
                sends.append([])
                for g in range(R):
                    out = G.fft_y_chunk(zimgs[i][g], N, nx, R, C, c)
                    want, stored = _expected_chunk(refs[i][g][0], refs[i][g][1], N, nx, R, C, c, kcut)
                    assert out.numel() == R * blk == want.numel()
                    unstored += _chunk_checked(G, "fft_y_chunk %d %s %s chunk %d sender %d component %d" % (N, name, scope, c, g, i),
                                               out, want, stored, rms)
                    sends[-1].append(out)
        chunks.append((blk, sends))
    # (the accumulators only now: check() lets go of what it has reported, and their guards are checked after the x passes)
    acc = pipe.new_accumulators()
    acch = pipe.new_accumulators(helmholtz=True) if ncomp == 3 else None
    for c, (blk, sends) in enumerate(chunks):
        for h in range(R):
            recv = [torch.cat([s_[g][h * blk:(h + 1) * blk] for g in range(R)]) for s_ in sends]
            G.fft_x_bin_chunk(recv, N, nx, R, C, c, h, packed, acc[0], acc[1])
            if acch is not None:
                G.fft_x_bin_chunk_helmholtz(recv, N, nx, R, C, c, h, packed, acch[0], acch[1], acch[2])
        if c == C - 1:                                               # both states of count: the sums again, the counts untouched
            before, p1 = acc[1].clone(), acc[0].clone()
            for h in range(R):
                recv = [torch.cat([s_[g][h * blk:(h + 1) * blk] for g in range(R)]) for s_ in sends]
                G.fft_x_bin_chunk(recv, N, nx, R, C, c, h, packed, acc[0], acc[1], count=False)
            torch.cuda.synchronize()
            assert torch.equal(acc[1], before), "count=False must leave nsample as it was, bit for bit"
            acc[0].copy_(p1)
    rep = _checked(G, "fft_x_bin_chunk %d %s %s" % (N, name, scope))
    assert sum(r.kind == "zeros" for r in rep) == (2 if acch is not None else 1)
    if packed and name in ("deep", "band"):
        assert unstored > 0, "the row cut of this k range is meant to leave rows unstored"
    if not packed:
        assert unstored == 0
    ref_ps, ref_ns = chk.separable_shell_sums(G.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
    assert np.array_equal(ref_ns, chk.shell_counts_exact(G.device, N, pipe.k2, pipe.thr))
    tab = pipe.finish(acc[0], acc[1])
    assert np.array_equal(tab[:, 3], ref_ns)
    assert np.allclose(tab[:, 2], ref_ps, rtol=2e-5, atol=0)
    if acch is not None:
        check_helmholtz(pipe.finish_helmholtz(*acch), hr.separable_helmholtz_sums(G.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr),
                        ("guarded chunk form", N, name, scope))
    G.release()


@pytest.mark.parametrize("C", [2, 4])
def test_spectrum_zimages_on_the_two_slot_exchange_workspace(G, C):
    """vps_spectrum_zimages on a one-rank communicator at 128: y pass, grouped send / receive and chunk x pass inside the library,
    on the exact two-slot `exchange` workspace, twice on the SAME workspace (one unit: the second call finds what the first left
    in both slots), in the three states."""
    from vpower import device as D
    N, ncomp = 128, 3
    comps = [chk.separable_factors(N, seed=60 + i) for i in range(ncomp)]
    other = [chk.separable_factors(N, seed=70 + i) for i in range(ncomp)]
    big = [chk.separable_factors(256, seed=80 + i) for i in range(ncomp)]
    pipe = D.PowerPipeline(N, 1.0, kernels=G, comm=D.SlabComm(enabled=False))
    pipe_big = D.PowerPipeline(256, 1.0, kernels=G, comm=D.SlabComm(enabled=False))
    G.release()
    G.state = "Z"
    z = {id(f): [G.fft_z(chk.separable_slab(G.device, c, 0, n_), n_, n_).clone() for c in f] for f, n_ in ((comps, N), (other, N), (big, 256))}
    _checked(G, "fft_z")
    per_chunk = [G.lib.vps_fft_y_chunk_elems(N, N, 1, C, c) for c in range(C)]
    assert G.lib.vps_spectrum_zimages_workspace_bytes(N, N, 1, C, ncomp) == 2 * 2 * ncomp * max(per_chunk) * 8
    G.comm_create(0, 1, D.HipKernels.comm_unique_id())
    try:
        def run_on(f, p, n_):
            def run():
                p.prepare()
                res, ptrs = [], set()
                with G.sequence():
                    for _ in range(2):
                        psum, ns = G.zeros((p.nbins,), torch.float64), G.zeros((p.nbins,), torch.int64)
                        G.spectrum_zimages(z[id(f)], n_, n_, C, psum, ns)
                        ptrs.add(G._kept["exchange"].payload().data_ptr())
                        res += [psum, ns]
                assert len(ptrs) == 1, "the two calls must run on one workspace"
                return res
            return run
        outs = _states(G, "spectrum_zimages 128, %d chunks" % C, run_on(comps, pipe, N), run_on(other, pipe, N), run_on(big, pipe_big, 256))
    finally:
        G.comm_destroy()
    ref_ps, ref_ns = chk.separable_shell_sums(G.device, comps, N, 1.0, pipe.k2, pipe.thr)
    nmax = float(ref_ns.max())
    for st, res in outs.items():
        for psum, ns in ((res[0], res[1]), (res[2], res[3])):
            tab = pipe.finish(psum, ns)
            assert np.array_equal(tab[:, 3], ref_ns), st
            assert np.allclose(tab[:, 2], ref_ps, rtol=2e-5, atol=0), st
        assert torch.equal(res[1], outs["Z"][1]) and torch.equal(res[3], outs["Z"][3])                # Nsample: bit-equal
        for i in (0, 2):                                                  # Psum: the same terms, added in another order
            assert bool(((res[i] - outs["Z"][i]).abs() <= 2 * nmax * 2.0 ** -53 * outs["Z"][i].abs()).all()), (st, i)
