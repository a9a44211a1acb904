"""Exact neighbour parity of the NN resampler -- cell list by the two-level bucket sort or the counting sort, then the column,
scatter or ring search and the exact fallback -- at the cell-list geometries the production particle counts select, against
float64 references computed on the device (oracle/gpu_checks.py: nn_slab_reference with its proof, nn_brute_force for every
point the proof does not cover; both pinned to the oracle by tests/test_nn_reference_cpu.py).

The particles (chk.nn_matrix_particles) are uniform in the unit box with a tenth of them in a Gaussian clump (sigma 0.01), an empty
box of ten lattice steps, a thousand duplicates at higher indices (exact ties), a few particles on lattice points, and a lattice
that reaches half a step beyond them.  Every leg (chk.NN_MATRIX) asserts its geometry through K.nn_plan, then per slab and
option set: indices bit-equal to the reference at EVERY point of the slab, the output bit-equal to the payload gathered at the
reference's indices, the search kind through K.nn_last_search, and 512 random points of the leg's slabs brute-forced against
the reference itself.  Legs:
  a. coverage guard: gshift 14 and 15, more than 512 groups, the largest sorted geometry, the counting sort and C3's own plan are
     in the matrix;
  b. the legs of chk.NN_MATRIX: 3.3e6 particles on a whole 64^3 lattice (groups of 8192 cells: the first geometry whose level-2
     counter scan takes two rounds); 7e6 particles on the whole 192^3 lattice under the default, scatter and ring searches; 1.4e7
     (float64 positions) ... 1.05e8 particles on slabs at the first, middle and last rows of 256^3 ... 448^3 lattices and of the
     1024^3 library lattice, and 5e7 on a jittered (non-uniform) lattice;
  c. the edges of the switch into the bucket sort (4 chunks of 4096 particles) on a whole 32^3 lattice, against brute force alone;
  d. (last) the legs that ran cover what leg a counted."""
import contextlib
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import gpu_checks as chk  # noqa: E402

C3_PARTICLES = 50_000_000
RANDOM_POINTS = 512      # per leg, dealt out evenly over its slabs
RAN = []     # (leg name, plan, search kind) of every run


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()


def _free(K):
    K._work.clear()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _options(opts):
    """Library options for the duration of the block; restored in a finally."""
    from vpower import _ffi
    prev = {k: _ffi.OPTIONS.get(k) for k in opts}
    try:
        for k, v in opts.items():
            _ffi.set_option(k, v)
        yield
    finally:
        for k, v in prev.items():
            _ffi.set_option(k, v)


def _plan(K, leg):
    return K.nn_plan(leg["n"], leg["dtype"] == "float64")


def _cells(pos, plan, idx):
    """Cell of the cell list (the kernels' rule: floor((p - lo) M / extent) per axis, clamped, x-major) of the particles idx."""
    M = plan["M"]
    lo, hi = pos.min(dim=0).values.double(), pos.max(dim=0).values.double()
    ext = torch.where(hi > lo, hi - lo, torch.ones_like(lo))
    c = torch.floor((pos[idx].double() - lo[None, :]) * (M / ext)[None, :]).clamp_(0, M - 1).to(torch.int64)
    return (c[:, 0] * M + c[:, 1]) * M + c[:, 2]


def _assert_same_neighbours(got, want, pos, taxes, x0, nx, plan, what):
    """A mismatch names the first offending lattice points: indices, both float64 distances, and the cell and group of the
    cell list that holds the particle the search should have found."""
    bad = torch.nonzero(got.reshape(-1).to(torch.int64) != want).squeeze(1)
    if bad.numel() == 0:
        return
    b = bad[:6]
    q = chk.lattice_points(taxes, x0, nx, b)
    g, w = got.reshape(-1)[b].to(torch.int64), want[b]
    ok = (g >= 0) & (g < pos.shape[0])
    dg = chk._dist2(q[:, 0], q[:, 1], q[:, 2], *(pos[g.clamp(0, pos.shape[0] - 1)].double()[:, c] for c in range(3)))
    dw = chk._dist2(q[:, 0], q[:, 1], q[:, 2], *(pos[w].double()[:, c] for c in range(3)))
    cw = _cells(pos, plan, w)
    ny, nz = taxes[1].numel(), taxes[2].numel()
    first = ["point (%d, %d, %d): got particle %d%s at d2 = %.17g, want %d at d2 = %.17g in cell %d, group %d"
             % (x0 + f // (ny * nz), (f // nz) % ny, f % nz, gi, "" if o else " (no particle)", a, wi, c, ci, ci >> plan["gshift"])
             for f, gi, o, a, wi, c, ci in zip(b.tolist(), g.tolist(), ok.tolist(), dg.tolist(), w.tolist(), dw.tolist(), cw.tolist())]
    raise AssertionError("%s: %d of %d lattice points differ; %s" % (what, bad.numel(), want.numel(), "; ".join(first)))


def _check_slab(K, leg, plan, pos, payload, axes, taxes, x0, nx, k, seed):
    """One slab: the reference once, then every option set of the leg against it.  -> [(options, kind, open, uncertified)]."""
    name = "%s rows [%d, %d)" % (leg["name"], x0, x0 + nx)
    idx, best, cert = chk.nn_slab_reference(pos, taxes, x0, nx, k)
    assert int(idx.min()) >= 0
    unc = chk.nn_settle(pos, taxes, x0, nx, idx, best, cert)        # (asserts the cap before anything is compared)
    assert int(idx.max()) < pos.shape[0]
    want_out = payload[idx].t().contiguous().reshape(4, nx, len(axes[1]), len(axes[2]))
    rows = []
    for opts in leg["runs"]:
        with _options(dict(opts, nn_stats=1)):
            out, got = K.nn_resample(pos, payload, axes, x0, nx, want_index=True)
            last = K.nn_last_search()
        what = "%s %r" % (name, opts)
        _assert_same_neighbours(got, idx, pos, taxes, x0, nx, plan, what)
        assert torch.equal(out, want_out), what + ": the output is not the payload of the nearest particles"
        assert last["kind"] == chk.nn_search_kind(leg["lattice"], opts), (what, last)
        assert last["tiles"] > 0 and last["open"] >= 0 and last["radii"] == int(last["kind"] == "column"), (what, last)
        RAN.append((leg["name"], plan, last["kind"]))
        rows.append((opts, last["kind"], last["open"], unc))
        del out, got
    # the local reference itself, on the device: random points of the slab, certified or not, against brute force
    g = torch.Generator(device=pos.device)
    g.manual_seed(seed)
    pick = torch.randint(0, idx.numel(), (-(-RANDOM_POINTS // len(leg["slabs"])),), generator=g, device=pos.device)
    bi, bb = chk.nn_brute_force(pos, chk.lattice_points(taxes, x0, nx, pick))
    assert torch.equal(idx[pick], bi) and torch.equal(best[pick], bb), name + ": the slab reference differs from brute force"
    return rows


# ------------------------------------------------------------------------------------------- a ----
def test_a_coverage_guard(K):
    plans = {leg["name"]: _plan(K, leg) for leg in chk.NN_MATRIX}
    for name, p in plans.items():
        print(name, p)
    vals = list(plans.values())
    assert any(p["gshift"] == 14 and p["sorted"] for p in vals) and any(p["gshift"] == 15 and p["sorted"] for p in vals)
    assert any(64 * 1024 < p["lds_fine"] < 128 * 1024 for p in vals) and any(p["lds_fine"] > 128 * 1024 for p in vals)
    assert any(p["sorted"] and p["ngroups"] > 512 for p in vals)
    top = max((p for p in vals if p["sorted"]), key=lambda p: p["ngroups"])
    assert top["ngroups"] == 2028 and top["M"] == 405 and top["gshift"] == 15      # (2048 groups is the sort's limit)
    assert any(not p["sorted"] and p["ngroups"] > 2048 for p in vals)
    assert K.nn_plan(C3_PARTICLES) in vals
    assert {leg["dtype"] for leg in chk.NN_MATRIX} == {"float32", "float64"}
    kinds = {chk.nn_search_kind(leg["lattice"], o) for leg in chk.NN_MATRIX for o in leg["runs"]}
    assert kinds == {"ring", "scatter", "column"}


# ------------------------------------------------------------------------------------------- b ----
@pytest.mark.parametrize("leg", chk.NN_MATRIX, ids=lambda l: l["name"])
def test_b_exact_neighbours(K, leg):
    """1.05e8 particles: 1.3 GB of positions, 1.7 GB of payload, 7 GB of workspace, half a GB per temporary of the references."""
    t0 = time.time()
    plan = _plan(K, leg)
    assert {f: plan[f] for f in leg["plan"]} == leg["plan"], plan
    axes = chk.nn_matrix_axes(leg["lattice"], seed=7)
    taxes = [chk._axis(a, K.device) for a in axes]
    x0, nx = leg["slabs"][0]
    pos, nbar = chk.nn_matrix_particles(K.device, leg["n"], getattr(torch, leg["dtype"]), axes, x0, nx, seed=leg["n"] % 1009)
    k = chk.nn_search_k(nbar, chk.nn_gap_min(taxes))
    g = torch.Generator(device=K.device)
    g.manual_seed(5)
    payload = torch.rand((leg["n"], 4), generator=g, device=K.device, dtype=torch.float32)
    rows = []
    for x0, nx in leg["slabs"]:
        rows += [(x0, nx) + r for r in _check_slab(K, leg, plan, pos, payload, axes, taxes, x0, nx, k, seed=x0 + 1)]
    torch.cuda.synchronize()
    print("\n%s: k = %d, %.1f s; (x0, nx, options, search, open points, uncertified points): %s" % (leg["name"], k, time.time() - t0, rows))
    del pos, payload
    _free(K)


# ------------------------------------------------------------------------------------------- c ----
@pytest.mark.parametrize("n", [16383, 16384, 16385])
def test_c_switch_into_the_bucket_sort(K, n):
    """4 NB_CHUNK - 1, 4 NB_CHUNK, 4 NB_CHUNK + 1 particles (NB_CHUNK = 4096): the counting sort's last size and the bucket sort's
    first two, whole 32^3 lattice, every point against brute force."""
    plan = K.nn_plan(n)
    assert plan["sorted"] == int(n >= 16384) and plan["nchunks"] == -(-n // 4096), plan
    axes = chk.nn_matrix_axes(("uniform", 32))
    taxes = [chk._axis(a, K.device) for a in axes]
    pos, _ = chk.nn_matrix_particles(K.device, n, torch.float32, axes, 0, 32, seed=n)
    payload = torch.rand((n, 4), device=K.device, dtype=torch.float32)
    idx, best = chk.nn_brute_force(pos, chk.lattice_points(taxes, 0, 32, torch.arange(32 ** 3, device=K.device)), batch=4096)
    for opts in ({}, {"nn_column": 0}, {"nn_query_centric": 1}):
        with _options(opts):
            out, got = K.nn_resample(pos, payload, axes, 0, 32, want_index=True)
            last = K.nn_last_search()
        _assert_same_neighbours(got, idx, pos, taxes, 0, 32, plan, "%d particles %r" % (n, opts))
        assert torch.equal(out, payload[idx].t().contiguous().reshape(4, 32, 32, 32))
        assert last["kind"] == chk.nn_search_kind(("uniform", 32), opts), last
        RAN.append(("edge %d" % n, plan, last["kind"]))
    _free(K)


# ------------------------------------------------------------------------------------------- d ----
def test_d_legs_ran_what_the_guard_counts(K):
    """Runs last, after the WHOLE file: a partial run (-k, --lf, one leg alone) has not recorded every leg and fails here by
    design; the message says so."""
    whole = "(this check needs every leg of the file to have run in the same session: %d runs recorded)" % len(RAN)
    for leg in chk.NN_MATRIX:
        for opts in leg["runs"]:
            want = (leg["name"], _plan(K, leg), chk.nn_search_kind(leg["lattice"], opts))
            assert RAN.count(want) == len(leg["slabs"]), ("runs of", want[0], want[2], whole)
    ran = [p for _, p, _ in RAN]
    assert K.nn_plan(C3_PARTICLES) in ran, whole
    assert any(p["sorted"] and p["ngroups"] == 2028 for p in ran) and any(not p["sorted"] and p["ngroups"] > 2048 for p in ran), whole
    assert {n for n, _, _ in RAN if n.startswith("edge")} == {"edge 16383", "edge 16384", "edge 16385"}, whole
