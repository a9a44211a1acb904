"""The direct CIC / TSC deposit (vps_deposit_assign: one sort record per particle, every brick gathers from its own and its lower
neighbours' buckets) against the float64 oracle: bit exact on the half-cell lattice, per cell within the float32 bar on hard
positions, at small counts, with 64-bit keys, under the other sort variants, on guarded memory and through the public surface.
Run on an MI355X:  python -m pytest tests/test_gpu_assign_direct.py -q -m gpu"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import assign_direct_ref as adr  # noqa: E402
import guarded as gd  # noqa: E402
import small_ref as sr  # noqa: E402
from oracle import vps_oracle as orc  # noqa: E402
from test_gpu_small_kernels import _assign_positions  # noqa: E402

PSUM_RTOL = 2e-5          # the project's bar for Psum per bin against the float64 oracle (tests/test_gpu_configs.py)
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()
    LATTICE.clear()


def _direct(K, pos, f, N, L, assignment):
    """-> float32 [C, N, N, N] on the host."""
    g = K.deposit_assign(K.to_device(pos), K.to_device(np.ascontiguousarray(f), torch.float32), N, L, assignment)
    assert g.shape == (f.shape[1], N, N, N) and g.dtype == torch.float32
    return g.cpu().numpy()


# ------------------------------------------------------------------ 1. bit exact on the half-cell lattice ----
LATTICE = {}      # (assignment, N, C) -> (pos float64, f float32 [n, C], L, oracle grid float32 [C, N, N, N], plan): one reference for both dtypes


def _lattice(K, assignment, N, C):
    key = (assignment, N, C)
    if key not in LATTICE:
        plan = K.deposit_assign_plan(1, C, N, assignment)
        pos, f, L = adr.lattice_particles(N, assignment, (plan["bx"], plan["by"], plan["bz"]), C, seed=N + sr.ORDER[assignment])
        ref = orc.deposit_assign(f.astype(np.float64), pos, N, L, assignment)
        ref32 = np.ascontiguousarray(np.moveaxis(ref, -1, 0)).astype(np.float32)
        assert np.array_equal(ref32.astype(np.float64), np.moveaxis(ref, -1, 0)), "the oracle grid is exact in float32"
        LATTICE[key] = (pos, f, L, ref32, K.deposit_assign_plan(len(pos), C, N, assignment))
    return LATTICE[key]


LATTICE_N = [16, 65, 96, 128, 250]


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("N", LATTICE_N)
def test_half_cell_lattice_is_bit_exact(K, N, C, dtype, assignment):
    """Positions on multiples of Lcell / 2 (Lcell = 2^-7), integer payloads: every weight product is a multiple of 2^-9 and every
    sum exact in float32 in any order, so the grid IS the float64 oracle's -- a brick face missed or counted twice shows as a
    wrong cell.  The particles together touch every cell of the grid and aim at the first and last cell of every brick on every
    axis from every offset (tests/assign_direct_ref.py).  N = 16: axes with one and with two bricks; 96: a partial last brick;
    250: a last brick two cells wide in x and y; 65: a last brick ONE cell wide in z, narrower than TSC's reach, where brick 0
    also gathers from the brick before the last."""
    pos, f, L, ref, plan = _lattice(K, assignment, N, C)
    assert plan["two_level"] == 1 and plan["wide_keys"] == 0 and plan["record_words"] == C + 7, plan
    assert (plan["nbx"], plan["nby"], plan["nbz"]) == tuple(-(-N // plan[k]) for k in ("bx", "by", "bz"))
    if N == 16:
        assert sorted((plan["nbx"], plan["nby"], plan["nbz"])) == [1, 1, 2], plan
    if N == 250 and C == 4:
        assert N % plan["bx"] == 2 and N % plan["by"] == 2, plan
    # source buckets per axis: the brick itself with one brick, both with two, else itself and its -1 neighbour -- and the one
    # before that where the -1 neighbour of brick 0 (the last, partial brick) is narrower than the order - 1 cells reached
    def sources(axis):
        nb, last = plan["nb" + axis], N - (plan["nb" + axis] - 1) * plan["b" + axis]
        return nb if nb <= 2 else (3 if last < sr.ORDER[assignment] - 1 else 2)
    assert plan["max_sources"] == sources("x") * sources("y") * sources("z"), plan
    if N == 65:
        assert N % plan["bz"] == 1 and N % plan["bx"] == 1 and plan["max_sources"] == (18 if assignment == "tsc" else 8), plan
    else:
        assert plan["max_sources"] <= 8, plan
    got = _direct(K, pos.astype(dtype), f, N, L, assignment)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "%d cells differ, first (c, x, y, z) %r: got %r, oracle %r" % (
        len(bad), bad[:4].tolist(), got[tuple(bad[:4].T)].tolist(), ref[tuple(bad[:4].T)].tolist())


@pytest.mark.parametrize("N", [96, 250])
def test_cic_on_cell_centres_is_the_ngp_deposit(K, N):
    """A particle on a cell centre has CIC weights exactly 1 and 0: the direct CIC grid IS the NGP grid of the same particles."""
    from vpower import interp
    L, n = N * adr.LCELL, 40001
    rng = np.random.default_rng(N)
    cell = rng.integers(0, N, (n, 3))
    cell[:4] = [[0, 0, 0], [N - 1, N - 1, N - 1], [0, N - 1, 7], [N - 1, 0, 0]]
    pos = (cell + 0.5) * adr.LCELL
    f = rng.integers(-8, 9, (n, 4)).astype(np.float32)
    for p in (pos, pos.astype(np.float32)):
        assert np.array_equal(orc.cell_index(p, N, L), cell)
        cic = interp.deposit_to_grid(f, p, N, L, assignment="cic", method="direct")
        ngp = interp.deposit_to_grid(f, p, N, L)
        assert cic.shape == (N, N, N, 4) and np.array_equal(cic, ngp)
        assert np.array_equal(interp.deposit_to_grid(f, p, N, L, assignment="ngp", method="direct"), ngp)


# ------------------------------------------------------------------ 2. per-cell bar on hard positions ----
def _per_cell_check(got_at, pos, f, N, L, assignment, what):
    """got_at(cells) -> float64 [m, C]: the grid's values on flat cells.  Returns the oracle's cells with a non-zero sum."""
    f64 = f.astype(np.float64)
    ref_cells, ref = sr.deposit_assign_sparse(f64, pos, N, L, assignment)
    bar_cells, bar = sr.deposit_assign_sparse(np.abs(f64), pos, N, L, assignment)
    n_cells, n_c = adr.contribution_counts(pos, N, L, assignment)
    assert np.array_equal(ref_cells, bar_cells) and n_c.max() <= 10 ** 4, n_c.max()
    n_on = sr.sparse_on(ref_cells, n_cells, n_c[:, None].astype(np.float64))
    got = got_at(ref_cells)
    err = np.abs(got - ref)
    allowed = (16 + n_on) * EPS * bar + n_on * sr.F32_TINY
    worst = np.max(err / np.where(allowed > 0, allowed, np.inf), initial=0.0)
    print("%s: worst per-cell error / bar = %.3g, most contributions to a cell %d" % (what, worst, n_c.max()))
    assert np.all(err <= allowed), (what, worst)
    assert np.all(got[n_on[:, 0] == 0] == 0)
    return ref_cells, ref


HARD = [(250, 2.5, 4), (96, 1.0, 3), (16, 1.0, 4)]


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,L,C", HARD, ids=["250", "96", "16"])
def test_hard_positions_per_cell(K, N, L, C, dtype, assignment):
    """100 003 particles on faces, centres, their float neighbours, outside the box and 1e10 away, standard-normal payloads.
    Per cell |got - ref| <= (16 + n_c) 2^-24 bar_c + n_c F32_TINY: bar_c the oracle's deposit of |f|, 16 the roundings of one
    record (small_ref.RECORD_RTOL), n_c the non-zero contributions to the cell (their float32 sum in any order; n_c <= 10^4 is
    asserted).  Cells nobody contributes to are exactly 0, and the channel sums are the payload's."""
    n = 100003
    pos = _assign_positions(N, L, n, dtype, seed=N + C)
    f = np.random.default_rng(C).standard_normal((n, C)).astype(np.float32)
    got = _direct(K, pos, f, N, L, assignment).reshape(C, -1)
    cells, _ = _per_cell_check(lambda c: got[:, c].T.astype(np.float64), pos, f, N, L, assignment,
                               "direct %s N=%d C=%d %s" % (assignment, N, C, np.dtype(dtype).name))
    rest = np.ones(N ** 3, dtype=bool)
    rest[cells] = False
    assert not got[:, rest].any(), "cells without a contribution must be exactly 0"
    f64 = f.astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64).sum(axis=1) - f64.sum(axis=0)) <= 27 * sr.RECORD_RTOL * np.abs(f64).sum(axis=0))


# ------------------------------------------------------------------ 3. small counts ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("count", [0, 1, 255, 257])
def test_small_counts(K, count, dtype, assignment):
    """Nothing, one particle, one short of a block and one over it (the special rows come first)."""
    for (N, L), C in (((96, 1.0), 4), ((16, 1.0), 1), ((250, 2.5), 3)):
        pos = _assign_positions(N, L, count, dtype, seed=count) if count else np.zeros((0, 3), dtype=dtype)
        f = np.random.default_rng(count).standard_normal((count, C)).astype(np.float32)
        got = _direct(K, pos, f, N, L, assignment).reshape(C, -1)
        if count == 0:
            assert not got.any()
            continue
        cells, _ = _per_cell_check(lambda c: got[:, c].T.astype(np.float64), pos, f, N, L, assignment,
                                   "direct %s N=%d n=%d" % (assignment, N, count))
        assert np.count_nonzero(got.any(axis=0)) <= len(cells)
        rest = np.ones(N ** 3, dtype=bool)
        rest[cells] = False
        assert not got[:, rest].any()


# ------------------------------------------------------------------ 4. 64-bit keys ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_wide_keys_at_2048(K, assignment):
    """N = 2048, C = 1: the smallest grid whose bricks x cells reach 2^32, so the sort runs on 64-bit keys (the plan must say so).
    The 34 GB grid stays on the device: the oracle's sparse cells are gathered and held to the per-cell bar, and the number of
    non-zero cells of the WHOLE grid is the number of oracle cells with a non-zero sum."""
    N, L, C, n = 2048, 1.0, 1, 100003
    plan = K.deposit_assign_plan(n, C, N, assignment)
    assert plan["wide_keys"] == 1 and plan["nbuckets"] * plan["cells"] >= 2 ** 32 and plan["two_level"] == 1, plan
    pos = _assign_positions(N, L, n, np.float32, seed=N + C)
    f = np.random.default_rng(C).standard_normal((n, C)).astype(np.float32)
    grid = K.deposit_assign(K.to_device(pos), K.to_device(f), N, L, assignment)
    flat = grid.view(C, -1)

    def got_at(cells):
        return flat[:, torch.as_tensor(cells, device=flat.device)].T.double().cpu().numpy()

    _, ref = _per_cell_check(got_at, pos, f, N, L, assignment, "direct %s N=2048" % assignment)
    nonzero = int(torch.count_nonzero(flat))
    del grid, flat
    torch.cuda.empty_cache()
    assert nonzero == int(np.count_nonzero(ref))


# ------------------------------------------------------------------ 5. sort variants ----
@pytest.mark.parametrize("opt,value,expect", [("sort_atomic", 1, dict(two_level=0)), ("sort_staged", 0, dict(two_level=1, staged=0))],
                         ids=["atomic", "unstaged"])
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_sort_variants(K, assignment, opt, value, expect):
    from vpower import _ffi
    N, C = 96, 4
    pos, f, L, ref, plan = _lattice(K, assignment, N, C)
    assert plan["two_level"] == 1 and plan["staged"] == 1, plan
    with _ffi.option(opt, value):
        now = K.deposit_assign_plan(len(pos), C, N, assignment)
        assert {k: now[k] for k in expect} == expect, now
        got = _direct(K, pos.astype(np.float32), f, N, L, assignment)
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------ 6. guarded run ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_guarded_exact_size_workspace_and_poisoned_grid(K, assignment):
    """On guarded memory: an exact-size workspace of its own key in the three states of the guarded tests (fresh and zeroed; left
    by a call of the same shape on other data; left by a call of a larger shape), the grid poisoned between guards.  No poison
    is left (every cell was written), no guard is touched, and the grid is the oracle's in every state."""
    from vpower import _ffi
    N, C = 96, 4
    pos, f, L, ref, _ = _lattice(K, assignment, N, C)
    G = gd.guarded_kernels()
    try:
        dpos, df = G.to_device(pos.astype(np.float32)), G.to_device(f, torch.float32)
        rng = np.random.default_rng(7)
        spos = G.to_device((rng.random((len(pos), 3)) * L).astype(np.float32))
        sf = G.to_device(rng.standard_normal((len(pos), C)).astype(np.float32))
        opos = G.to_device((rng.random((3 * len(pos) + 5, 3)) * 1.0).astype(np.float32))
        of = G.to_device(rng.standard_normal((3 * len(pos) + 5, C)).astype(np.float32))
        order = sr.ORDER[assignment]
        want_bytes = _ffi.lib().vps_deposit_assign_workspace_bytes(len(pos), C, N, order)

        def checked(what):
            torch.cuda.synchronize()
            rep = G.check()
            assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
            left = [(r.name, r.shape, len(r.poison)) for r in rep if r.kind == "empty" and len(r.poison)]
            assert left == [], "%s: cells still hold the poison: %r" % (what, left)
            return rep

        for state in ("Z", "D-same", "D-other"):
            G.release()
            G.state = "Z"
            if state == "D-same":
                G.deposit_assign(spos, sf, N, L, assignment)
            elif state == "D-other":
                G.deposit_assign(opos, of, 128, 1.0, assignment)
            if state != "Z":
                checked("the call before %s" % state)
                G.state = "D"
            grid = G.deposit_assign(dpos, df, N, L, assignment)
            rep = checked("deposit_assign %s, state %s" % (assignment, state))
            ws = [r for r in rep if r.kind == "workspace"]
            assert [(r.name, r.nbytes) for r in ws] == [("deposit_assign", want_bytes)], ws
            assert np.array_equal(grid.cpu().numpy(), ref), state
    finally:
        G.state = "Z"
        G.release()
        G.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 7. through the public surface ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_public_surface(K, assignment):
    """deposit_to_grid(method="direct") at the shape and bar of test_higher_order_assignment_and_deconvolution, and
    deposit_to_field(..., method="direct").spctrm("momentum", deconvolve=True): shell counts bit equal to the oracle table of
    the direct field's own grids, Psum within the project's bar of it and within 1e-4 of the expansion route's spectrum (the two
    fields differ by float32 summation order only)."""
    from vpower import interp
    rng = np.random.default_rng(21)
    N, Np, L = 32, 60000, 2.0
    pos = (rng.random((Np, 3)) * L).astype(np.float32)
    pos[:100] = np.array([L - 1e-4, 1e-5, L / 2], dtype=np.float32)          # periodic wrap on two faces
    f = rng.standard_normal((Np, 4)).astype(np.float32)
    grid = interp.deposit_to_grid(f, pos, N, L, assignment=assignment, method="direct")
    ref = orc.deposit_assign(f.astype(np.float64), pos, N, L, assignment)
    assert grid.shape == (N, N, N, 4)
    assert np.allclose(grid, ref, rtol=0, atol=2e-5 * np.abs(ref).max())
    g1 = interp.deposit_to_grid(f[:, 0], pos.astype(np.float64), N, L, assignment=assignment, method="direct")
    assert g1.shape == (N, N, N)
    assert np.allclose(g1, orc.deposit_assign(f[:, 0].astype(np.float64), pos.astype(np.float64), N, L, assignment),
                       rtol=0, atol=2e-5 * np.abs(ref).max())
    g7 = interp.deposit_to_grid(np.concatenate((f, f[:, :3]), axis=1), pos, N, L, assignment=assignment, method="direct")
    assert g7.shape == (N, N, N, 7)       # four channels, then three
    assert np.allclose(g7[..., 4:], ref[..., :3], rtol=0, atol=2e-5 * np.abs(ref).max())
    vel = rng.standard_normal((Np, 3))
    dens = np.exp(0.3 * rng.standard_normal(Np))
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    box = gp.deposit_to_field(N, assignment=assignment, method="direct")
    assert box.assignment == assignment
    sp = box.spctrm("momentum", deconvolve=True)
    vx, vy, vz, m = box.vx, box.vy, box.vz, box.mass
    P = orc.vector_power(vx * m, vy * m, vz * m, L, N)
    r = orc.spectrum_table(P * orc.window_inv2(N, assignment), L, N, "library")
    assert np.array_equal(sp.Nsample, r[:, 3])
    assert np.allclose(sp.Psum, r[:, 2], rtol=PSUM_RTOL, atol=0)
    se = gp.deposit_to_field(N, assignment=assignment, method="expand").spctrm("momentum", deconvolve=True)
    assert np.array_equal(sp.Nsample, se.Nsample)
    assert np.allclose(sp.Psum, se.Psum, rtol=1e-4, atol=0)
    ngp = gp.deposit_to_field(N, method="direct").spctrm("momentum")
    assert np.allclose(ngp.Psum, gp.deposit_to_field(N).spctrm("momentum").Psum, rtol=1e-6, atol=0)   # "direct" with NGP is the NGP route


# ------------------------------------------------------------------ 8. refusals ----
def test_refusals_leave_the_context_usable(K):
    from vpower import _ffi
    lib = K.lib
    N, L, C, n = 32, 1.0, 4, 1000
    rng = np.random.default_rng(0)
    pos = K.to_device(rng.random((n, 3)).astype(np.float32))
    f = K.to_device(rng.standard_normal((n, C)).astype(np.float32))
    grid = K.empty((C, N, N, N), torch.float32)
    work = K.workspace("deposit_assign", lib.vps_deposit_assign_workspace_bytes(n, C, N, 3))
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ERR_ARG = -1

    def call(pos_=p(pos), f_=p(f), n_=n, C_=C, N_=N, L_=L, order_=3, grid_=p(grid), work_=p(work)):
        rc = lib.vps_deposit_assign(K.ctx, pos_, 0, f_, n_, C_, N_, L_, order_, grid_, work_)
        return rc, lib.vps_last_error(K.ctx).decode()

    K._stream()
    for kw, word in ((dict(order_=1), "order"), (dict(order_=4), "order"), (dict(C_=2), "C=2"), (dict(C_=5), "C=5"),
                     (dict(N_=0), "np/N"), (dict(n_=-1), "np/N"), (dict(L_=0.0), "Lbox"), (dict(grid_=None), "null buffer"),
                     (dict(work_=None), "null buffer"), (dict(pos_=None), "null buffer"), (dict(f_=None), "null buffer")):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "vps_deposit_assign" in msg and word in msg, (kw, rc, msg)
    assert lib.vps_deposit_assign(None, p(pos), 0, p(f), n, C, N, L, 3, p(grid), p(work)) == ERR_ARG
    out = (ctypes.c_int64 * len(_ffi.DEPOSIT_ASSIGN_PLAN_FIELDS))()
    assert lib.vps_deposit_assign_plan(K.ctx, n, C, N, 5, out) == ERR_ARG and "order" in lib.vps_last_error(K.ctx).decode()
    assert lib.vps_deposit_assign_plan(K.ctx, n, C, N, 2, None) == ERR_ARG
    with pytest.raises(KeyError):
        K.deposit_assign(pos, f, N, L, "pcs")
    with pytest.raises(_ffi.VpsError, match="C=2"):
        K.deposit_assign(pos, f[:, :2].contiguous(), N, L, "tsc")
    # np = 0 with null particle buffers is a valid call: zeros everywhere
    rc, msg = call(pos_=None, f_=None, n_=0)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not grid.any()
    # ... and the context still deposits
    rc, msg = call()
    assert rc == 0, msg
    ref = orc.deposit_assign(f.cpu().numpy().astype(np.float64), pos.cpu().numpy(), N, L, "tsc")
    assert np.allclose(grid.permute(1, 2, 3, 0).cpu().numpy(), ref, rtol=0, atol=2e-5 * np.abs(ref).max())
