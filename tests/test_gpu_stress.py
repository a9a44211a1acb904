"""The tensor quantities of vps_deposit_field (VPS_SUBGRID_STRESS, VPS_DISPERSION_TENSOR: one sort, two accumulation launches
with three second-moment tile channels each, in the NGP brick kernel and in the fused CIC / TSC kernel) against the float64
reference of tests/stress_ref.py: bit equal on exact inputs, within a derived per-cell bar on hard inputs, under every sort
variant, on guarded memory, behind a busy side stream, their refusals everywhere else, and the public surface down to the
multi-rank driver.  Every case fails on a library without the codes ("vps_deposit_field: quantity 10").
Run on an MI355X:  python -m pytest tests/test_gpu_stress.py -q -m gpu"""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import assign_direct_ref as adr  # noqa: E402
import correlation_ref as cref  # noqa: E402
import guarded as gd  # noqa: E402
import second_moment_ref as smr  # noqa: E402
import stream_probe as sp  # noqa: E402
import stress_ref as st  # noqa: E402

PSUM_RTOL = 2e-5          # the project's bar for Psum per bin against the float64 reference
XI_BAR = 4 * 1.7e-7       # tests/test_gpu_correlation.py: XI_BAR
U = 2.0 ** -24            # one float32 rounding, relative
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts")
CACHE = {}
BIG = (1024, 504, 16, (40, 40))      # N, x0, nx of the thin slab with 16 KiB-per-channel bricks; the corner its particles reach
WIDE = (2048, 1020, 16, (40, 40))    # ... and of the slab whose CIC / TSC sort, keyed by the WHOLE grid's bricks, has 64-bit keys


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()
    CACHE.clear()


def _code(name):
    from vpower import device as D
    return D.QUANTITY[name]


def _dev(K, pos, vel, rho):
    return K.to_device(pos), K.to_device(vel), K.to_device(rho)


def _tensor(K, t, N, L, x0, nx, name, assignment="ngp", out=None):
    got = K.deposit_field(t[0], t[1], t[2], N, L, x0, nx, _code(name), out=out, assignment=assignment)
    assert got.shape == (6, nx, N, N) and got.dtype == torch.float32
    return got


# ------------------------------------------------------------------ exact inputs ----
def _exact_inputs(N, assignment, x0=0, nx=None, box=None, seed=0):
    """rho_p = 1, integer velocities in [-3, 3], L = N LCELL (vol a power of two), positions on the half-cell lattice.
    NGP: every cell of the rows (of the corner `box`) holds 0, 1, 2 or 4 particles at its centre.  CIC / TSC: sites four cells
    apart (shifted by 0 or -1 cell per axis, so clouds never overlap but cross brick edges and the periodic faces), each holding
    0, 1, 2 or 4 particles AT THE SAME POINT -- a cell centre or a face per axis for CIC (weights 1 | 1/2, 1/2), a face for TSC
    (weights 1/2, 1/2, 0).  A cell then receives k in {1, 2, 4} contributions of ONE weight w = 2^-m: R = k w, P_i = w sum v_i,
    S_ij = w sum v_i v_j are exact in float32 in any order, and so is the one division P_i P_j / R = w (sum v_i)(sum v_j) / k."""
    nx = N if nx is None else nx
    ny, nz = box if box is not None else (N, N)
    rng = np.random.default_rng(1000 * N + seed + {"ngp": 0, "cic": 1, "tsc": 2}[assignment])
    if assignment == "ngp":
        rows = np.arange(N) if nx == N else np.arange(x0 - 1, x0 + nx + 1)                       # (one row outside each edge of a slab)
        cx, cy, cz = np.meshgrid(rows, np.arange(ny), np.arange(nz), indexing="ij")
        cells = np.stack((cx.ravel() % N, cy.ravel(), cz.ravel()), axis=1)
        count = rng.choice(np.array([0, 1, 2, 4]), len(cells), p=[0.4, 0.3, 0.2, 0.1] if box is None else [0.7, 0.15, 0.1, 0.05])
        half = 2 * np.repeat(cells, count, axis=0) + 1
    else:
        lo = 4 if box is not None else 0                       # (the corner: no cloud may wrap out of it)
        sx = np.arange(0, N, 4) if nx == N else np.arange((x0 // 4) * 4 - 4, x0 + nx + 4, 4)
        hi_y, hi_z = (ny, nz) if box is None else (ny - 4, nz - 4)
        gx, gy, gz = np.meshgrid(sx, np.arange(lo, hi_y, 4), np.arange(lo, hi_z, 4), indexing="ij")
        sites = np.stack((gx.ravel(), gy.ravel(), gz.ravel()), axis=1) - rng.integers(0, 2, (gx.size, 3))
        on_face = np.ones_like(sites) if assignment == "tsc" else rng.integers(0, 2, sites.shape)
        half_site = 2 * sites + 1 + on_face                    # centre of cell c: 2 c + 1; the face above it: 2 c + 2
        count = rng.choice(np.array([0, 1, 2, 4]), len(sites), p=[0.1, 0.3, 0.3, 0.3])
        half = np.repeat(half_site, count, axis=0)
        half %= 2 * N
    L = N * adr.LCELL
    pos = (half * (adr.LCELL / 2)).astype(np.float32)
    vel = rng.integers(-3, 4, (len(pos), 3)).astype(np.float32)
    rho = np.ones(len(pos), dtype=np.float32)
    perm = rng.permutation(len(pos))
    return pos[perm], vel[perm], rho, L


def _exact_case(K, N, assignment, x0=0, nx=None, box=None):
    key = ("exact", N, assignment, x0, nx)
    if key not in CACHE:
        pos, vel, rho, L = _exact_inputs(N, assignment, x0, nx, box)
        m = st.moments(pos, vel, rho, N, L, assignment, x0, N if nx is None else nx, box)
        assert set(np.unique(m["n"])) <= {0, 1, 2, 4} and (m["n"] == 4).any() and (m["n"] == 1).any()
        ref = {q: st.fields(m, L / N, q) for q in st.QUANTITIES}
        for q in ref:
            r32 = ref[q].astype(np.float32)
            assert np.array_equal(r32.astype(np.float64), ref[q]), "the reference is exact in float32"
            assert r32[:3].any() and (r32[3:] < 0).any() and (r32[3:] > 0).any()
            ref[q] = r32
        CACHE[key] = (_dev(K, pos, vel, rho), L, m, ref)
    return CACHE[key]


def _assert_bits(got, ref, m, box, what):
    """got [6, nx, N, N] on the device against ref [6, nx, ny, nz] float32: bit equal in the corner, zero outside it."""
    if box is not None:
        ny, nz = box
        corner = got[:, :, :ny, :nz]
        assert int(torch.count_nonzero(got)) == int(torch.count_nonzero(corner)), what + ": a cell outside the corner is not 0"
        got = corner
    g = got.cpu().numpy()
    diff = int(np.sum(g != ref))
    assert diff == 0, "%s: %d cells differ" % (what, diff)
    assert g[:3].min() >= 0, what
    assert not g[:, m["n"] <= 1].any(), what + ": a cell with one contribution (or none) must be exactly 0"


@pytest.mark.parametrize("N,assignment", [(32, "ngp"), (32, "cic"), (32, "tsc"), (96, "ngp")])
def test_exact_inputs_are_bit_equal(K, N, assignment):
    """All six channels of both codes bit equal to the float64 reference cast to float32 on the whole grid; at N = 32 every
    slab of G = 2 and 4 ranks is bit equal to its rows.  N = 96: ragged bricks, several bricks per axis."""
    t, L, m, ref = _exact_case(K, N, assignment)
    for q in st.QUANTITIES:
        whole = _tensor(K, t, N, L, 0, N, q, assignment)
        _assert_bits(whole, ref[q], m, None, "%s %s N=%d" % (assignment, q, N))
        if N == 32:
            for G in (2, 4):
                for r in range(G):
                    x0, nx = r * (N // G), N // G
                    assert torch.equal(_tensor(K, t, N, L, x0, nx, q, assignment), whole[:, x0:x0 + nx]), (q, G, r)


@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
def test_exact_inputs_on_the_1024_slab(K, assignment):
    """N = 1024, rows [504, 520): the brick holds 4096 cells, a channel 16 KiB, the 7-channel tile 112 KiB (the kernel's dynamic
    LDS limit is raised first).  Bit equal in the corner the particles reach, zero elsewhere."""
    N, x0, nx, box = BIG
    t, L, m, ref = _exact_case(K, N, assignment, x0, nx, box)
    plan = K.deposit_plan(len(t[0]), 4, N, x0, nx) if assignment == "ngp" else K.deposit_assign_plan(len(t[0]), 4, N, assignment)
    assert 7 * plan["cells"] * 4 == 112 * 1024, plan
    for q in st.QUANTITIES:
        _assert_bits(_tensor(K, t, N, L, x0, nx, q, assignment), ref[q], m, box, "%s %s slab" % (assignment, q))


# ------------------------------------------------------------------ hard inputs ----
def _hard(N, slab=None, n=200_000):
    """The inputs of tests/test_gpu_second_moment.py::test_hard_inputs_per_cell_bar (|v|^2 = 10^6 sigma^2, lognormal rho, 30 % of
    the particles in a few cells) on a grid of 32 cells per axis; slab = (N, x0, nx, box): the same cloud laid into the corner
    of the thin slab, 16 rows deep, four cells off the faces."""
    rng = np.random.default_rng(64)
    pos = rng.random((n, 3))
    hot = n * 3 // 10
    centres = (rng.integers(0, 32, (24, 3)) + 0.5) / 32
    pos[:hot] = centres[rng.integers(0, 24, hot)] + (rng.random((hot, 3)) - 0.5) * (0.9 / 32)
    bulk = np.array([300.0, -400.0, 1200.0])
    vel = (bulk + 1.3 * rng.standard_normal((n, 3)) / np.sqrt(3.0)).astype(np.float32)
    rho = np.exp(0.5 * rng.standard_normal(n)).astype(np.float32)
    if slab is None:
        return pos, vel, rho, 1.0
    Nb, x0, nx, _ = slab
    cell = np.stack((x0 + 1 + pos[:, 0] * (nx - 2), 4 + pos[:, 1] * 31, 4 + pos[:, 2] * 31), axis=1)
    return cell / Nb, vel, rho, 1.0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
@pytest.mark.parametrize("where", ["N32", "slab1024"])
def test_hard_inputs_per_cell_bar(K, where, assignment, dtype):
    """Per cell and channel ij: |got - ref| <= (n_c + 8) 2^-24 (A_ii + A_jj) / 2, times vol (code 10) or 1 / R (code 11), with
    A_ii = sum w rho v_i^2 the absolute sums: the absolute term sum of S_ij and |P_i P_j| / R are both at most (A_ii + A_jj) / 2
    (AM-GM, Cauchy-Schwarz), and (n_c + 8) U is the project's float32 summation bar.  Diagonals are never negative, empty cells
    are 0, and the diagonal sum is within the scalar's bar (n_c + 8) 2^-24 S2 of VPS_SUBGRID_ENERGY (VPS_DISPERSION)."""
    from vpower import device as D
    slab = BIG if where == "slab1024" else None
    N, x0, nx, box = slab if slab else (32, 0, 32, None)
    pos, vel, rho, L = _hard(N, slab)
    pos = pos.astype(dtype)
    key = ("hard", where, assignment, np.dtype(dtype).name)
    if key not in CACHE:
        CACHE[key] = st.moments(pos, vel, rho, N, L, assignment, x0, nx, box)
    m = CACHE[key]
    assert m["n"].max() > 1000
    vol = (L / N) ** 3
    occupied = m["n"] > 0
    Rs = np.where(occupied, m["R"], 1.0)
    t = _dev(K, pos, vel, rho)
    cut = (lambda a: a) if box is None else (lambda a: a[..., :box[0], :box[1]])
    for q, scale, scalar in (("subgrid_stress", vol, D.SUBGRID_ENERGY), ("dispersion_tensor", 1.0 / Rs, D.DISPERSION)):
        full = _tensor(K, t, N, L, x0, nx, q, assignment).double().cpu().numpy()
        got = cut(full)
        assert np.count_nonzero(full) == np.count_nonzero(got), "cells outside the corner must be 0"
        ref = st.fields(m, L / N, q)
        bar = st.bars(m, scale)
        err = np.abs(got - ref)
        worst = float(np.max(err[:, occupied] / bar[:, occupied]))
        print("%s %s %s %s: worst error / bar = %.3f" % (where, assignment, np.dtype(dtype).name, q, worst))
        assert not got[:, ~occupied].any(), q + ": empty cells must be 0"
        assert got[:3].min() >= 0, q
        assert np.all(err <= bar), "%s: worst error / bar = %.3f in %d cells" % (q, worst, int(np.sum(err > bar)))
        sc = cut(K.deposit_field(t[0], t[1], t[2], N, L, x0, nx, scalar, assignment=assignment)[0].double().cpu().numpy())
        tr_bar = (m["n"] + 8) * U * st.trace(m["A"]) * scale
        tr_err = np.abs(st.trace(got) - sc)
        print("   diagonal sum against the scalar: worst / bar = %.3f" % float(np.max(tr_err[occupied] / tr_bar[occupied])))
        assert np.all(tr_err <= tr_bar), q
        if assignment == "ngp":
            assert not got[:, m["n"] == 1].any()


# ------------------------------------------------------------------ sort variants ----
@pytest.mark.parametrize("option", [("sort_atomic", 1), ("sort_staged", 0), ("sort_groups", 7)])
def test_sort_variants_give_the_same_cells(K, option):
    """The cells of the exact cases -- whole grids at N = 32 (every route) and 96, every route on the N = 1024 slab -- under
    the one-atomic-per-particle ranking, the unstaged scatter and another group count."""
    from vpower import _ffi
    name, value = option
    for N, assignment, slab in ((32, "ngp", None), (32, "cic", None), (32, "tsc", None), (96, "ngp", None),
                                (1024, "ngp", BIG), (1024, "cic", BIG), (1024, "tsc", BIG)):
        x0, nx, box = (slab[1], slab[2], slab[3]) if slab else (0, N, None)
        t, L, m, ref = _exact_case(K, N, assignment, x0, nx if slab else None, box)
        with _ffi.option(name, value):
            for q in st.QUANTITIES:
                _assert_bits(_tensor(K, t, N, L, x0, nx, q, assignment), ref[q], m, box, "%s=%s %s %s" % (name, value, assignment, q))


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_wide_keys_on_a_thin_slab_of_2048(K, assignment):
    """64-bit sort keys need bricks x cells >= 2^32.  The NGP sort is keyed by the slab's bricks and stays far below on a thin
    slab of any grid (plan queries); the CIC / TSC sort is keyed by the bricks of the WHOLE grid whatever the slab, so at
    N = 2048 its keys are 64-bit on a slab of 16 rows too.  There: both codes on the exact inputs, rows [1020, 1036) across a
    brick edge, bit equal in the corner the particles reach and zero elsewhere."""
    N, x0, nx, box = WIDE
    for n_ in (1024, 2048, 4096):
        assert K.deposit_plan(1000, 4, n_, 0, 16)["wide_keys"] == 0, n_
    t, L, m, ref = _exact_case(K, N, assignment, x0, nx, box)
    plan = K.deposit_assign_plan(len(t[0]), 4, N, assignment)
    assert plan["wide_keys"] == 1 and plan["nbuckets"] * plan["cells"] >= 2 ** 32, plan
    for q in st.QUANTITIES:
        got = _tensor(K, t, N, L, x0, nx, q, assignment)
        _assert_bits(got, ref[q], m, box, "%s %s wide keys" % (assignment, q))
        del got
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ guarded memory ----
@pytest.mark.parametrize("case", ["ngp32", "tsc32", "ngp1024"])
def test_guarded_exact_size_workspace_and_poisoned_fields(K, case):
    """The workspace is exactly what the 4-channel call's size function returns, between guards, in the three states of
    tests/guarded.py; the output is exactly 6 nx N N poisoned floats between 1 MiB guards.  No guard is touched, no poison is
    left, and the fields are the exact ones."""
    from vpower import _ffi
    assignment = case[:3]
    N, x0, nx, box = BIG if case == "ngp1024" else (32, 5, 13, None)
    (dpos, dvel, drho), L, m, ref = _exact_case(K, N, assignment, *((x0, nx, box) if box else ()))
    pos, vel, rho = dpos.cpu().numpy(), dvel.cpu().numpy(), drho.cpu().numpy()
    if assignment == "ngp":
        key, want = "deposit", _ffi.lib().vps_deposit_workspace_bytes(len(pos), 4, N, nx)
    else:
        key, want = "deposit_field_assign", _ffi.lib().vps_deposit_assign_workspace_bytes(len(pos), 4, N, 3)
    rng = np.random.default_rng(3)
    G = gd.guarded_kernels()
    try:
        t = _dev(G, pos, vel, rho)
        ovel = rng.integers(-3, 4, vel.shape).astype(np.float32)
        other = _dev(G, pos[rng.permutation(len(pos))], ovel, rho)
        larger = _dev(G, np.concatenate((pos, pos[::-1])), np.concatenate((ovel, vel)), np.concatenate((rho, rho)))

        def checked(what):
            torch.cuda.synchronize()
            rep = G.check()
            assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
            left = [(r.name, r.shape, len(r.poison)) for r in rep if r.kind == "empty" and len(r.poison)]
            assert left == [], "%s: cells still hold the poison: %r" % (what, left)
            return rep

        for state, before in (("Z", None), ("D-same", other), ("D-other", larger)):
            for q in st.QUANTITIES:
                G.release()
                G.state = "Z"
                if before is not None:
                    _tensor(G, before, N, L, x0, nx, q, assignment)
                    checked("the call before")
                    G.state = "D"
                got = _tensor(G, t, N, L, x0, nx, q, assignment)
                rep = checked("%s %s state %s" % (case, q, state))
                assert [(r.name, r.nbytes) for r in rep if r.kind == "workspace"] == [(key, want)], rep
                assert [r.nbytes for r in rep if r.kind == "empty"] == [4 * 6 * nx * N * N], rep
                want_rows = ref[q] if box else ref[q][:, x0:x0 + nx]
                mm = m if box else {"n": m["n"][x0:x0 + nx]}
                _assert_bits(got, want_rows, mm, box, "%s %s state %s" % (case, q, state))
    finally:
        G.state = "Z"
        G.release()
        G.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ stream contract ----
@pytest.mark.parametrize("assignment", ["ngp", "cic"])
@pytest.mark.parametrize("q", st.QUANTITIES)
def test_side_stream_behind_the_blocker(K, assignment, q):
    """deposit_field of both codes on a side stream behind the blocker of tests/stream_probe.py, the inputs swapped in on that
    stream: it returns with the blocker pending, gives the reference of the TRUE data and the bits of the null-stream call."""
    N = 32
    if "blocker" not in CACHE:
        CACHE["blocker"] = sp.Blocker(K.device)
    data = []
    for seed in (11, 12):                       # true, decoy (exact inputs: the bits do not depend on the order of the LDS adds)
        pos, vel, rho, L = _exact_inputs(N, assignment, seed=seed)
        n = min(len(pos), 20000)
        data.append((pos[:n], vel[:n], rho[:n]))
    n = min(len(data[0][0]), len(data[1][0]))
    data = [tuple(a[:n] for a in d) for d in data]
    refs = [[st.fields(st.moments(d[0], d[1], d[2], N, L, assignment), L / N, q)] for d in data]
    true, decoy = _dev(K, *data[0]), _dev(K, *data[1])
    bufs = [b.clone() for b in decoy]
    case = sp.Case("deposit_field-%s-%s" % (q, assignment), bufs, list(true),
                   lambda: [K.deposit_field(bufs[0], bufs[1], bufs[2], N, L, 0, N, _code(q), assignment=assignment)],
                   refs[0], refs[1], ["field"])
    sp.run_case(case, CACHE["blocker"])


# ------------------------------------------------------------------ refusals ----
def test_refusals_name_the_quantity_and_enqueue_nothing(K):
    from vpower import _ffi
    from vpower import device as D
    lib = K.lib
    N, L, n = 32, 1.0, 1000
    rng = np.random.default_rng(0)
    pos = K.to_device(rng.random((n, 3)).astype(np.float32))
    vel = K.to_device(rng.standard_normal((n, 3)).astype(np.float32))
    rho = K.to_device((rng.random(n) + 0.5).astype(np.float32))
    rhov = K.density_velocity_vector(vel, rho)
    chans = K.deposit_field(pos, vel, rho, N, L, 0, N, D.VM)
    chans0 = chans.clone()
    nan = float("nan")
    out = torch.full((6, N, N, N), nan, dtype=torch.float32, device=K.device)
    spec = torch.full((3, N // 2, N, N, 2), nan, dtype=torch.float32, device=K.device)
    nyq = torch.full((3, N, N, 2), nan, dtype=torch.float32, device=K.device)
    zimg = torch.full((4 * K.zimage_elems(N, N), 2), nan, dtype=torch.float32, device=K.device)
    work = K.workspace("refusals", max(lib.vps_deposit_assign_workspace_bytes(n, 4, N, 3), lib.vps_deposit_fft_zy_workspace_bytes_shared(n, N, N),
                                       lib.vps_nn_workspace_bytes(n, 0, N ** 3), lib.vps_deposit_workspace_bytes(n, 4, N, N)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ax = np.ascontiguousarray((np.arange(N) + 0.5) / N)
    names = {D.SUBGRID_STRESS: "VPS_SUBGRID_STRESS", D.DISPERSION_TENSOR: "VPS_DISPERSION_TENSOR"}
    assert sorted(names) == [10, 11]
    K._stream()

    def refused(rc, q, code=-1):
        msg = lib.vps_last_error(K.ctx).decode()
        assert rc == code and ("quantity %d" % q in msg or names[q] in msg), (q, rc, msg)
        torch.cuda.synchronize()
        for buf in (out, spec, nyq, zimg):
            assert bool(torch.isnan(buf).all()), "a refused call wrote something"
        assert torch.equal(chans, chans0)

    for q in names:
        assert lib.vps_deposit_fft_zy_supported(K.ctx, N, q) == 0 and lib.vps_deposit_fft_zy_supported(K.ctx, 64, q) == 0
        refused(lib.vps_field_algebra(K.ctx, q, 0, L / N, p(chans), N ** 3), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, 0, L / N, p(chans), N ** 3, p(out)), q)
        refused(lib.vps_nn_resample_quantity(K.ctx, p(pos), 0, p(rhov), n, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N,
                                             0, N, L / N, q, 0, p(out), None, p(work)), q)
        refused(lib.vps_deposit_fft_zy(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(spec), p(nyq), p(work)), q)
        refused(lib.vps_deposit_fft_z(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        refused(lib.vps_deposit_fft_z_slab(K.ctx, p(pos), 0, p(vel), p(rho), n, n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        for flags in (D.FLAG_REFERENCE_MOMENTUM_BUG, D.FLAG_INPUT_IS_VM, D.FLAG_ASSIGN("cic") | D.FLAG_REFERENCE_MOMENTUM_BUG,
                      D.FLAG_ASSIGN("tsc") | D.FLAG_INPUT_IS_VM, 0x10, 0x70, D.FLAG_ASSIGN("cic") | 0x20):
            refused(lib.vps_deposit_field(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, flags, p(out), p(work)), q)
        # the value 0x300 ("pcs") stays refused, whatever the quantity
        rc = lib.vps_deposit_field(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0x300, p(out), p(work))
        assert rc == -1 and "VPS_FLAG_ASSIGN" in lib.vps_last_error(K.ctx).decode()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
    with pytest.raises(ValueError):
        D.FLAG_ASSIGN("pcs")
    with pytest.raises(ValueError, match="density_weight"):
        D.resolve_quantity("subgrid_stress", 0.5)
    # ... and the context still deposits
    got = K.deposit_field(pos, vel, rho, N, L, 0, N, D.SUBGRID_STRESS).double().cpu().numpy()
    m = st.moments(pos.cpu().numpy(), vel.cpu().numpy(), rho.cpu().numpy(), N, L)
    assert np.all(np.abs(got - st.fields(m, L / N, "subgrid_stress")) <= st.bars(m, (L / N) ** 3))


def test_python_refusals_by_name(K):
    from vpower import interp
    rng = np.random.default_rng(2)
    n, L = 5000, 1.0
    pos, vel = rng.random((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    gp = interp.GasParticles(pos, dens * (L / 16) ** 3, dens, vel, L)
    for box in (gp.ann_interp_to_field(16), gp.deposit_to_field(16, assignment="cic", method="direct")):
        for q in st.QUANTITIES:
            with pytest.raises(Exception, match=q):
                box.spctrm(q)
            with pytest.raises(Exception, match=q):
                getattr(box, q)()
    box = gp.deposit_to_field(16)
    for q in st.QUANTITIES:
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            box.helmholtz_spctrm(q)
        with pytest.raises(ValueError, match="density_weight"):
            box.spctrm(q, density_weight=0.5)


# ------------------------------------------------------------------ public surface ----
@pytest.fixture(scope="module")
def surface():
    rng = np.random.default_rng(21)
    N, n, L = 32, 40_000, 2.0
    pos = (rng.random((n, 3)) * L).astype(np.float32)
    pos[:100] = np.array([L - 1e-4, 1e-5, L / 2], dtype=np.float32)          # periodic wrap on two faces
    vel = (rng.standard_normal((n, 3)) + np.sin(2 * np.pi * pos[:, ::-1] / L)).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    return N, L, pos, vel, dens


def _box(surface, route):
    from vpower import interp
    N, L, pos, vel, dens = surface
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    return gp.deposit_to_field(N) if route == "ngp" else gp.deposit_to_field(N, assignment=route, method="fused")


@pytest.mark.parametrize("route", ["ngp", "cic", "tsc"])
def test_spectra_and_real_space_grids(K, surface, route):
    """spctrm of both names (ngp; cic with deconvolve=True; tsc): Nsample exact, Psum within 2e-5 of the float64 contraction
    sum_ij |T_ij|^2 (diagonals once, off-diagonals twice); subgrid_stress() / dispersion_tensor() are the kernel's output."""
    N, L, pos, vel, dens = surface
    box = _box(surface, route)
    m = st.moments(pos, vel, dens, N, L, route)
    window = route if route == "cic" else None
    t = _dev(K, pos, vel, dens)
    for q in st.QUANTITIES:
        s = box.spctrm(q, deconvolve=window is not None)
        assert box._chans is None and box._src is not None, "a spectrum must not materialise the field"
        r = st.table(st.fields(m, L / N, q), L, N, window=window)
        rel = float(np.max(np.abs(s.Psum - r[:, 2]) / np.abs(r[:, 2])))
        print("%s %s: max relative Psum error %.3g" % (route, q, rel))
        assert np.array_equal(s.Nsample, r[:, 3]), q
        assert np.allclose(s.Psum, r[:, 2], rtol=PSUM_RTOL, atol=0), (q, rel)
        g = getattr(box, q)()
        assert g.shape == (6, N, N, N) and g.dtype == np.float32
        # (two runs add a cell's floats in LDS in different orders: each is within the per-cell bar of the reference, so they
        #  are within two bars of each other; empty cells and single NGP contributions are 0 in both)
        direct = _tensor(K, t, N, L, 0, N, q, route).double().cpu().numpy()
        bar = st.bars(m, (L / N) ** 3 if q == "subgrid_stress" else 1.0 / np.where(m["R"] != 0, m["R"], 1.0))
        assert np.all(np.abs(g - direct) <= 2 * bar), q
        assert np.all(np.abs(g - st.fields(m, L / N, q)) <= bar), q


def test_correlation_of_the_contraction(K, surface, monkeypatch):
    """correlation('subgrid_stress') on the NGP field: against the float64 reference fed the six float32 fields the pipeline was
    handed (the bars of tests/test_gpu_correlation.py), and those six are the kernel's fields with the off-diagonals times the
    float32 sqrt(2); the structure function follows."""
    from vpower import device as D
    N, L, pos, vel, dens = surface
    seen = []
    inner = D.CorrelationPipeline.correlation

    def recording(self, fields, subtract_mean=True):
        seen.append([f.cpu().numpy() for f in fields])
        return inner(self, fields, subtract_mean=subtract_mean)
    monkeypatch.setattr(D.CorrelationPipeline, "correlation", recording)
    box = _box(surface, "ngp")
    cf = box.correlation("subgrid_stress")
    assert len(seen[-1]) == 6
    # (another deposit adds a cell's floats in another order: both are within the per-cell bar of the reference)
    m = st.moments(pos, vel, dens, N, L)
    ref, bar = st.fields(m, L / N, "subgrid_stress"), st.bars(m, (L / N) ** 3)
    for c in range(6):
        f = np.sqrt(2.0) if c >= 3 else 1.0
        assert np.all(np.abs(seen[-1][c] - f * ref[c]) <= f * (bar[c] + 2 * U * np.abs(ref[c]))), c
    xr, cnt, xi0 = cref.correlation(seen[-1], box.Lbox)
    assert np.array_equal(cf.Nsample, cnt) and len(cf) == N // 2
    e = max(float(np.max(np.abs(cf.xi - xr))), abs(cf.xi0 - xi0)) / xi0
    s2 = box.structure_function("subgrid_stress")
    e2 = float(np.max(np.abs(s2[:, 1] - 2 * (xi0 - xr)))) / (2 * xi0)
    print("correlation of the contraction: worst |xi - xi_ref| / xi(0) = %.3g, S2: %.3g" % (e, e2))
    assert max(e, e2) <= XI_BAR


@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    d = tmp_path_factory.mktemp("stress_driver")
    rng = np.random.default_rng(5)
    N, n, L = 32, 40000, 1
    path = str(d / "snap.npz")
    np.savez(path, Coordinates=(rng.random((n, 3)) * 0.999).astype(np.float32), Masses=(rng.random(n) + 0.5).astype(np.float32),
             Velocities=rng.standard_normal((n, 3)).astype(np.float32), Density=np.exp(0.3 * rng.standard_normal(n)).astype(np.float32))
    return d, path, N, L


def _driver_rank(rank, world, port, argv):
    for p in (ROOT, os.path.join(ROOT, "large-velocity-power-spectrum_amd"), SCRIPTS):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import parallel_optimized as po
        assert po.main(argv) == 0
    finally:
        dist.destroy_process_group()


def test_driver_one_and_two_ranks(K, snapshot):
    """parallel_optimized.py --quantity subgrid_stress --gridding cic at N = 32: the in-process run (one rank) against the
    float64 contraction of the driver's own preprocessing, and two gloo ranks sharing the GPU against the one-rank table --
    counts exact, sums to 2e-5.  The children run under a time limit of their own; nothing is tried again."""
    import socket
    import time
    import torch.multiprocessing as mp
    sys.path.insert(0, SCRIPTS)
    try:
        import parallel_optimized as po
    finally:
        sys.path.remove(SCRIPTS)
    d, path, N, L = snapshot
    out1, out2 = d / "out1", d / "out2"
    out1.mkdir()
    out2.mkdir()
    common = ["-i", path, "-N", str(N), "-l", str(L), "-f", "--quantity", "subgrid_stress", "--gridding", "cic"]
    assert po.main(common + ["-o", str(out1)]) == 0
    one = np.loadtxt(str(out1 / "Pk.txt"))
    z = np.load(path)
    dpos, dvel = K.to_device(z["Coordinates"]), K.to_device(z["Velocities"])
    K.preprocess(dpos, dvel, K.to_device(z["Masses"]), True, True)
    m = st.moments(dpos.cpu().numpy(), dvel.cpu().numpy(), z["Density"], N, float(L), "cic")
    r = st.table(st.fields(m, L / N, "subgrid_stress"), float(L), N, flavour="script")
    assert np.array_equal(one[:, 3], r[:, 3].astype(np.float32))
    assert np.allclose(one[:, 2], r[:, 2].astype(np.float32), rtol=PSUM_RTOL, atol=0), np.max(np.abs(one[:, 2] - r[:, 2]) / r[:, 2])
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.spawn(_driver_rank, args=(2, port, common + ["-o", str(out2)]), nprocs=2, join=False)
    deadline = time.monotonic() + 180
    try:
        while not ctx.join(timeout=2):
            assert time.monotonic() < deadline, "the ranks did not finish in time"
    finally:
        for pr in ctx.processes:
            if pr.is_alive():
                pr.kill()
                pr.join()
    two = np.loadtxt(str(out2 / "Pk.txt"))
    assert np.array_equal(two[:, 3], one[:, 3])
    assert np.allclose(two[:, 2], one[:, 2], rtol=PSUM_RTOL, atol=0), np.max(np.abs(two[:, 2] - one[:, 2]) / one[:, 2])
