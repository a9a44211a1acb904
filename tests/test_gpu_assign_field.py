"""The fused direct CIC / TSC deposit on x-slabs (vps_deposit_field with VPS_FLAG_ASSIGN: one sort record per particle keyed by
the whole grid's bricks, the quantity formed in the owner brick's epilogue, only the slab's rows written) against the float64
oracle: per slab and per quantity on the half-cell lattice, on hard positions against the direct route, on guarded memory, under
the other sort variants, at small counts, its refusals, the untouched NGP call, the public surface and the multi-rank driver.
Run on an MI355X:  python -m pytest tests/test_gpu_assign_field.py -q -m gpu"""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import assign_direct_ref as adr  # noqa: E402
import guarded as gd  # noqa: E402
import route_refs as rr  # noqa: E402
import small_ref as sr  # noqa: E402
from oracle import vps_oracle as orc  # noqa: E402
from test_gpu_guarded import FIELD_BAR, QUANTITY_IDS, _quantities  # noqa: E402
from test_gpu_assign_direct import HARD  # noqa: E402
from test_gpu_small_kernels import _assign_positions  # noqa: E402

PSUM_RTOL = 2e-5          # the project's bar for Psum per bin against the float64 reference
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts")


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()
    LATTICE.clear()


def _fused(K, t, N, L, x0, nx, name, assignment, out=None):
    """t = (pos, vel, rho) on the device -> the fields of quantity id `name` on the rows [x0, x0 + nx), float32 on the device."""
    q, flags = _quantities()[name]
    return K.deposit_field(t[0], t[1], t[2], N, L, x0, nx, q, flags, out=out, assignment=assignment)


# ------------------------------------------------------------------ 1. half-cell lattice, per-slab parity ----
LATTICE = {}      # (assignment, N) -> (pos float64, vel, rho float32, L, {quantity id: [float64 fields [N, N, N]]})


def _lattice(K, assignment, N):
    """The lattice particles of the direct route's tests with their four integer columns split into an integer density in
    [1, 8] and integer velocities in [-2, 2]: rho v is an integer of at most 16 and every cell total of [rho v, rho] exact in
    float32 in any order (the bound is asserted).  One float64 reference per (assignment, N) for every slab and dtype."""
    key = (assignment, N)
    if key not in LATTICE:
        plan = K.deposit_assign_plan(1, 4, N, assignment)
        pos, f, L = adr.lattice_particles(N, assignment, (plan["bx"], plan["by"], plan["bz"]), 4, seed=N + sr.ORDER[assignment])
        rho = np.maximum(np.abs(f[:, 3]), 1).astype(np.float32)
        vel = np.trunc(f[:, :3] / 4).astype(np.float32)
        assert rho.min() >= 1 and rho.max() <= 8 and np.abs(vel).max() <= 2
        _, n_c = adr.contribution_counts(pos, N, L, assignment)
        assert n_c.max() * 16 * 2 ** 9 < 2 ** 24, "partial sums stay exact in float32"
        vec = orc.density_velocity_vector(vel.astype(np.float64), rho.astype(np.float64))
        grid = orc.deposit_assign(vec, pos, N, L, assignment)               # [N, N, N, 4] float64, exact
        assert np.array_equal(grid.astype(np.float32).astype(np.float64), grid) and grid[..., 3].min() > 0
        refs = {name: K.to_device(np.stack(rr.reference_fields(grid, L / N, name))) for name in QUANTITY_IDS}   # float64, resident
        LATTICE[key] = (pos, vel, rho, L, refs, plan)
    return LATTICE[key]


def _splits(N, plan):
    """[(what, [(x0, nx), ...])] of the issue's table."""
    even = lambda G: [(i * (N // G), N // G) for i in range(G)]      # noqa: E731
    if N == 16:
        return [("G=%d" % G, even(G)) for G in (2, 4, 8, 16)]
    if N == 65:
        return [("uneven", [(0, 1), (1, 32), (33, 32)])]
    if N == 96:
        out = [("G=%d" % G, even(G)) for G in (3, 6)]
        bx = plan["bx"]
        if (N // 3) % bx == 0 and (N // 6) % bx == 0:      # every edge on a brick edge: add a split that is off them
            out.append(("off-brick", [(0, bx + 1), (bx + 1, N - bx - 2), (N - 1, 1)]))
        return out
    if N == 250:
        return [("G=5", even(5))]
    raise KeyError(N)


def _check_slab(got, refs, name, x0, nx, what):
    """got: float32 on the device; refs[name]: float64 [ncomp, N, N, N] on the device.  Returns got."""
    ref = refs[name][:, x0:x0 + nx]
    assert got.shape == ref.shape and got.dtype == torch.float32, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs().amax(dim=(1, 2, 3)).cpu().numpy()
    top = ref.abs().amax(dim=(1, 2, 3)).cpu().numpy()
    for c in range(len(err)):
        assert err[c] <= FIELD_BAR * top[c], "%s component %d: max error %.3g against %.3g x %.3g" % (what, c, err[c], FIELD_BAR, top[c])
    if name == "density_1":
        assert torch.equal(got[0], ref[0].float()), what + ": the density totals are exact"
    if name == "vm":
        assert torch.equal(got[3], ref[3].float()), what + ": the mass channel is exact"
    return got


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", [16, 65, 96, 250])
def test_lattice_slabs_per_quantity(K, N, dtype, assignment):
    """Every slab of every split, every quantity id: each component within FIELD_BAR of the float64 quantity of the oracle's
    CIC / TSC grid, VPS_DENSITY (alpha = 1) and the mass of VPS_VM bit equal to it, and the slabs of a split concatenated along x
    bit equal to the x0 = 0, nx = N call -- the same kernel and epilogue on exact totals, so a face missed or counted twice at a
    slab edge is a wrong cell.  N = 16: slabs down to one row (narrower than TSC's reach), the window wrapping at x0 = 0 and the
    last slab's upper targets in slab 0; 65: a one-row slab, partial bricks on every axis; 96: slab edges off the brick edges;
    250.  One slab of N - 1 rows: nx + order - 1 >= N keeps every particle."""
    pos, vel, rho, L, refs, plan = _lattice(K, assignment, N)
    t = (K.to_device(pos.astype(dtype)), K.to_device(vel), K.to_device(rho))
    whole = {name: _check_slab(_fused(K, t, N, L, 0, N, name, assignment), refs, name, 0, N, "%s N=%d whole %s" % (assignment, N, name))
             for name in QUANTITY_IDS}
    splits = _splits(N, plan)
    if N == 96:
        edges = {x0 for _, slabs in splits for x0, _ in slabs}
        assert any(x0 % plan["bx"] for x0 in edges), ("no slab edge off a brick edge", plan, splits)
    for what, slabs in splits:
        assert slabs[0][0] == 0 and sum(nx for _, nx in slabs) == N
        for name in QUANTITY_IDS:
            parts = [_check_slab(_fused(K, t, N, L, x0, nx, name, assignment), refs, name, x0, nx,
                                 "%s N=%d %s [%d,%d) %s" % (assignment, N, what, x0, x0 + nx, name)) for x0, nx in slabs]
            cat = torch.cat(parts, dim=1)
            if not torch.equal(cat, whole[name]):
                bad = torch.nonzero(cat != whole[name]).cpu().numpy()
                raise AssertionError("%s N=%d %s %s: %d cells differ from the whole-grid call, first (c, x, y, z) %r" % (
                    assignment, N, what, name, len(bad), bad[:4].tolist()))
    for x0 in (0, 1):
        for name in ("vm", "velocity"):
            g = _check_slab(_fused(K, t, N, L, x0, N - 1, name, assignment), refs, name, x0, N - 1,
                            "%s N=%d [%d,%d) %s" % (assignment, N, x0, x0 + N - 1, name))
            assert torch.equal(g, whole[name][:, x0:x0 + N - 1])


# ------------------------------------------------------------------ 2. hard positions ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,L,C", HARD, ids=["250", "96", "16"])
def test_hard_positions_against_the_direct_route(K, N, L, C, dtype, assignment):
    """100 003 particles on faces, centres, their float neighbours, outside the box and 1e10 away; standard-normal velocities and
    positive densities.  VPS_VM through the fused call on two slabs against the direct route's raw grid of the explicit
    [rho v, rho] payload + vps_field_algebra(VM), rows of the slab, per component within FIELD_BAR; cells the oracle gives no
    contribution are exactly 0."""
    from vpower import device as D
    n = 100003
    pos = _assign_positions(N, L, n, dtype, seed=N + C)
    rng = np.random.default_rng(C)
    vel = rng.standard_normal((n, 3)).astype(np.float32)
    rho = (np.abs(rng.standard_normal(n)) + 0.05).astype(np.float32)
    t = (K.to_device(pos), K.to_device(vel), K.to_device(rho))
    raw = K.deposit_assign(t[0], K.density_velocity_vector(t[1], t[2]), N, L, assignment)
    K.field_algebra(raw, D.VM, 0, L / N)
    ref = raw.double().cpu().numpy()
    cells, _ = sr.deposit_assign_sparse(rho.astype(np.float64)[:, None], pos, N, L, assignment)
    touched = np.zeros(N ** 3, dtype=bool)
    touched[cells] = True
    touched = touched.reshape(N, N, N)
    half = N // 2 + 1                                   # two slabs, the edge off the middle
    for x0, nx in ((0, half), (half, N - half)):
        got = _fused(K, t, N, L, x0, nx, "vm", assignment).double().cpu().numpy()
        assert got.shape == (4, nx, N, N)
        for c in range(4):
            r = ref[c, x0:x0 + nx]
            err, top = float(np.abs(got[c] - r).max()), float(np.abs(r).max())
            print("%s N=%d [%d,%d) component %d: max error / max |ref| = %.3g" % (assignment, N, x0, x0 + nx, c, err / top))
            assert err <= FIELD_BAR * top, (assignment, N, x0, c, err, top)
        assert not got[:, ~touched[x0:x0 + nx]].any(), "cells without a contribution must be exactly 0"


# ------------------------------------------------------------------ 3. guarded memory ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_guarded_exact_size_workspace_and_poisoned_fields(K, assignment):
    """N = 96, one interior slab and the last one: the workspace is exactly vps_deposit_assign_workspace_bytes(np, 4, N, order)
    bytes between guards (fresh; left by a call on other data), the fields exactly ncomp nx N N poisoned floats.  No guard is
    touched, no poison is left, and the fields are the reference's."""
    from vpower import _ffi
    N = 96
    pos, vel, rho, L, refs, _ = _lattice(K, assignment, N)
    want_bytes = _ffi.lib().vps_deposit_assign_workspace_bytes(len(pos), 4, N, sr.ORDER[assignment])
    G = gd.guarded_kernels()
    try:
        t = (G.to_device(pos.astype(np.float32)), G.to_device(vel), G.to_device(rho))
        rng = np.random.default_rng(7)
        other = (G.to_device((rng.random((len(pos), 3)) * L).astype(np.float32)),
                 G.to_device(rng.standard_normal((len(pos), 3)).astype(np.float32)), G.to_device((rng.random(len(pos)) + 0.1).astype(np.float32)))

        def checked(what):
            torch.cuda.synchronize()
            rep = G.check()
            assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
            left = [(r.name, r.shape, len(r.poison)) for r in rep if r.kind == "empty" and len(r.poison)]
            assert left == [], "%s: cells still hold the poison: %r" % (what, left)
            return rep

        for x0, nx in ((37, 22), (96 - 13, 13)):
            for state in ("Z", "D-same"):
                for name in ("vm", "velocity", "energy"):
                    G.release()
                    G.state = "Z"
                    if state == "D-same":
                        _fused(G, other, N, L, x0, nx, name, assignment)
                        checked("the call before")
                        G.state = "D"
                    got = _fused(G, t, N, L, x0, nx, name, assignment)
                    rep = checked("deposit_field %s %s [%d,%d) state %s" % (assignment, name, x0, x0 + nx, state))
                    ws = [r for r in rep if r.kind == "workspace"]
                    assert [(r.name, r.nbytes) for r in ws] == [("deposit_field_assign", want_bytes)], ws
                    outs = [r for r in rep if r.kind == "empty"]
                    assert [r.nbytes for r in outs] == [4 * refs[name].shape[0] * nx * N * N], outs
                    _check_slab(got, refs, name, x0, nx, "guarded %s %s" % (assignment, name))
    finally:
        G.state = "Z"
        G.release()
        G.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 4. sort variants ----
@pytest.mark.parametrize("opt,value", [("sort_atomic", 1), ("sort_staged", 0)], ids=["atomic", "unstaged"])
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_sort_variants(K, assignment, opt, value):
    from vpower import _ffi
    N = 96
    pos, vel, rho, L, refs, _ = _lattice(K, assignment, N)
    t = (K.to_device(pos.astype(np.float32)), K.to_device(vel), K.to_device(rho))
    slabs = [(0, 32), (32, 32), (64, 32)]
    base = [_fused(K, t, N, L, x0, nx, "vm", assignment).clone() for x0, nx in slabs]
    with _ffi.option(opt, value):
        for (x0, nx), b in zip(slabs, base):
            got = _check_slab(_fused(K, t, N, L, x0, nx, "vm", assignment), refs, "vm", x0, nx, "%s %s" % (opt, assignment))
            assert torch.equal(got, b)


# ------------------------------------------------------------------ 5. small counts ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("count", [0, 1, 255, 257])
def test_small_counts(K, count, assignment):
    """Nothing, one particle, one short of a block and one over it, on a slab: np = 0 gives all zeros for every quantity."""
    from vpower import device as D
    N, L, x0, nx = 96, 1.0, 40, 30
    rng = np.random.default_rng(count)
    pos = _assign_positions(N, L, count, np.float32, seed=count) if count else np.zeros((0, 3), dtype=np.float32)
    if count:
        pos[0] = [(x0 + 3.3) * L / N, 0.21, 0.77]        # the one particle lies in the slab
    vel = rng.standard_normal((count, 3)).astype(np.float32)
    rho = (np.abs(rng.standard_normal(count)) + 0.05).astype(np.float32)
    t = (K.to_device(pos), K.to_device(vel), K.to_device(rho))
    if count == 0:
        for name in QUANTITY_IDS:
            got = _fused(K, t, N, L, x0, nx, name, assignment)
            assert got.shape[1:] == (nx, N, N) and not got.any(), name
        return
    raw = K.deposit_assign(t[0], K.density_velocity_vector(t[1], t[2]), N, L, assignment)
    K.field_algebra(raw, D.VM, 0, L / N)
    ref = raw[:, x0:x0 + nx].double().cpu().numpy()
    got = _fused(K, t, N, L, x0, nx, "vm", assignment).double().cpu().numpy()
    assert got[3].any()
    for c in range(4):
        assert np.abs(got[c] - ref[c]).max() <= FIELD_BAR * np.abs(ref[c]).max(), (count, c)
    assert np.array_equal(got[3] != 0, ref[3] != 0)


# ------------------------------------------------------------------ 6. refusals ----
def test_refusals_leave_the_context_usable(K):
    from vpower import device as D
    lib = K.lib
    N, L, n = 32, 1.0, 1000
    rng = np.random.default_rng(0)
    pos = K.to_device(rng.random((n, 3)).astype(np.float32))
    vel = K.to_device(rng.standard_normal((n, 3)).astype(np.float32))
    rho = K.to_device((rng.random(n) + 0.5).astype(np.float32))
    rhov = K.density_velocity_vector(vel, rho)
    before = K.deposit_field(pos, vel, rho, N, L, 0, N, D.VELOCITY).cpu().numpy()
    out = K.empty((4, N, N, N), torch.float32)
    work = K.workspace("refusals", max(lib.vps_deposit_assign_workspace_bytes(n, 4, N, 3), lib.vps_deposit_fft_zy_workspace_bytes_shared(n, N, N),
                                       lib.vps_nn_workspace_bytes(n, 0, N ** 3)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ERR_ARG = -1
    CIC, TSC = D.FLAG_ASSIGN("cic"), D.FLAG_ASSIGN("tsc")
    assert (CIC, TSC) == (0x100, 0x200)
    K._stream()

    def refused(rc, who):
        msg = lib.vps_last_error(K.ctx).decode()
        assert rc == ERR_ARG and who in msg, (who, rc, msg)

    def field(q, flags):
        return lib.vps_deposit_field(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, int(q), flags, p(out), p(work))

    refused(field(D.VELOCITY, 0x300), "vps_deposit_field")
    refused(field(D.VELOCITY, CIC | D.FLAG_INPUT_IS_VM), "vps_deposit_field")
    refused(field(D.VELOCITY, TSC | D.FLAG_INPUT_IS_VM), "vps_deposit_field")
    K._chk(lib.vps_set_density_weight(K.ctx, 0.5))
    refused(field(D.DENSITY, CIC | D.FLAG_REFERENCE_MOMENTUM_BUG), "vps_deposit_field")          # vps_check_weighted's rules
    refused(field(D.LOG_DENSITY, TSC | (1 << 4)), "vps_deposit_field")
    refused(field(D.WEIGHTED, CIC | D.FLAG_SHARE_ENERGY), "vps_deposit_field")
    ctx2 = D.HipKernels()                                                                           # alpha never set
    try:
        ctx2._stream()
        rc = lib.vps_deposit_field(ctx2.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, D.WEIGHTED, CIC, p(out), p(work))
        assert rc == ERR_ARG and "vps_set_density_weight" in lib.vps_last_error(ctx2.ctx).decode()
    finally:
        ctx2.close()
    spec = K.empty((3, N // 2, N, N), torch.complex64)
    nyq = K.empty((3, N, N), torch.complex64)
    zimg = K.empty((4 * K.zimage_elems(N, N),), torch.complex64)
    ax = np.ascontiguousarray((np.arange(N) + 0.5) / N)
    from vpower import _ffi
    for flag in (CIC, TSC, 0x300):
        refused(lib.vps_deposit_fft_zy(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, D.VELOCITY, flag, p(spec), p(nyq), p(work)),
                "vps_deposit_fft_zy")
        refused(lib.vps_deposit_fft_z(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, D.VELOCITY, flag, p(zimg), p(work)),
                "vps_deposit_fft_zy")
        refused(lib.vps_deposit_fft_z_slab(K.ctx, p(pos), 0, p(vel), p(rho), n, n, N, L, 0, N, D.VELOCITY, flag, p(zimg), p(work)),
                "vps_deposit_fft_zy")
        refused(lib.vps_field_algebra(K.ctx, D.VELOCITY, flag, L / N, p(out), N ** 3), "vps_field_algebra")
        refused(lib.vps_field_algebra_out(K.ctx, D.VELOCITY, flag, L / N, p(out), N ** 3, p(spec)), "vps_field_algebra")
        refused(lib.vps_nn_resample_quantity(K.ctx, p(pos), 0, p(rhov), n, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N,
                                             0, N, L / N, D.VELOCITY, flag, p(out), None, p(work)), "vps_nn_resample_quantity")
    with pytest.raises(ValueError):
        D.FLAG_ASSIGN("pcs")
    with pytest.raises(ValueError):
        K.deposit_field(pos, vel, rho, N, L, 0, N, D.VELOCITY, assignment="pcs")
    # the wrapper sizes the workspace from assignment=: the bits in flags= (which would run CIC / TSC in the NGP workspace) are
    # refused before anything is allocated or enqueued
    for bits in (CIC, TSC, 0x300, CIC | D.FLAG_REFERENCE_MOMENTUM_BUG):
        for a in ("ngp", "cic", "tsc"):
            with pytest.raises(ValueError, match="assignment="):
                K.deposit_field(pos, vel, rho, N, L, 0, N, D.VELOCITY, flags=bits, assignment=a)
    with pytest.raises(ValueError, match="assignment="):
        K.deposit_field(pos, vel, rho, N, L, 0, N, D.VELOCITY, flags=CIC)
    # ... and the context still deposits: the NGP call gives what it gave, the flagged call the CIC field
    assert np.array_equal(K.deposit_field(pos, vel, rho, N, L, 0, N, D.VELOCITY).cpu().numpy(), before)
    got = K.deposit_field(pos, vel, rho, N, L, 8, 16, D.VM, assignment="cic").double().cpu().numpy()
    vec = orc.density_velocity_vector(vel.cpu().numpy().astype(np.float64), rho.cpu().numpy().astype(np.float64))
    ref = rr.reference_fields(orc.deposit_assign(vec, pos.cpu().numpy(), N, L, "cic"), L / N, "vm")
    for c in range(4):
        assert np.abs(got[c] - ref[c][8:24]).max() <= FIELD_BAR * np.abs(ref[c]).max()


# ------------------------------------------------------------------ 7. the NGP call is untouched ----
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_ngp_call_is_untouched(K, assignment):
    """deposit_field without the bits is bit equal before and after a flagged call on the same context (integer payloads: the
    float32 sums do not depend on the order of the adds), differs from the flagged field, and the two workspaces are separate
    allocations."""
    from vpower import device as D
    N, L, n, x0, nx = 64, 1.0, 50000, 16, 24
    rng = np.random.default_rng(3)
    pos = K.to_device(rng.random((n, 3)).astype(np.float32))
    vel = K.to_device(rng.integers(-2, 3, (n, 3)).astype(np.float32))       # integer rho v, Lcell^3 = 2^-18: the NGP momentum is
    rho = K.to_device(rng.integers(1, 9, n).astype(np.float32))             # exact in any order of the LDS adds, so bit equal
    first = K.deposit_field(pos, vel, rho, N, L, x0, nx, D.MOMENTUM).clone()
    flagged = K.deposit_field(pos, vel, rho, N, L, x0, nx, D.MOMENTUM, assignment=assignment)
    again = K.deposit_field(pos, vel, rho, N, L, x0, nx, D.MOMENTUM)
    assert torch.equal(first, again)
    assert not torch.equal(first, flagged)
    assert torch.equal(K.deposit_field(pos, vel, rho, N, L, x0, nx, D.MOMENTUM, assignment="ngp"), first)
    a, b = K._work["deposit"], K._work["deposit_field_assign"]
    lo, hi = sorted([(a.data_ptr(), a.numel()), (b.data_ptr(), b.numel())])
    assert lo[0] + lo[1] <= hi[0], "the two workspaces alias"
    assert b.numel() >= K.lib.vps_deposit_assign_workspace_bytes(n, 4, N, sr.ORDER[assignment])


# ------------------------------------------------------------------ 8. public surface ----
def _float64_table(fields, L, N, assignment, flavour):
    """The float64 reference table: numpy fftn of the float64 fields, windowed in float64, binned by the oracle."""
    if len(fields) == 3:
        P = orc.vector_power(fields[0], fields[1], fields[2], L, N)
    else:
        P = orc.scalar_power(fields[0], L, N)
    if assignment is not None:
        P = P * orc.window_inv2(N, assignment)
    return orc.spectrum_table(P, L, N, flavour)


@pytest.fixture(scope="module")
def surface():
    rng = np.random.default_rng(21)
    N, Np, L = 32, 60000, 2.0
    pos = (rng.random((Np, 3)) * L).astype(np.float32)
    pos[:100] = np.array([L - 1e-4, 1e-5, L / 2], dtype=np.float32)          # periodic wrap on two faces
    vel = rng.standard_normal((Np, 3)).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(Np)).astype(np.float32)
    vec = orc.density_velocity_vector(vel.astype(np.float64), dens.astype(np.float64))
    grids = {a: orc.deposit_assign(vec, pos, N, L, a) for a in ("cic", "tsc")}
    return N, Np, L, pos, vel, dens, grids


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_public_surface(K, surface, assignment):
    """deposit_to_field(N, a, method="fused") is a lazy field carrying its assignment; its spectra against method="direct" and
    against the float64 reference (numpy fftn of the reference fields of the oracle grid, window in float64, library bins):
    Nsample bit equal, Psum within PSUM_RTOL of both.  Its grids materialise through the same call with VPS_VM."""
    from vpower import interp
    N, Np, L, pos, vel, dens, grids = surface
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    fused = gp.deposit_to_field(N, assignment=assignment, method="fused")
    direct = gp.deposit_to_field(N, assignment=assignment, method="direct")
    assert fused.assignment == assignment and fused._chans is None and fused._src is not None
    for q in ("momentum", "velocity", "density"):
        sf, sd = fused.spctrm(q, deconvolve=True), direct.spctrm(q, deconvolve=True)
        assert fused._chans is None, "a spectrum must not materialise the field"
        r = _float64_table(rr.reference_fields(grids[assignment], L / N, "density_1" if q == "density" else q), L, N, assignment, "library")
        assert np.array_equal(sf.Nsample, r[:, 3]) and np.array_equal(sf.Nsample, sd.Nsample), q
        for what, ref in (("float64 reference", r[:, 2]), ("direct", sd.Psum)):
            rel = np.max(np.abs(sf.Psum - ref) / np.abs(ref))
            print("%s %s against %s: max relative Psum error %.3g" % (assignment, q, what, rel))
            assert np.allclose(sf.Psum, ref, rtol=PSUM_RTOL, atol=0), (q, what, rel)
    hf, hd = fused.helmholtz_spctrm("velocity", deconvolve=True), direct.helmholtz_spctrm("velocity", deconvolve=True)
    r = _float64_table(rr.reference_fields(grids[assignment], L / N, "velocity"), L, N, assignment, "library")
    assert np.array_equal(hf[0].Nsample, r[:, 3]) and np.allclose(hf[0].Psum, r[:, 2], rtol=PSUM_RTOL, atol=0)
    for a, b in zip(hf, hd):
        assert np.array_equal(a.Nsample, b.Nsample)
    assert np.allclose(hf[0].Psum, hd[0].Psum, rtol=PSUM_RTOL, atol=0)
    # the compressive part within the bar of ITS OWN shell sum, the solenoidal part -- a float64 difference of the two sums -- within
    # the bar of the total's (the rule of tests/test_gpu_helmholtz.py: _check)
    assert np.all(np.abs(hf[1].Psum - hd[1].Psum) <= PSUM_RTOL * np.abs(hd[1].Psum)), \
        np.max(np.abs(hf[1].Psum - hd[1].Psum) / np.abs(hd[1].Psum))
    assert np.all(np.abs(hf[2].Psum - hd[2].Psum) <= PSUM_RTOL * np.abs(hd[0].Psum))
    ref = rr.reference_fields(grids[assignment], L / N, "vm")
    for got, want in zip((fused.vx, fused.vy, fused.vz, fused.mass), ref):
        assert np.abs(got - want).max() <= FIELD_BAR * np.abs(want).max()
    assert fused._src is None and fused.assignment == assignment
    # with "ngp", "fused" is today's lazy NGP field
    n1, n2 = gp.deposit_to_field(N, method="fused"), gp.deposit_to_field(N)
    assert n1._src is not None and not hasattr(n1, "assignment")
    s1, s2 = n1.spctrm("momentum"), n2.spctrm("momentum")
    # (the same route twice: float32 summation order is all that can differ, as in test_gpu_assign_direct.py)
    assert np.allclose(s1.Psum, s2.Psum, rtol=1e-6, atol=0) and np.array_equal(s1.Nsample, s2.Nsample)
    with pytest.raises(ValueError, match="method"):
        interp.deposit_to_grid(vel[:, 0], pos, N, L, assignment=assignment, method="fused")


# ------------------------------------------------------------------ 9. the driver ----
@pytest.fixture(scope="module")
def snapshot(tmp_path_factory, K):
    """An .npz snapshot at N = 32 and the float64 reference tables of its CIC / TSC velocity spectra: the driver's own
    preprocessing (the existing kernel) on copies, float32 positions as the driver deposits them, the oracle's grid."""
    d = tmp_path_factory.mktemp("assign_field_driver")
    rng = np.random.default_rng(5)
    N, Np, L = 32, 40000, 1
    coords = (rng.random((Np, 3)) * 0.999).astype(np.float32)
    mass = (rng.random(Np) + 0.5).astype(np.float32)
    vel = rng.standard_normal((Np, 3)).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(Np)).astype(np.float32)
    path = str(d / "snap.npz")
    np.savez(path, Coordinates=coords, Masses=mass, Velocities=vel, Density=dens)
    dpos, dvel = K.to_device(coords), K.to_device(vel)
    K.preprocess(dpos, dvel, K.to_device(mass), True, True)
    vec = orc.density_velocity_vector(dvel.cpu().numpy().astype(np.float64), dens.astype(np.float64))
    refs = {}
    for a in ("cic", "tsc"):
        grid = orc.deposit_assign(vec, dpos.cpu().numpy(), N, float(L), a)
        refs[a] = _float64_table(rr.reference_fields(grid, L / N, "velocity"), float(L), N, a, "script")
    return d, path, N, L, (coords, mass, vel, dens), refs


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_driver_single_process(K, snapshot, assignment):
    sys.path.insert(0, SCRIPTS)
    try:
        import parallel_optimized as po
    finally:
        sys.path.remove(SCRIPTS)
    d, path, N, L, (coords, mass, vel, dens), refs = snapshot
    nn = po.velocity_spectrum(coords.copy(), mass, vel.copy(), N, L)
    tab = po.velocity_spectrum(coords.copy(), mass, vel.copy(), N, L, density=dens, gridding=assignment, deconvolve=True)
    r = refs[assignment]
    assert tab.dtype == np.float32 and tab.shape == nn.shape
    assert np.array_equal(tab[:, 3], nn[:, 3]) and np.array_equal(tab[:, 3], r[:, 3].astype(np.float32))
    assert np.allclose(tab[:, 2], r[:, 2], rtol=PSUM_RTOL, atol=0), np.max(np.abs(tab[:, 2] - r[:, 2]) / r[:, 2])
    with pytest.raises(Exception, match="densit"):
        po.velocity_spectrum(coords.copy(), mass, vel.copy(), N, L, gridding=assignment)
    with pytest.raises(ValueError, match="deconvolve"):
        po.velocity_spectrum(coords.copy(), mass, vel.copy(), N, L, deconvolve=True)


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


def test_driver_two_ranks(snapshot):
    """Two gloo ranks sharing the GPU run main() with --gridding cic --deconvolve -f: Pk.txt has the single-process counts and
    Psum within PSUM_RTOL of the same float64 reference.  The children run under a time limit of their own; a failing child
    ends the test, nothing is tried again."""
    import socket
    import time
    import torch.multiprocessing as mp
    d, path, N, L, _, refs = snapshot
    out = d / "out2"
    out.mkdir()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    argv = ["-i", path, "-o", str(out), "-N", str(N), "-l", str(L), "-f", "--gridding", "cic", "--deconvolve"]
    ctx = mp.spawn(_driver_rank, args=(2, port, argv), nprocs=2, join=False)
    deadline = time.monotonic() + 180
    try:
        while not ctx.join(timeout=2):
            assert time.monotonic() < deadline, "the ranks did not finish in time"
    finally:
        for pr in ctx.processes:
            if pr.is_alive():
                pr.kill()
                pr.join()
    tab = np.loadtxt(str(out / "Pk.txt"))
    r = refs["cic"]
    assert np.array_equal(tab[:, 3], r[:, 3].astype(np.float32))
    assert np.allclose(tab[:, 2], r[:, 2].astype(np.float32), rtol=PSUM_RTOL, atol=0), np.max(np.abs(tab[:, 2] - r[:, 2]) / r[:, 2])
