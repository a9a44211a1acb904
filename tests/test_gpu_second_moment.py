"""The second-moment quantities of vps_deposit_field (VPS_TOTAL_ENERGY, VPS_SUBGRID_ENERGY, VPS_DISPERSION: a fifth LDS tile
channel S2 = sum w rho_p |v_p|^2 in the NGP brick kernel and in the fused CIC / TSC kernel) against the float64 reference of
tests/second_moment_ref.py: bit equal on integer payloads, within a derived per-cell bar on hard inputs, on guarded memory, behind
a busy side stream, their refusals everywhere else, and the public surface down to the multi-rank driver.
Run on an MI355X:  python -m pytest tests/test_gpu_second_moment.py -q -m gpu"""
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import assign_direct_ref as adr  # noqa: E402
import guarded as gd  # noqa: E402
import second_moment_ref as smr  # noqa: E402
import small_ref as sr  # noqa: E402
import stream_probe as sp  # noqa: E402
from oracle import vps_oracle as orc  # noqa: E402

PSUM_RTOL = 2e-5          # the project's bar for Psum per bin against the float64 reference
U = 2.0 ** -24            # one float32 rounding, relative
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts")
CACHE = {}


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()
    CACHE.clear()


def _codes():
    from vpower import device as D
    return {"total_energy": D.TOTAL_ENERGY, "subgrid_energy": D.SUBGRID_ENERGY, "dispersion": D.DISPERSION, "energy": D.ENERGY}


def _field(K, t, N, L, x0, nx, name, assignment="ngp", out=None):
    """t = (pos, vel, rho) on the device -> [nx, N, N] float32 on the device."""
    got = K.deposit_field(t[0], t[1], t[2], N, L, x0, nx, _codes()[name], out=out, assignment=assignment)
    assert got.shape == (1, nx, N, N) and got.dtype == torch.float32
    return got[0]


def _dev(K, pos, vel, rho):
    return K.to_device(pos), K.to_device(vel), K.to_device(rho)


def _integer_payload(rng, n):
    """v integers in [-4, 4], rho in {1, 2, 4}: rho v is an integer, (px^2 + py^2 + pz^2) / rho = rho |v|^2 <= 192 exactly."""
    return rng.integers(-4, 5, (n, 3)).astype(np.float32), rng.choice(np.array([1, 2, 4], dtype=np.float32), n)


def _exact_total(m, vol):
    """float32 field vol S2 of exact moments; asserts that no float32 addition of the kernel can round."""
    S2 = m["S2"]
    assert S2.max() < 2 ** 24 and np.array_equal(S2.astype(np.float32).astype(np.float64), S2), "every partial sum stays exact in float32"
    tot = (vol * S2).astype(np.float32)
    assert np.array_equal(tot.astype(np.float64), vol * S2)
    return tot


# ------------------------------------------------------------------ a. exact, NGP ----
def _ngp_exact(K, N):
    key = ("ngp", N)
    if key not in CACHE:
        rng = np.random.default_rng(100 + N)
        n, L = 200_000, N * 2.0 ** -3
        pos = (rng.random((n, 3)) * L).astype(np.float32)
        vel, rho = _integer_payload(rng, n)
        m = smr.moments(pos, vel, rho, N, L)
        vol = (L / N) ** 3
        assert vol == 2.0 ** -9
        psum = float(np.sum(rho.astype(np.float64) * (vel.astype(np.float64) ** 2).sum(axis=1)))
        CACHE[key] = (_dev(K, pos, vel, rho), L, vol, m, _exact_total(m, vol), psum)
    return CACHE[key]


def _ngp_slabs(N):
    return [(0, 16), (16, 16), (5, 7)] if N == 32 else [(0, N // 2), (N // 2, N - N // 2), (5, 7)]


@pytest.mark.parametrize("N", [32, 65, 96])
def test_ngp_total_energy_is_bit_exact(K, N):
    """2 10^5 particles, integer v in [-4, 4], rho in {1, 2, 4}, L = N / 8 (vol = 2^-9): VPS_TOTAL_ENERGY is bit equal to the
    float64 reference on the whole grid, every slab is bit equal to its rows, and the sum over the cells is vol sum_p rho |v|^2
    exactly.  N = 65: partial last bricks, the non-vec4 stream-out; N = 96: several bricks per axis."""
    t, L, vol, m, tot, psum = _ngp_exact(K, N)
    whole = _field(K, t, N, L, 0, N, "total_energy")
    assert np.array_equal(whole.cpu().numpy(), tot), "whole grid: %d cells differ" % int(np.sum(whole.cpu().numpy() != tot))
    assert float(whole.double().sum()) == vol * psum
    for x0, nx in _ngp_slabs(N):
        got = _field(K, t, N, L, x0, nx, "total_energy")
        assert torch.equal(got, whole[x0:x0 + nx]), (N, x0, nx)


@pytest.mark.parametrize("N", [32, 65, 96])
def test_ngp_energy_plus_subgrid_is_total(K, N):
    """On the same exact inputs VPS_ENERGY + VPS_SUBGRID_ENERGY is within 2 ulp (float32, of VPS_TOTAL_ENERGY) of
    VPS_TOTAL_ENERGY in every cell, the sub-grid part is never negative and it is exactly 0 in cells with one particle.
    Holds because the sub-grid epilogue subtracts the resolved energy as VPS_ENERGY itself forms it (hardware reciprocal, about
    nine roundings, up to 3 ulp of its own): measured worst 0.5 ulp at N = 32, 2.0 ulp at N = 65 and 96.  (Formed as
    vol (S2 - |P|^2 / R) with a division of its own, the sum missed the total by 3 / 4 / 4 ulp.)"""
    t, L, vol, m, tot, _ = _ngp_exact(K, N)
    en = _field(K, t, N, L, 0, N, "energy").double().cpu().numpy()
    sub = _field(K, t, N, L, 0, N, "subgrid_energy").double().cpu().numpy()
    assert sub.min() >= 0 and not sub[m["n"] <= 1].any()
    ulp = np.spacing(tot).astype(np.float64)
    live = tot > 0
    miss = np.abs(en + sub - tot)[live] / ulp[live]
    print("N=%d: energy + subgrid against total, worst %.2f ulp, %d of %d cells beyond 2 ulp" % (N, miss.max(), int((miss > 2).sum()), miss.size))
    assert not en[~live].any() and not sub[~live].any()
    assert miss.max() <= 2.0, (N, miss.max(), int((miss > 2).sum()))


# ------------------------------------------------------------------ b. exact, CIC / TSC ----
def _lattice(K, assignment, N=32):
    """The half-cell lattice of the direct route's tests (dyadic weights) with the integer payloads of (a)."""
    key = ("lattice", assignment, N)
    if key not in CACHE:
        plan = K.deposit_assign_plan(1, 4, N, assignment)
        pos, f, L = adr.lattice_particles(N, assignment, (plan["bx"], plan["by"], plan["bz"]), 4, seed=7 * N + sr.ORDER[assignment])
        vel = np.trunc(f[:, :3] / 2).astype(np.float32)
        rho = np.array([1, 2, 4], dtype=np.float32)[np.abs(f[:, 3]).astype(np.int64) % 3]
        assert np.abs(vel).max() <= 4
        _, n_c = adr.contribution_counts(pos, N, L, assignment)
        assert n_c.max() * 192 * 2 ** 9 < 2 ** 24, "partial sums of S2 stay exact in float32"
        vol = (L / N) ** 3
        assert vol == 2.0 ** -21
        m = smr.moments(pos, vel, rho, N, L, assignment)
        psum = float(np.sum(rho.astype(np.float64) * (vel.astype(np.float64) ** 2).sum(axis=1)))
        CACHE[key] = (pos, vel, rho, L, vol, m, _exact_total(m, vol), psum)
    return CACHE[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_assign_total_energy_is_bit_exact(K, assignment, dtype):
    """N = 32 on the half-cell lattice: VPS_TOTAL_ENERGY bit equal to the reference on the whole grid and on every slab of eight
    rows; the weights of a particle sum to 1, so the sum over the cells is vol sum_p rho |v|^2 exactly."""
    N = 32
    pos, vel, rho, L, vol, m, tot, psum = _lattice(K, assignment, N)
    t = _dev(K, pos.astype(dtype), vel, rho)
    whole = _field(K, t, N, L, 0, N, "total_energy", assignment)
    assert np.array_equal(whole.cpu().numpy(), tot), "%d cells differ" % int(np.sum(whole.cpu().numpy() != tot))
    assert float(whole.double().sum()) == vol * psum
    for x0 in range(0, N, 8):
        assert torch.equal(_field(K, t, N, L, x0, 8, "total_energy", assignment), whole[x0:x0 + 8]), (assignment, x0)
    sub = _field(K, t, N, L, 0, N, "subgrid_energy", assignment)
    disp = _field(K, t, N, L, 0, N, "dispersion", assignment)
    assert float(sub.min()) >= 0 and float(disp.min()) >= 0


@pytest.mark.parametrize("assignment", ["ngp", "cic"])
def test_tile_of_80_kib_at_1024(K, assignment):
    """N = 1024 is where the brick holds 4096 cells: the 5-channel tile is 80 KiB and the kernel's dynamic LDS limit is raised
    first.  One slab of eight rows, integer payloads on the half-cell lattice: bit equal to the reference of the slab."""
    N, x0, nx, n = 1024, 509, 8, 200_000
    plan = K.deposit_plan(n, 4, N, x0, nx) if assignment == "ngp" else K.deposit_assign_plan(n, 4, N, assignment)
    cells = plan["cells"]
    assert 5 * cells * 4 > 64 * 1024, plan
    rng = np.random.default_rng(1024)
    L = N * adr.LCELL
    h = rng.integers(0, 2 * N, (n, 3))
    h[:, 0] = rng.integers(2 * (x0 - 2), 2 * (x0 + nx + 2), n)          # around the slab, both sides of its edges
    if assignment == "ngp":
        h = h | 1                                                        # cell centres: never on a face
    pos = (h * (adr.LCELL / 2)).astype(np.float32)
    vel, rho = _integer_payload(rng, n)
    m = smr.moments(pos, vel, rho, N, L, assignment, x0, nx)
    vol = (L / N) ** 3
    tot = _exact_total(m, vol)
    assert m["n"].max() > 1 and tot.any()
    got = _field(K, _dev(K, pos, vel, rho), N, L, x0, nx, "total_energy", assignment).cpu().numpy()
    assert np.array_equal(got, tot), "%d cells differ" % int(np.sum(got != tot))
    sub = _field(K, _dev(K, pos, vel, rho), N, L, x0, nx, "subgrid_energy", assignment).double().cpu().numpy()
    ref = smr.quantity(m, L / N, "subgrid_energy")
    assert sub.min() >= 0 and np.all(np.abs(sub - ref) <= (m["n"] + 8) * U * vol * m["S2"])


# ------------------------------------------------------------------ c. hard inputs ----
def _hard(N=64, n=200_000):
    """v = bulk + delta with |bulk| = 10^3 |delta|, lognormal rho, 30 % of the particles in a few cells (more than 10^3
    contributions each), the rest uniform: most occupied cells hold one or two particles."""
    if "hard" not in CACHE:
        rng = np.random.default_rng(64)
        L = 1.0
        pos = rng.random((n, 3))
        hot = n * 3 // 10
        centres = (rng.integers(0, N, (24, 3)) + 0.5) / N
        pos[:hot] = centres[rng.integers(0, 24, hot)] + (rng.random((hot, 3)) - 0.5) * (0.9 / N)
        bulk = np.array([300.0, -400.0, 1200.0])                       # |bulk| = 1300
        vel = (bulk + 1.3 * rng.standard_normal((n, 3)) / np.sqrt(3.0)).astype(np.float32)
        rho = np.exp(0.5 * rng.standard_normal(n)).astype(np.float32)
        CACHE["hard"] = (pos, vel, rho, L)
    return CACHE["hard"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
def test_hard_inputs_per_cell_bar(K, assignment, dtype):
    """Per cell |S2_got - S2_ref| <= (n_cell + 8) 2^-24 sum |terms| (one float32 rounding per LDS add plus the roundings of one
    term: the product rho v, three squares, two adds, the division, the weight product and the product with it), n_cell the
    contributions the reference counts; VPS_SUBGRID_ENERGY and VPS_DISPERSION get the same absolute bar times vol and 1 / R --
    the bar is on the second moment, the subtraction cancels by construction (|v|^2 is 10^6 sigma^2 here).  Never negative;
    empty cells are 0; NGP cells with one particle are exactly 0, and at least 5 % of the occupied cells are such cells."""
    N = 64
    pos, vel, rho, L = _hard(N)
    pos = pos.astype(dtype)
    key = ("hard_ref", assignment, np.dtype(dtype).name)
    if key not in CACHE:
        CACHE[key] = smr.moments(pos, vel, rho, N, L, assignment)
    m = CACHE[key]
    vol = (L / N) ** 3
    ncell, S2, R = m["n"], m["S2"], m["R"]
    occupied = ncell > 0
    assert ncell.max() > 1000, ncell.max()
    if assignment == "ngp":
        single = float(np.sum(ncell == 1)) / float(np.sum(occupied))
        assert single >= 0.05, single
    t = _dev(K, pos, vel, rho)
    got = {q: _field(K, t, N, L, 0, N, q, assignment).double().cpu().numpy() for q in smr.QUANTITIES}
    bar = (ncell + 8) * U * S2                                # every term is positive: S2 is the sum of the absolute terms
    Rs = np.where(occupied, R, 1.0)
    for q, scale in (("total_energy", vol), ("subgrid_energy", vol), ("dispersion", 1.0 / Rs)):
        ref = smr.quantity(m, L / N, q)
        err = np.abs(got[q] - ref)
        worst = float(np.max(err[occupied] / (bar * scale)[occupied]))
        print("%s %s %s: worst error / bar = %.3f" % (assignment, np.dtype(dtype).name, q, worst))
        assert not got[q][~occupied].any(), q + ": empty cells must be 0"
        assert got[q].min() >= 0, q
        assert np.all(err <= bar * scale), "%s: worst error / bar = %.3f in %d cells" % (q, worst, int(np.sum(err > bar * scale)))
    if assignment == "ngp":
        assert not got["subgrid_energy"][ncell == 1].any() and not got["dispersion"][ncell == 1].any()


# ------------------------------------------------------------------ d. nothing to deposit ----
@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
def test_no_particles_writes_zeros_over_the_poison(K, assignment):
    N, L, x0, nx = 32, 1.0, 3, 9
    t = (K.to_device(np.zeros((0, 3), dtype=np.float32)), K.to_device(np.zeros((0, 3), dtype=np.float32)),
         K.to_device(np.zeros(0, dtype=np.float32)))
    for q in smr.QUANTITIES:
        out = torch.full((1, nx, N, N), float("nan"), dtype=torch.float32, device=K.device)
        got = _field(K, t, N, L, x0, nx, q, assignment, out=out)
        assert got.data_ptr() == out.data_ptr() and not bool(torch.isnan(out).any()) and not bool(out.any()), (assignment, q)


# ------------------------------------------------------------------ e. guarded memory ----
@pytest.mark.parametrize("assignment", ["ngp", "tsc"])
def test_guarded_exact_size_workspace_and_poisoned_fields(K, assignment):
    """The workspace is exactly what the 4-channel call's size function returns, between guards, in the three states of
    tests/guarded.py (fresh; left by the same shape on other data; left by a larger call); the field is exactly nx N N poisoned
    floats.  No guard is touched, no poison is left, and the field is the exact one."""
    from vpower import _ffi
    if assignment == "ngp":
        N = 65
        (dpos, dvel, drho), L, vol, m, tot, _ = _ngp_exact(K, N)
        pos, vel, rho = dpos.cpu().numpy(), dvel.cpu().numpy(), drho.cpu().numpy()
        x0, nx, key = 5, 41, "deposit"
        want = _ffi.lib().vps_deposit_workspace_bytes(len(pos), 4, N, nx)
    else:
        N = 32
        pos, vel, rho, L, vol, m, tot, _ = _lattice(K, assignment, N)
        pos = pos.astype(np.float32)
        x0, nx, key = 11, 13, "deposit_field_assign"
        want = _ffi.lib().vps_deposit_assign_workspace_bytes(len(pos), 4, N, 3)
    rng = np.random.default_rng(3)
    G = gd.guarded_kernels()
    try:
        t = _dev(G, pos, vel, rho)
        ovel, orho = _integer_payload(rng, len(pos))
        other = _dev(G, pos[rng.permutation(len(pos))], ovel, orho)
        larger = _dev(G, np.concatenate((pos, pos[::-1])), np.concatenate((ovel, vel)), np.concatenate((orho, rho)))

        def checked(what):
            torch.cuda.synchronize()
            rep = G.check()
            assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
            left = [(r.name, r.shape, len(r.poison)) for r in rep if r.kind == "empty" and len(r.poison)]
            assert left == [], "%s: cells still hold the poison: %r" % (what, left)
            return rep

        for state, before in (("Z", None), ("D-same", other), ("D-other", larger)):
            for q in ("total_energy", "subgrid_energy"):
                G.release()
                G.state = "Z"
                if before is not None:
                    _field(G, before, N, L, x0, nx, q, assignment)
                    checked("the call before")
                    G.state = "D"
                got = _field(G, t, N, L, x0, nx, q, assignment)
                rep = checked("%s %s state %s" % (assignment, q, state))
                assert [(r.name, r.nbytes) for r in rep if r.kind == "workspace"] == [(key, want)], rep
                assert [r.nbytes for r in rep if r.kind == "empty"] == [4 * nx * N * N], rep
                if q == "total_energy":
                    assert np.array_equal(got.cpu().numpy(), tot[x0:x0 + nx]), (assignment, state)
                else:
                    assert float(got.min()) >= 0
    finally:
        G.state = "Z"
        G.release()
        G.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ f. stream contract ----
@pytest.mark.parametrize("assignment", ["ngp", "cic"])
def test_side_stream_behind_the_blocker(K, assignment):
    """deposit_field(SUBGRID_ENERGY) on a side stream behind the blocker of tests/stream_probe.py, the inputs swapped in on that
    stream: it returns with the blocker pending, gives the reference of the TRUE data and the bits of the null-stream call."""
    from vpower import device as D
    N, n, L = 64, 100_000, 1.0
    if "blocker" not in CACHE:
        CACHE["blocker"] = sp.Blocker(K.device)
    data = []
    for seed in (11, 12):                       # true, decoy
        # (half-cell lattice and integer payloads: every cell total is exact, so the side-stream and null-stream calls agree to
        #  the bit whatever order the LDS adds come in)
        rng = np.random.default_rng(seed)
        pos = (rng.integers(0, 2 * N, (n, 3)) * (L / (2 * N))).astype(np.float32)
        vel, rho = _integer_payload(rng, n)
        ref = smr.quantity(smr.moments(pos, vel, rho, N, L, assignment), L / N, "subgrid_energy")
        data.append((_dev(K, pos, vel, rho), [ref]))
    (true, ref), (decoy, decoy_ref) = data
    bufs = [b.clone() for b in decoy]
    case = sp.Case("deposit_field-subgrid-%s" % assignment, bufs, list(true),
                   lambda: [K.deposit_field(bufs[0], bufs[1], bufs[2], N, L, 0, N, D.SUBGRID_ENERGY, assignment=assignment)[0]],
                   ref, decoy_ref, ["field"])
    sp.run_case(case, CACHE["blocker"])


# ------------------------------------------------------------------ g. refusals ----
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
    out = torch.full((4, N, N, N), nan, dtype=torch.float32, device=K.device)
    spec = torch.full((3, N // 2, N, N, 2), nan, dtype=torch.float32, device=K.device)
    nyq = torch.full((3, N, N, 2), nan, dtype=torch.float32, device=K.device)
    zimg = torch.full((4 * K.zimage_elems(N, N), 2), nan, dtype=torch.float32, device=K.device)
    work = K.workspace("refusals", max(lib.vps_deposit_assign_workspace_bytes(n, 4, N, 3), lib.vps_deposit_fft_zy_workspace_bytes_shared(n, N, N),
                                       lib.vps_nn_workspace_bytes(n, 0, N ** 3), lib.vps_deposit_workspace_bytes(n, 4, N, N)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ax = np.ascontiguousarray((np.arange(N) + 0.5) / N)
    names = {D.TOTAL_ENERGY: "VPS_TOTAL_ENERGY", D.SUBGRID_ENERGY: "VPS_SUBGRID_ENERGY", D.DISPERSION: "VPS_DISPERSION"}
    K._stream()

    def refused(rc, q):
        msg = lib.vps_last_error(K.ctx).decode()
        assert rc == -1 and ("quantity %d" % q in msg or names[q] in msg), (q, rc, msg)
        torch.cuda.synchronize()
        for buf in (out, spec, nyq, zimg):
            assert bool(torch.isnan(buf).all()), "a refused call wrote something"
        assert torch.equal(chans, chans0)

    for q in names:
        assert lib.vps_deposit_fft_zy_supported(K.ctx, N, q) == 0 and lib.vps_deposit_fft_zy_supported(K.ctx, 64, q) == 0
        assert lib.vps_deposit_fft_zy_supported(K.ctx, 64, D.ENERGY) == 1
        refused(lib.vps_field_algebra(K.ctx, q, 0, L / N, p(chans), N ** 3), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, 0, L / N, p(chans), N ** 3, p(out)), q)
        refused(lib.vps_nn_resample_quantity(K.ctx, p(pos), 0, p(rhov), n, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N,
                                             0, N, L / N, q, 0, p(out), None, p(work)), q)
        refused(lib.vps_deposit_fft_zy(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(spec), p(nyq), p(work)), q)
        refused(lib.vps_deposit_fft_z(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        refused(lib.vps_deposit_fft_z_slab(K.ctx, p(pos), 0, p(vel), p(rho), n, n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        for flags in (D.FLAG_REFERENCE_MOMENTUM_BUG, D.FLAG_INPUT_IS_VM, D.FLAG_ASSIGN("cic") | D.FLAG_REFERENCE_MOMENTUM_BUG,
                      D.FLAG_ASSIGN("tsc") | D.FLAG_INPUT_IS_VM):
            refused(lib.vps_deposit_field(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, flags, p(out), p(work)), q)
    # ... and the context still deposits
    got = K.deposit_field(pos, vel, rho, N, L, 0, N, D.TOTAL_ENERGY)[0].double().cpu().numpy()
    m = smr.moments(pos.cpu().numpy(), vel.cpu().numpy(), rho.cpu().numpy(), N, L)
    assert np.all(np.abs(got - smr.quantity(m, L / N, "total_energy")) <= (m["n"] + 8) * U * (L / N) ** 3 * m["S2"])


# ------------------------------------------------------------------ h. spectra and surface ----
@pytest.fixture(scope="module")
def surface():
    rng = np.random.default_rng(21)
    N, n, L = 64, 400_000, 2.0
    pos = (rng.random((n, 3)) * L).astype(np.float32)
    pos[:100] = np.array([L - 1e-4, 1e-5, L / 2], dtype=np.float32)          # periodic wrap on two faces
    vel = (rng.standard_normal((n, 3)) + np.sin(2 * np.pi * pos[:, ::-1] / L)).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    return N, L, pos, vel, dens


@pytest.mark.parametrize("assignment", ["ngp", "cic"])
def test_spectra_and_real_space_grids(K, surface, assignment):
    """spctrm of the three names on a lazy particle-backed field (NGP; fused CIC with deconvolve=True): Nsample exact, Psum
    within 2e-5 of the float64 table of the reference field; the spectrum does not materialise the field.  Parseval: over a k
    range that holds every mode but k = 0 the shell sums of 'subgrid_energy' add up to 0.5 a^2 (N^3 sum f^2 - (sum f)^2) of the
    real-space grid BoxField.subgrid_energy() returns."""
    from vpower import interp
    N, L, pos, vel, dens = surface
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    box = gp.deposit_to_field(N) if assignment == "ngp" else gp.deposit_to_field(N, assignment=assignment, method="fused")
    key = ("surface", assignment)
    if key not in CACHE:
        CACHE[key] = smr.moments(pos, vel, dens, N, L, assignment)
    m = CACHE[key]
    window = None if assignment == "ngp" else assignment
    for q in smr.QUANTITIES:
        s = box.spctrm(q, deconvolve=window is not None)
        assert box._chans is None and box._src is not None, "a spectrum must not materialise the field"
        r = smr.table(smr.quantity(m, L / N, q), L, N, window=window)
        rel = float(np.max(np.abs(s.Psum - r[:, 2]) / np.abs(r[:, 2])))
        print("%s %s: max relative Psum error %.3g" % (assignment, q, rel))
        assert np.array_equal(s.Nsample, r[:, 3]), q
        assert np.allclose(s.Psum, r[:, 2], rtol=PSUM_RTOL, atol=0), (q, rel)
    grids = {"subgrid_energy": box.subgrid_energy(), "total_energy": box.total_energy(), "dispersion": box.dispersion()}
    assert box._src is not None and box._chans is None
    for q, g in grids.items():
        ref = smr.quantity(m, L / N, q)
        assert g.shape == (N, N, N) and g.dtype == np.float64 and g.min() >= 0
        assert np.abs(g - ref).max() <= 1e-5 * np.abs(ref).max(), q
    kf = 2 * np.pi / L
    s = box.spctrm("subgrid_energy", kmin=kf, kmax=np.sqrt(3.0) * (N // 2 + 1) * kf, kres=kf)
    f = grids["subgrid_energy"]
    a = orc.power_const(L, N)
    want = 0.5 * a * a * (N ** 3 * np.sum(f * f) - np.sum(f) ** 2)
    assert float(np.sum(s.Nsample)) == N ** 3 - 1
    assert abs(float(np.sum(s.Psum)) - want) <= PSUM_RTOL * want, (float(np.sum(s.Psum)), want)


def test_fields_without_particles_raise_by_name(K, surface):
    from vpower import interp
    N, L, pos, vel, dens = surface
    gp = interp.GasParticles(pos[:5000], dens[:5000] * (L / 16) ** 3, dens[:5000], vel[:5000], L)
    for box in (gp.ann_interp_to_field(16), gp.deposit_to_field(16, assignment="cic", method="direct")):
        for q in smr.QUANTITIES:
            with pytest.raises(Exception, match=q):
                box.spctrm(q)
    box = gp.deposit_to_field(16)
    box.vx                                          # materialised: four channels, the particles are let go
    with pytest.raises(Exception, match="subgrid_energy"):
        box.subgrid_energy()


@pytest.fixture(scope="module")
def snapshot(tmp_path_factory):
    d = tmp_path_factory.mktemp("second_moment_driver")
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
    """parallel_optimized.py --quantity subgrid_energy --gridding cic at N = 32: the in-process run (one rank) against the float64
    reference of the driver's own preprocessing, and two gloo ranks sharing the GPU against the one-rank table -- counts exact,
    sums to 2e-5.  The children run under a time limit of their own; a failing child ends the test, nothing is tried again."""
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
    common = ["-i", path, "-N", str(N), "-l", str(L), "-f", "--quantity", "subgrid_energy", "--gridding", "cic"]
    assert po.main(common + ["-o", str(out1)]) == 0
    one = np.loadtxt(str(out1 / "Pk.txt"))
    z = np.load(path)
    dpos, dvel = K.to_device(z["Coordinates"]), K.to_device(z["Velocities"])
    K.preprocess(dpos, dvel, K.to_device(z["Masses"]), True, True)
    m = smr.moments(dpos.cpu().numpy(), dvel.cpu().numpy(), z["Density"], N, float(L), "cic")
    r = smr.table(smr.quantity(m, L / N, "subgrid_energy"), float(L), N, flavour="script")
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
