"""Edge-shape parity of the small kernels at the two ends of the pipeline: preprocess.hip (prep_reduce, prep_apply,
totals_kernel), hist.hip (pair_k_kernel, hist_pairs_kernel) and assign_expand_kernel / rhov_kernel of deposit.hip, each against a
plain float64 reference (oracle/vps_oracle.py, tests/small_ref.py, numpy) at the counts where a thread takes a second
grid-stride trip, around one wave and one workgroup, and at the values the hot-path tests never reach (negative minima, values
on histogram edges, positions on cell faces and far outside the box).
Run on an MI355X:  python -m pytest tests/test_gpu_small_kernels.py -q -m gpu
Every test calls through vpower.device / the C ABI.  The bars are derived in DESIGN.md section 3 ("Small kernels")."""
import numpy as np
import pytest
import torch

import small_ref as sr
from helpers import golden
from oracle import vps_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from vpower import device
    return device.default_kernels()


@pytest.fixture(scope="module")
def T(K):
    """Elements one trip of the capped grid-stride reductions covers: num_cu * 8 workgroups of 256 threads."""
    return K.device_info()["num_cu"] * 8 * 256


def _count(T, tag):
    return {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+77": 3 * T + 77}.get(tag, tag)


COUNTS = [1, 63, 64, 65, 255, 256, 257, "T-1", "T", "T+1", "3T+77"]


def _marked(n, T):
    """Where the extremes go: the first element, the last, and one in the middle of the last (partial) trip."""
    last_trip = (n - 1) // T * T
    return 0, n - 1, last_trip + (n - 1 - last_trip) // 2


def _below(x, dtype):
    """A value below x: for float64 one that float32 cannot hold."""
    if dtype == np.float64:
        v = np.nextafter(np.float64(x) - 0.25, -np.inf)
        assert np.float64(np.float32(v)) != v
        return v
    return np.float32(x) - np.float32(0.25)


# ------------------------------------------------------------------ 1. preprocess ----
@pytest.fixture(scope="module")
def particles(T):
    """One draw for every count (prefixes are used): velocities with a mean offset, log-normal masses, uniform [0, 1)."""
    rng = np.random.default_rng(101)
    n = 3 * T + 77
    vel = (rng.standard_normal((n, 3)) * 0.8 + np.array([0.3, -0.35, 0.25])).astype(np.float32)
    mass = np.exp(0.7 * rng.standard_normal(n)).astype(np.float32)
    return rng.random((n, 3)), vel, mass


def _pos_all_negative_minima(u, n, T, dtype):
    pos = (u[:n] * 4.0 - 2.5).astype(dtype)                 # [-2.5, 1.5): every axis minimum is negative
    for a, i in enumerate(_marked(n, T)):
        pos[i, a] = _below(-2.5, dtype)
    return pos


def _pos_mixed_signs(u, n, T, dtype):
    """x entirely positive, y entirely negative, z >= 0 with -0.0 and +0.0 both present as its extreme."""
    pos = np.empty((n, 3), dtype=dtype)
    pos[:, 0] = u[:n, 0] * 2.5 + 0.5
    pos[:, 1] = -(u[:n, 1] * 2.5 + 0.5)
    pos[:, 2] = u[:n, 2] * 2.0 + 0.125
    i0, i1, i2 = _marked(n, T)
    pos[i1, 0] = _below(0.5, dtype)                          # the smallest positive value: last element
    pos[i2, 1] = _below(-3.0, dtype)                         # the most negative: in the last trip
    pos[i0, 2] = 0.0
    pos[i2, 2] = -0.0
    return pos


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("count", COUNTS)
def test_preprocess_minimum_shift_and_bulk(K, T, particles, count, dtype):
    """vps_preprocess: the minimum is numpy's, exactly, wherever it sits (first element, last, last partial trip of the capped
    grid) and whatever its sign -- the order-preserving image behind atomicMin has one branch per sign; the shifted positions
    are numpy's, exactly; the bulk velocity is the float32 nearest the float64 quotient (one ulp: the order of the float64
    sums moves the quotient by 1e-13) and the velocities are exactly vel - float32(bulk).  The shift-only and the bulk-only
    forms likewise.  NaN and infinite positions are out of scope: fmin drops a NaN, numpy's min propagates it."""
    n = _count(T, count)
    u, vel, mass = particles
    vel, mass = vel[:n], mass[:n]
    m64 = mass.astype(np.longdouble)
    ref_bulk = np.array([float((m64 * vel[:, a]).sum() / m64.sum()) for a in range(3)])
    dmass = K.to_device(mass)

    # both steps, every minimum negative
    pos = _pos_all_negative_minima(u, n, T, dtype)
    dp, dv = K.to_device(pos), K.to_device(vel)
    mn, bv = K.preprocess(dp, dv, dmass)
    assert np.array_equal(mn, pos.min(axis=0).astype(np.float64)), (mn, pos.min(axis=0))
    assert np.array_equal(dp.cpu().numpy(), pos - pos.min(axis=0))
    assert dp.dtype == (torch.float32 if dtype == np.float32 else torch.float64)
    ulp = np.abs(np.spacing(ref_bulk.astype(np.float32))).astype(np.float64)
    print("bulk", bv, "ref", ref_bulk, "err/ulp", np.abs(bv - ref_bulk) / ulp)
    assert np.all(np.abs(bv - ref_bulk) <= ulp)
    assert np.array_equal(bv, bv.astype(np.float32).astype(np.float64))
    assert np.array_equal(dv.cpu().numpy(), vel - bv.astype(np.float32))

    # shift only: one axis positive, one negative, one with both zeros as its extreme
    pos2 = _pos_mixed_signs(u, n, T, dtype)
    dp = K.to_device(pos2)
    mn, bv0 = K.preprocess(dp, None, None, shift_to_origin=True, remove_bulk_velocity=False)
    assert np.array_equal(mn, pos2.min(axis=0).astype(np.float64)), (mn, pos2.min(axis=0))
    assert np.array_equal(dp.cpu().numpy(), pos2 - pos2.min(axis=0))
    assert np.all(bv0 == 0)

    # bulk only: the positions come back bit for bit
    dp, dv = K.to_device(pos2), K.to_device(vel)
    mn0, bv2 = K.preprocess(dp, dv, dmass, shift_to_origin=False, remove_bulk_velocity=True)
    assert np.all(mn0 == 0) and np.all(np.abs(bv2 - ref_bulk) <= ulp)
    back = dp.cpu().numpy()
    assert np.array_equal(back.view(np.uint32 if dtype == np.float32 else np.uint64),
                          pos2.view(np.uint32 if dtype == np.float32 else np.uint64))
    assert np.array_equal(dv.cpu().numpy(), vel - bv2.astype(np.float32))


def test_preprocess_refusals_leave_the_context_usable(K):
    from vpower import _ffi
    with pytest.raises(_ffi.VpsError, match="need at least one particle"):
        K.preprocess(K.zeros((0, 3), torch.float32), K.zeros((0, 3), torch.float32), K.zeros((0,), torch.float32))
    pos = np.array([[1.0, -2.0, 3.0], [0.5, -1.0, 4.0]], dtype=np.float32)
    dp, dv = K.to_device(pos), K.to_device(np.ones((2, 3), dtype=np.float32))
    with pytest.raises(_ffi.VpsError, match="total mass is zero"):
        K.preprocess(dp, dv, K.zeros((2,), torch.float32))
    dp = K.to_device(pos)
    mn, _ = K.preprocess(dp, None, None, remove_bulk_velocity=False)
    assert np.array_equal(mn, [0.5, -2.0, 3.0]) and np.array_equal(dp.cpu().numpy(), pos - pos.min(axis=0))


# ------------------------------------------------------------------ 2. totals ----
TOTALS_RTOL = 1e-12      # of the sum of the absolute terms: the project's float64 bar


def _check_totals(got, v, mass):
    ref, ab = sr.totals_exact(v, mass)
    print("totals err / sum|term|", np.abs(got - ref) / np.where(ab > 0, ab, 1))
    assert np.all(np.abs(got - ref) <= TOTALS_RTOL * ab), (got, ref, ab)


@pytest.mark.parametrize("count", COUNTS)
def test_totals_particle_and_field_layout(K, T, particles, count):
    """vps_totals over [n, 3] velocities (strides 3, 1) and over the channel-major [4, n] form (strides 1, n), against sums in
    extended precision of the float32 inputs promoted to float64."""
    n = _count(T, count)
    _, vel, mass = particles
    vel, mass = vel[:n], mass[:n]
    dv, dm = K.to_device(vel), K.to_device(mass)
    _check_totals(K.particle_totals(dv, dm), vel, mass)
    _check_totals(K.totals(dv, dm, 3, 1, n), vel, mass)
    chans = K.to_device(np.concatenate((vel.T, mass[None, :]), axis=0))       # [4, n]
    _check_totals(K.totals(chans, chans[3], 1, n, n), vel, mass)


def test_totals_of_a_field_larger_than_one_trip_and_of_nothing(K, T, particles):
    N = 96
    n = N ** 3
    assert n > T
    _, vel, mass = particles
    chans = np.concatenate((vel[:n].T, mass[None, :n]), axis=0).reshape(4, N, N, N)
    _check_totals(K.field_totals(K.to_device(chans)), vel[:n], mass[:n])
    assert np.array_equal(K.totals(K.zeros((0, 3), torch.float32), K.zeros((0,), torch.float32), 3, 1, 0), np.zeros(5))


# ------------------------------------------------------------------ 3. un-fused binning ----
@pytest.mark.parametrize("N,L", [(96, 1.0), (250, 2.5), (128, 1.0)])
def test_pair_k_bit_exact(K, N, L):
    """sqrt((kx kx + ky ky) + kz kz) over the 'ij' meshgrid of three DIFFERENT axes, one of them shifted as the script shifts
    it: the kernel is compiled without contraction, so every value is numpy's."""
    ks = orc.k_axis(L, N)
    ax = [ks - 2 * np.pi / L * 0.25, ks * 1.5, ks[::-1].copy()]
    got = K.pair_k(*ax).cpu().numpy()
    kx, ky, kz = np.meshgrid(*ax, indexing="ij")
    assert np.array_equal(got, np.sqrt((kx * kx + ky * ky) + kz * kz).ravel())


@pytest.fixture(scope="module")
def hist_inputs():
    rng = np.random.default_rng(7)
    n = 128 ** 3
    return rng.random(n), sr.dyadic_weights(rng, n)


def _library_edges():
    kmin, kmax, kres = orc.default_k_range(1.0, 1024)
    c, e = orc.edges_library(kmin, kmax, kres)
    assert np.array_equal(c, golden("bin_edges.npz")["library_centres_1024"])
    return e


def _check_hist(K, k, w, edges):
    """Counts exact, sums to 1e-12 (the weights are dyadic: numpy's sums are exact, and so is any correct kernel's), the
    count-only form, and accumulation over two calls."""
    ref_n, _ = np.histogram(k, bins=edges)
    ref_s, _ = np.histogram(k, bins=edges, weights=w)
    dk, dw = K.to_device(k), K.to_device(w)
    psum, ns = K.hist_pairs(dk, dw, edges)
    assert ns.dtype == torch.int64 and np.array_equal(ns.cpu().numpy(), ref_n)
    assert np.allclose(psum.cpu().numpy(), ref_s, rtol=1e-12, atol=0)
    psum1, ns1 = K.hist_pairs(dk, None, edges)
    assert np.array_equal(ns1.cpu().numpy(), ref_n) and np.array_equal(psum1.cpu().numpy(), ref_n.astype(np.float64))
    K.hist_pairs(dk, dw, edges, psum=psum, nsample=ns)                      # the kernel ADDS
    assert np.array_equal(ns.cpu().numpy(), 2 * ref_n)
    assert np.allclose(psum.cpu().numpy(), 2 * ref_s, rtol=1e-12, atol=0)
    return ref_n


@pytest.mark.parametrize("count", [1, 257, 128 ** 3])
@pytest.mark.parametrize("edges_name", ["linspace", "library", "repeat_mid", "repeat_end", "one_bin"])
def test_hist_pairs_matches_numpy_histogram(K, T, hist_inputs, edges_name, count):
    """numpy.histogram(k, edges[, weights]) on values that sit ON every edge, one float64 step to either side of it, outside
    the range, on e[-1] (the last bin is right-closed; that value is the LAST element, in the last grid-stride trip) and NaN."""
    base, w = hist_inputs
    edges = sr.hist_edge_sets(_library_edges())[edges_name]
    assert count == 1 or count == 257 or count > T
    k = sr.hist_values(base, edges, count)
    assert k[-1] == edges[-1]
    ref_n = _check_hist(K, k, w[:count], edges)
    assert ref_n[-1] >= 1                                               # e[-1] itself was counted


def test_hist_pairs_bin_limit(K, hist_inputs):
    """The largest admitted number of bins (the histogram of a workgroup lives in LDS) gives numpy's histogram; one more bin is
    refused on the host, by name, and the context goes on working."""
    from vpower import _ffi
    base, w = hist_inputs
    nmax = K.device_info()["hist_max_bins"]
    lds = K.lib.vps_hist_max_bins(K.ctx)
    print("hist_max_bins", nmax)
    assert nmax == lds and nmax >= 3276                                 # 64 KiB of LDS at the least
    n = 600011
    edges = np.linspace(1.0, 1.0 + nmax / 8.0, nmax + 1)
    k = sr.hist_values(base, edges, n)
    _check_hist(K, k, w[:n], edges)
    edges1 = np.linspace(1.0, 1.0 + (nmax + 1) / 8.0, nmax + 2)
    with pytest.raises(_ffi.VpsError, match="at most %d bins" % nmax):
        K.hist_pairs(K.to_device(k), None, edges1)
    small = np.array([1.0, 2.0, 3.0])
    _, ns = K.hist_pairs(K.to_device(np.array([1.5, 2.5, 3.0, 0.5])), None, small)
    assert np.array_equal(ns.cpu().numpy(), [1, 2])


# ------------------------------------------------------------------ 4. CIC / TSC expansion ----
GRIDS = [(250, 2.5), (96, 1.0), (2048, 1.0)]
DENSE_CELLS = 1 << 24        # dense float64 oracle grids up to this many values, the sparse form of it beyond


def _assign_positions(N, L, n, dtype, seed):
    """n positions: the rows where the expansion can go wrong first (faces, centres, their float neighbours, the first and the
    last cell of every axis, outside the box, FAR outside the box), uniform ones after them."""
    rng = np.random.default_rng(seed)
    lc = L / N
    i = np.array([0, 1, 2, N // 2, N - 2, N - 1, N], dtype=np.float64)
    faces, centres = i * lc, (i + 0.5) * lc
    special = np.concatenate([
        [0.37 * L],                                                     # (an ordinary first particle: count 1)
        faces, centres,
        np.nextafter(faces.astype(dtype), dtype(-np.inf)), np.nextafter(faces.astype(dtype), dtype(np.inf)),
        np.nextafter(centres.astype(dtype), dtype(-np.inf)), np.nextafter(centres.astype(dtype), dtype(np.inf)),
        rng.random(12) * lc, L - rng.random(12) * lc,                    # within one cell of 0 and of L
        [-0.3 * L, 1.7 * L, -L, 2 * L, 0.0, -0.0, L],
        [1e10, -1e10, 3e7 * L, -2.9e8 * lc],                            # the far values of the NGP edge test
    ])
    m = min(n, 3 * len(special))
    pos = rng.random((n, 3)) * L
    # every special value on every axis, against ordinary values on the other two
    for a in range(3):
        rows = np.arange(a, m, 3)
        pos[rows, a] = special[(rows // 3) % len(special)]
    if n > 1:
        pos[n - 1] = [1e10, (N - 0.5) * lc, -2.9e8 * lc]                 # the last thread of the last block
    return pos.astype(dtype)


def _expand(K, pos, f, N, L, assignment):
    pe, fe = K.assign_expand(K.to_device(pos), K.to_device(f), N, L, assignment)
    S = sr.ORDER[assignment] ** 3
    assert pe.shape == (len(pos) * S, 3) and fe.shape == (len(pos) * S, f.shape[1])
    return pe.cpu().numpy(), fe.cpu().numpy()


def _check_expand(K, pos, f, N, L, assignment):
    """The kernel's own records, binned in float64 by the rule the NGP deposit applies to them, against the oracle per cell."""
    pe, fe = _expand(K, pos, f, N, L, assignment)
    assert np.all(pe >= 0) and np.all(pe < np.float32(L))
    ci = orc.cell_index(pe, N, L)
    got_cells, got = sr.sparse_sum((ci[:, 0] * N + ci[:, 1]) * N + ci[:, 2], fe)
    f64 = f.astype(np.float64)
    if N ** 3 * f.shape[1] <= DENSE_CELLS:
        ref_cells, ref = sr.dense_to_sparse(orc.deposit_assign(f64, pos, N, L, assignment))
        bar_cells, bar = sr.dense_to_sparse(orc.deposit_assign(np.abs(f64), pos, N, L, assignment))
    else:
        ref_cells, ref = sr.deposit_assign_sparse(f64, pos, N, L, assignment)
        bar_cells, bar = sr.deposit_assign_sparse(np.abs(f64), pos, N, L, assignment)
    cells = np.union1d(np.union1d(got_cells, ref_cells), bar_cells)
    got, ref, bar = sr.sparse_on(cells, got_cells, got), sr.sparse_on(cells, ref_cells, ref), sr.sparse_on(cells, bar_cells, bar)
    err = np.abs(got - ref)
    worst = np.max(err / np.where(bar > 0, bar, np.inf), initial=0.0)
    print("expand %s N=%d n=%d: worst per-cell error / (sum |f| w) = %.3g (bar %.3g), largest error where the oracle has nothing %.3g"
          % (assignment, N, len(pos), worst, sr.RECORD_RTOL, np.max(err[bar == 0], initial=0.0)))
    assert np.all(err <= sr.RECORD_RTOL * bar + sr.F32_TINY)
    # the channel sums are the payload's
    tot, ab = f64.sum(axis=0), np.abs(f64).sum(axis=0)
    assert np.all(np.abs(fe.astype(np.float64).sum(axis=0) - tot) <= 27 * sr.RECORD_RTOL * ab)


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("N,L", GRIDS)
def test_assign_expand_per_cell(K, N, L, C, dtype, assignment):
    """100 003 particles (no multiple of 256): the weighted sub-particles of assign_expand, WITHOUT the float32 deposit, per
    cell within 16 * 2^-24 of the oracle's deposit of |f| -- including positions on faces and centres, next to them, outside
    the box and 1e10 away from it (the oracle's int64 % says where those belong)."""
    n = 100003
    pos = _assign_positions(N, L, n, dtype, seed=N + C)
    f = np.random.default_rng(C).standard_normal((n, C)).astype(np.float32)
    _check_expand(K, pos, f, N, L, assignment)


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("count", [1, 255, 257])
def test_assign_expand_small_counts(K, count, dtype, assignment):
    """Around one workgroup: one particle, one short of a block, one over it (the special rows come first)."""
    for (N, L), C in (((250, 2.5), 4), ((2048, 1.0), 1), ((96, 1.0), 4)):
        pos = _assign_positions(N, L, count, dtype, seed=count)
        f = np.random.default_rng(count).standard_normal((count, C)).astype(np.float32)
        _check_expand(K, pos, f, N, L, assignment)


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,L", GRIDS)
def test_assign_expand_weights_are_a_partition_of_unity(K, N, L, dtype, assignment):
    n = 1031
    pos = _assign_positions(N, L, n, dtype, seed=5)
    _, fe = _expand(K, pos, np.ones((n, 1), dtype=np.float32), N, L, assignment)
    wsum = fe.astype(np.float64).reshape(n, -1).sum(axis=1)
    assert np.all(fe >= 0) and np.all(np.abs(wsum - 1) <= 27 * sr.RECORD_RTOL), np.abs(wsum - 1).max()


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_deposit_to_grid_assignment_n250(K, assignment):
    """Through the float32 deposit, N not a power of two, Lbox != 1: the existing bar of the N = 32 test."""
    from vpower import interp
    N, L, n = 250, 2.5, 100003
    pos = _assign_positions(N, L, n, np.float32, seed=9)
    f = np.random.default_rng(9).standard_normal(n).astype(np.float32)
    grid = interp.deposit_to_grid(f, pos, N, L, assignment=assignment)
    ref = orc.deposit_assign(f.astype(np.float64), pos, N, L, assignment)
    assert grid.shape == ref.shape
    assert np.allclose(grid, ref, rtol=0, atol=2e-5 * np.abs(ref).max())


def test_cic_on_cell_centres_is_the_ngp_deposit(K):
    """A particle on a cell centre has CIC weights exactly 1 and 0 (Lcell = 2^-7 here, so that the centres are exact): with
    small-integer payloads the CIC grid IS the NGP grid of the same particles, cell for cell."""
    from vpower import interp
    N, L, n = 96, 96 / 128.0, 40001
    rng = np.random.default_rng(3)
    cell = rng.integers(0, N, (n, 3))
    cell[:4] = [[0, 0, 0], [N - 1, N - 1, N - 1], [0, N - 1, 7], [N - 1, 0, 0]]
    pos = (cell + 0.5) * (L / N)
    f = rng.integers(-8, 9, (n, 4)).astype(np.float32)
    for p in (pos, pos.astype(np.float32)):
        assert np.array_equal(orc.cell_index(p, N, L), cell)
        cic = interp.deposit_to_grid(f, p, N, L, assignment="cic")
        ngp = interp.deposit_to_grid(f, p, N, L)
        assert np.array_equal(cic, ngp)
        assert np.array_equal(cic.sum(axis=(0, 1, 2)), f.astype(np.float64).sum(axis=0))


@pytest.mark.parametrize("count", [1, 255, 257, "T+1"])
def test_density_velocity_vector_bit_exact(K, T, particles, count):
    n = _count(T, count)
    _, vel, rho = particles
    got = K.density_velocity_vector(K.to_device(vel[:n]), K.to_device(rho[:n])).cpu().numpy()
    ref = orc.density_velocity_vector(vel[:n], rho[:n])
    assert ref.dtype == np.float32 and np.array_equal(got, ref)
    assert np.array_equal(got[:, :3], vel[:n] * rho[:n, None]) and np.array_equal(got[:, 3], rho[:n])


# ---- one per-cell quantity algebra (csrc/quantity.h, deposit.hip: cell_quantity) --------------------------------------------------
# The brick epilogue, the grid kernel and the rho arms of the NN emit form a quantity through the same inline functions, so two
# routes that reach them with the same [rho v, rho] must agree bit for bit -- nothing here needs a tolerance.
def _quantities():
    from vpower import device as D
    return [("velocity", D.VELOCITY, 0), ("momentum", D.MOMENTUM, 0), ("momentum_bug", D.MOMENTUM, D.FLAG_REFERENCE_MOMENTUM_BUG),
            ("energy", D.ENERGY, 0), ("vm", D.VM, 0), ("weighted_third", D.WeightedVelocity(1.0 / 3.0), 0),
            ("weighted_minus_half", D.WeightedVelocity(-0.5), 0), ("density_1", D.Density(1.0), 0),
            ("density_half", D.Density(0.5), 0), ("log_density", D.LOG_DENSITY, 0)]


QUANTITY_IDS = [q[0] for q in _quantities()]


def _integer_particles(N, seed):
    """Integer-valued rho and v (cell totals are exact whatever the order of the LDS adds), a grid sparse enough to leave empty
    cells, a handful of particles without density."""
    rng = np.random.default_rng(seed)
    n = N ** 3 // 2
    pos = rng.random((n, 3)).astype(np.float32)
    vel = rng.integers(-4, 5, (n, 3)).astype(np.float32)
    rho = rng.integers(1, 6, n).astype(np.float32)
    rho[:: n // 7] = 0.0
    return pos, vel, rho


@pytest.fixture(scope="module")
def raw_grids(K):
    """N -> (particles on the device, the raw four-channel deposit of [rho v, rho]); computed once, never written to."""
    out = {}
    for N in (10, 16):
        pos, vel, rho = _integer_particles(N, 300 + N)
        dp, dv, dr = K.to_device(pos), K.to_device(vel), K.to_device(rho)
        raw = K.deposit(dp, K.density_velocity_vector(dv, dr), N, 1.0, 0, N).clone()
        assert int((raw[3] == 0).sum()) > N, "the grid is meant to have empty cells"
        out[N] = (dp, dv, dr, raw)
    return out


@pytest.mark.parametrize("N", [10, 16])       # 10: the brick kernel's scalar stream-out; 16: its vec4 path, partial bricks
@pytest.mark.parametrize("name", QUANTITY_IDS)
def test_deposit_field_is_deposit_then_field_algebra(K, raw_grids, name, N):
    from vpower import device as D
    _, q, flags = _quantities()[QUANTITY_IDS.index(name)]
    dp, dv, dr, raw = raw_grids[N]
    fused = K.deposit_field(dp, dv, dr, N, 1.0, 0, N, q, flags)
    grid = raw.clone()
    K.field_algebra(grid, q, flags, 1.0 / N)
    assert fused.shape[0] == D.NCOMP[int(q)]
    assert torch.equal(fused, grid[: fused.shape[0]])


@pytest.mark.parametrize("vm", [0, 1], ids=["rhov", "input_is_vm"])
@pytest.mark.parametrize("N", [10, 16])       # 10: 250 threads, a partial (and only) block
@pytest.mark.parametrize("name", QUANTITY_IDS)
def test_field_algebra_in_place_is_field_algebra_out(K, raw_grids, name, N, vm):
    from vpower import device as D
    _, q, flags = _quantities()[QUANTITY_IDS.index(name)]
    flags |= D.FLAG_INPUT_IS_VM if vm else 0
    rng = np.random.default_rng(17 + N)
    chans = raw_grids[N][3].clone()
    chans[:3] += K.to_device(rng.standard_normal((3, N, N, N)).astype(np.float32))     # float data: no atomics on this route
    chans[3] *= K.to_device(np.exp(rng.standard_normal((N, N, N))).astype(np.float32))
    keep = chans.clone()
    out = K.field_algebra_out(chans, q, flags, 1.0 / N)
    assert torch.equal(chans, keep), "field_algebra_out only reads its input"
    K.field_algebra(chans, q, flags, 1.0 / N)
    n = D.NCOMP[int(q)]
    assert out.shape[0] == n and torch.equal(chans[:n], out)
    assert torch.equal(chans[n:], keep[n:]), "the channels a quantity does not have stay what they were"


@pytest.fixture(scope="module")
def nn_inputs(K):
    rng = np.random.default_rng(91)
    n, N = 20000, 32
    pos = rng.random((n, 3)).astype(np.float32)
    vel = rng.standard_normal((n, 3)).astype(np.float32)
    rho = np.exp(0.5 * rng.standard_normal(n)).astype(np.float32)
    rho[:: n // 9] = 0.0
    dp = K.to_device(pos)
    pay = K.density_velocity_vector(K.to_device(vel), K.to_device(rho))
    ax = orc.lattice_axes_library(1.0, N)
    return dp, pay, (ax, ax, ax), N


# (the grid route forms alpha - 1 on the device in float, the NN route takes it from the host's double: the weighted velocity at
# exponents whose two forms of alpha - 1 agree)
@pytest.mark.parametrize("kernel", ["column", "query_centric"])
@pytest.mark.parametrize("name", ["weighted_half", "weighted_minus_half", "density_1", "density_half", "log_density"])
def test_nn_quantity_is_nn_payload_then_field_algebra(K, nn_inputs, name, kernel):
    from vpower import _ffi, device as D
    q = {"weighted_half": D.WeightedVelocity(0.5), "weighted_minus_half": D.WeightedVelocity(-0.5), "density_1": D.Density(1.0),
         "density_half": D.Density(0.5), "log_density": D.LOG_DENSITY}[name]
    dp, pay, axes, N = nn_inputs
    opt = "nn_column" if kernel == "column" else "nn_query_centric"
    _ffi.set_option(opt, 1)
    try:
        direct, i1 = K.nn_resample_quantity(dp, pay, axes, 0, N, 1.0 / N, q, want_index=True)
        assert K.nn_last_search()["kind"] == ("column" if kernel == "column" else "ring"), "the option did not select the search"
        raw, i0 = K.nn_resample(dp, pay, axes, 0, N, want_index=True)
    finally:
        _ffi.set_option(opt, None)
    assert torch.equal(i0, i1)
    assert int((raw[3] == 0).sum()) > 0, "some lattice points are meant to have a nearest particle without density"
    assert torch.equal(direct, K.field_algebra_out(raw, q, 0, 1.0 / N))
