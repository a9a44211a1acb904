"""CPU pins of tests/small_ref.py (the references of tests/test_gpu_small_kernels.py) to the oracle and to numpy, and of the
numpy.histogram behaviour the GPU test assumes."""
import math

import numpy as np
import pytest

import small_ref as sr
from oracle import vps_oracle as orc


def _positions(N, L, n, seed):
    rng = np.random.default_rng(seed)
    lc = L / N
    pos = rng.random((n, 3)) * 3 * L - L                                  # inside and outside the box
    pos[:N + 1, 0] = np.arange(N + 1) * lc                                  # faces
    pos[:N, 1] = (np.arange(N) + 0.5) * lc                                  # centres
    pos[-4:, 2] = [1e10, -1e10, 3e7 * L, -2.9e8 * lc]
    return pos


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("C", [1, 4])
def test_sparse_deposit_is_the_oracles(assignment, C):
    N, L, n = 16, 2.5, 3000
    pos = _positions(N, L, n, 1)
    f = np.random.default_rng(2).standard_normal((n, C))
    dense = orc.deposit_assign(f, pos, N, L, assignment)
    cells, vals = sr.deposit_assign_sparse(f, pos, N, L, assignment)
    assert np.all(np.diff(cells) > 0) and cells.min() >= 0 and cells.max() < N ** 3
    full = np.zeros((N ** 3, C))
    full[cells] = vals
    bar = orc.deposit_assign(np.abs(f), pos, N, L, assignment).reshape(-1, C)
    assert np.all(np.abs(full - dense.reshape(-1, C)) <= 1e-13 * bar)       # the same terms, another order of float64 sums
    # the absolute-sum variant behind the bars, and the dense -> sparse form used below 2^24 cells
    bc, bv = sr.deposit_assign_sparse(np.abs(f), pos, N, L, assignment)
    assert np.all(bv >= 0) and np.allclose(sr.sparse_on(np.arange(N ** 3), bc, bv), bar, rtol=1e-13, atol=0)
    dc, dv = sr.dense_to_sparse(dense)
    assert np.array_equal(sr.sparse_on(np.arange(N ** 3), dc, dv), dense.reshape(-1, C))


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
def test_weights_are_a_partition_of_unity(assignment):
    N, L = 250, 2.5
    pos = _positions(N, L, 5000, 3)
    c0, w = sr.assign_weights(pos, N, L, assignment)
    assert w.shape == (5000, 3, sr.ORDER[assignment]) and np.all(w >= 0) and np.all(w <= 1)
    assert np.all(np.abs(w.sum(axis=-1) - 1) <= 4 * np.finfo(np.float64).eps)
    inside = (pos >= 0) & (pos < L)
    lo = c0[inside]
    assert lo.min() >= -1 and lo.max() <= N - 1                              # the first cell of an in-box particle
    assert c0[-4, 2] > 2 ** 31 and c0[-1, 2] < -2 ** 28                     # the far ones do not fit an int32 / need the wrap
    assert sr.RECORD_RTOL == 16 * 2.0 ** -24 and (1 + 2.0 ** -24) ** 12 - 1 < sr.RECORD_RTOL


def test_sparse_sum_and_alignment():
    cells, vals = sr.sparse_sum([5, 2, 5, 9, 2, 2], np.array([[1.0], [2.0], [3.0], [4.0], [5.0], [6.0]]))
    assert np.array_equal(cells, [2, 5, 9]) and np.array_equal(vals[:, 0], [13.0, 4.0, 4.0])
    on = sr.sparse_on(np.array([1, 2, 5, 7, 9]), cells, vals)
    assert np.array_equal(on[:, 0], [0.0, 13.0, 4.0, 0.0, 4.0])
    with pytest.raises(AssertionError):
        sr.sparse_on(np.array([1, 2, 5]), cells, vals)


def test_totals_exact_is_fsum():
    rng = np.random.default_rng(4)
    n = 20001
    v = (rng.standard_normal((n, 3)) + 0.3).astype(np.float32)
    m = np.exp(rng.standard_normal(n)).astype(np.float32)
    tot, ab = sr.totals_exact(v, m)
    m64, v64 = m.astype(np.float64), v.astype(np.float64)
    terms = [m64, m64 * v64[:, 0], m64 * v64[:, 1], m64 * v64[:, 2],
             m64 * ((v64[:, 0] * v64[:, 0] + v64[:, 1] * v64[:, 1]) + v64[:, 2] * v64[:, 2])]
    for a, t in enumerate(terms):
        assert abs(tot[a] - math.fsum(t)) <= 1e-15 * math.fsum(np.abs(t))
        assert abs(ab[a] - math.fsum(np.abs(t))) <= 1e-15 * ab[a]
    assert np.array_equal(sr.totals_exact(np.zeros((0, 3), np.float32), np.zeros(0, np.float32))[0], np.zeros(5))


def _by_definition(k, w, e):
    """e[i] <= k < e[i+1], the last bin right-closed: counts and fsum'd weights, straight from the definition."""
    nb = len(e) - 1
    cnt, tot = np.zeros(nb, dtype=np.int64), np.zeros(nb)
    for i in range(nb):
        sel = (k >= e[i]) & ((k < e[i + 1]) if i < nb - 1 else (k <= e[i + 1]))
        cnt[i] = sel.sum()
        tot[i] = math.fsum(w[sel])
    return cnt, tot


@pytest.mark.parametrize("name", ["linspace", "library", "repeat_mid", "repeat_end", "one_bin"])
def test_numpy_histogram_behaves_as_the_gpu_test_assumes(name):
    kmin, kmax, kres = orc.default_k_range(1.0, 64)
    edges = sr.hist_edge_sets(orc.edges_library(kmin, kmax, kres)[1])[name]
    assert np.all(np.diff(edges) >= 0)
    rng = np.random.default_rng(6)
    n = 5000
    k = sr.hist_values(rng.random(n), edges, n)
    w = sr.dyadic_weights(rng, n)
    assert k[-1] == edges[-1] and np.isnan(k).sum() == 3 and (k < edges[0]).any() and (k > edges[-1]).any()
    for v in edges:                                                          # every edge and both its neighbours are in there
        assert (k == v).any() and (k == np.nextafter(v, np.inf)).any() and (k == np.nextafter(v, -np.inf)).any()
    cnt, tot = _by_definition(k, w, edges)
    hn, _ = np.histogram(k, bins=edges)
    hs, _ = np.histogram(k, bins=edges, weights=w)
    assert np.array_equal(hn, cnt) and hn.sum() == np.sum((k >= edges[0]) & (k <= edges[-1]))
    assert np.array_equal(hs, tot)                                           # dyadic weights: exact in any order
    assert hn[-1] >= 1                                                       # the last edge is counted


def test_numpy_histogram_repeated_edges_and_the_last_edge():
    mid = sr.hist_edge_sets([0.0, 1.0])["repeat_mid"]
    j = int(np.flatnonzero(np.diff(mid) == 0)[0])                            # bins j = [3.5, 3.5) is empty, j + 1 starts at 3.5
    hn, _ = np.histogram([mid[j]], bins=mid)
    assert hn[j] == 0 and hn[j + 1] == 1 and hn.sum() == 1
    end = sr.hist_edge_sets([0.0, 1.0])["repeat_end"]
    hn, _ = np.histogram([end[-1]], bins=end)
    assert hn[-1] == 1 and hn.sum() == 1                                     # [11, 11]: closed, so it holds the value
    hn, _ = np.histogram([np.nextafter(end[-1], -np.inf)], bins=end)
    assert hn[-2] == 1 and hn.sum() == 1
    one = sr.hist_edge_sets([0.0, 1.0])["one_bin"]
    assert np.array_equal(np.histogram([one[0], one[1], np.nextafter(one[1], np.inf), np.nan], bins=one)[0], [2])


def test_dyadic_weights_sum_exactly():
    w = sr.dyadic_weights(np.random.default_rng(8), 100000)
    assert np.all(w > 0) and np.array_equal(w * 1024, np.round(w * 1024))
    assert np.sum(w) == math.fsum(w) == np.sum(w[::-1]) == float(np.cumsum(w)[-1])
