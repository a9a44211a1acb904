"""float64 references for the small kernels at the two ends of the pipeline, where oracle/vps_oracle.py has none:
sparse forms of the CIC / TSC deposit (a dense float64 grid of 2048^3 cells is 64 GiB), the absolute-sum grid behind the
per-cell bars, exact totals, and the edge sets / probe values of the un-fused histogram.

TEST INFRASTRUCTURE ONLY; tests/test_small_ref_cpu.py pins every function here to the oracle or to numpy."""
import numpy as np

ORDER = {"cic": 2, "tsc": 3}

# A record of assign_expand is payload * wx * wy * wz in float32.  Each axis weight carries at most 3 float32 roundings (the
# cast of the float64 offset, and two of: the subtraction, the square, the product with 1/2), the two products of the three
# weights and the product with the payload 3 more: (1 + 2^-24)^12 - 1 < 16 * 2^-24.
RECORD_RTOL = 16 * 2.0 ** -24
# ... of a NORMAL float32: a record below the smallest normal one (a weight of 1e-32 next to a face, times two small ones) has
# no relative precision left, so a cell may be off by that much absolutely, whatever it holds.
F32_TINY = float(np.finfo(np.float32).tiny)


def assign_weights(pos, N, L, assignment):
    """(c0 int64 [np, 3], w float64 [np, 3, order]): first cell (NOT yet periodic) and per-axis weights of every particle --
    the same expressions, in the same order, as oracle.vps_oracle.deposit_assign."""
    s = np.asarray(pos, dtype=np.float64) / (L / float(N))
    if ORDER[assignment] == 2:
        c0 = np.floor(s - 0.5)
        fr = s - 0.5 - c0
        w = np.stack((1 - fr, fr), axis=-1)
    else:
        ic = np.floor(s)
        d = s - (ic + 0.5)
        c0 = ic - 1
        w = np.stack((0.5 * (0.5 - d) ** 2, 0.75 - d * d, 0.5 * (0.5 + d) ** 2), axis=-1)
    return c0.astype(np.int64), w


def sparse_sum(flat, values):
    """Sum the rows of values [n, C] (float64) that share a flat cell number: (cells sorted unique [m], sums [m, C])."""
    values = np.asarray(values, dtype=np.float64)
    cells, inv = np.unique(np.asarray(flat, dtype=np.int64), return_inverse=True)
    inv = inv.ravel()
    out = np.empty((len(cells), values.shape[1]))
    for c in range(values.shape[1]):
        out[:, c] = np.bincount(inv, weights=values[:, c], minlength=len(cells))
    return cells, out


def deposit_assign_sparse(f, pos, N, L, assignment):
    """oracle.vps_oracle.deposit_assign on the cells that receive something: (flat cell numbers sorted [m], sums [m, C]),
    flat = (ix N + iy) N + iz.  f is [np, C] float64."""
    order = ORDER[assignment]
    f = np.asarray(f, dtype=np.float64)
    c0, w = assign_weights(pos, N, L, assignment)
    flats, vals = [], []
    for jx in range(order):
        for jy in range(order):
            for jz in range(order):
                wt = w[:, 0, jx] * w[:, 1, jy] * w[:, 2, jz]
                flats.append((((c0[:, 0] + jx) % N) * N + (c0[:, 1] + jy) % N) * N + (c0[:, 2] + jz) % N)
                vals.append(f * wt[:, None])
    return sparse_sum(np.concatenate(flats), np.concatenate(vals))


def dense_to_sparse(grid):
    """A dense [N, N, N, C] grid in the form of deposit_assign_sparse: its nonzero cells."""
    g = grid.reshape(-1, grid.shape[-1])
    cells = np.flatnonzero(np.any(g != 0, axis=1))
    return cells, g[cells]


def sparse_on(cells, a_cells, a_vals):
    """The values of the sparse grid (a_cells, a_vals) on `cells` (sorted), zero where it has none."""
    out = np.zeros((len(cells), a_vals.shape[1]))
    i = np.searchsorted(cells, a_cells)
    assert np.all(i < len(cells)) and np.array_equal(cells[i], a_cells), "cells must contain every cell of the sparse grid"
    out[i] = a_vals
    return out


def totals_exact(v, mass):
    """(totals[5], abs[5]) for v [n, 3] and mass [n] float32: sum m, sum m v_c, sum m |v|^2 and the sums of the absolute terms,
    the float32 inputs promoted to float64 (m v_c is then exact) and summed in extended precision."""
    m = np.asarray(mass, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    terms = [m, m * v[:, 0], m * v[:, 1], m * v[:, 2], m * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])]
    tot = np.array([float(t.astype(np.longdouble).sum()) for t in terms])
    ab = np.array([float(np.abs(t).astype(np.longdouble).sum()) for t in terms])
    return tot, ab


# ---- the un-fused histogram ------------------------------------------------------------------------------------------------
def hist_edge_sets(library_edges):
    """{name: edges} of the histogram tests: np.linspace as the script builds them, the library's np.arange edges (from
    tests/golden/bin_edges.npz), two equal consecutive edges in the middle, two at the end, and one single bin."""
    lin = np.linspace(0.5 * 2 * np.pi, 64.5 * 2 * np.pi, 65)
    mid = np.array([1.0, 2.0, 3.5, 3.5, 5.0, 7.0, 11.0])
    end = np.array([1.0, 2.0, 3.5, 5.0, 7.0, 11.0, 11.0])
    return {"linspace": lin, "library": np.asarray(library_edges, dtype=np.float64), "repeat_mid": mid, "repeat_end": end,
            "one_bin": np.array([2.0, 9.0])}


def hist_probe_values(edges):
    """Values that sit where a histogram kernel goes wrong: every edge, its two float64 neighbours, values below the first and
    above the last edge, a few NaN (numpy and the kernel both ignore them) and, LAST, e[-1] itself (counted: the last bin is
    right-closed)."""
    e = np.asarray(edges, dtype=np.float64)
    span = e[-1] - e[0]
    return np.concatenate((e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), [e[0] - 0.1 * span, e[0] - 1e3, e[-1] + 0.1 * span,
                           e[-1] + 1e3, np.nan, np.nan, np.nan], [e[-1]]))


def hist_values(base01, edges, n):
    """n values for one edge set: base01 (uniform in [0, 1), at least n of them) stretched to 5 % beyond both ends of the
    edges, with hist_probe_values written over its END -- in the last grid-stride trip of a kernel, e[-1] in the last element."""
    e = np.asarray(edges, dtype=np.float64)
    span = e[-1] - e[0]
    k = (e[0] - 0.05 * span) + base01[:n] * (1.1 * span)
    p = hist_probe_values(e)[-n:]
    k[n - len(p):] = p
    return k


def dyadic_weights(rng, n):
    """Positive float64 weights k / 1024, k in [1, 2^20]: every partial sum of fewer than 2^33 of them is exact in float64,
    in ANY order.  numpy.histogram forms its weighted sums as differences of running sums over all the values, whose error
    is relative to the total, not to the bin: with such weights it is exact, and so is every correct kernel."""
    return rng.integers(1, 1 << 20, n).astype(np.float64) / 1024.0
