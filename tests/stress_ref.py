"""float64 reference of the tensor quantities (VPS_SUBGRID_STRESS, VPS_DISPERSION_TENSOR) and of the spectrum of their full
contraction: test infrastructure, never imported by the package.  Built on second_moment_ref.contributions.  Per cell, over the
contributions (particle p, weight w) it receives,
    S_ij = sum w rho_p v_i v_j,   P = sum w rho_p v_p,   R = sum w rho_p,   A_ii = sum w rho_p v_i^2 (the absolute sums)
and with vol = Lcell^3, d_ij = S_ij - P_i P_j / R,
    subgrid_stress = vol d_ij,   dispersion_tensor = d_ij / R
all 0 where R = 0, the three diagonal components clamped at 0 from below, the off-diagonal ones not.  Six components in the
order xx, yy, zz, xy, xz, yz."""
import numpy as np

import density_ref as dref
import second_moment_ref as smr

QUANTITIES = ("subgrid_stress", "dispersion_tensor")
IJ = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
SCALAR_OF = {"subgrid_stress": "subgrid_energy", "dispersion_tensor": "dispersion"}     # the trace


def moments(pos, vel, rho, N, L, assignment="ngp", x0=0, nx=None, box=None):
    """{"S": [6, nx, N, N], "A": [3, nx, N, N], "P": [3, nx, N, N], "R", "n": [nx, N, N]} float64 (n: contributions, int64) on
    the rows [x0, x0 + nx) (default: the whole grid).  box = (ny, nz): every contribution to those rows must lie in the corner
    y < ny, z < nz (asserted) and the arrays are [.., nx, ny, nz] -- the reference of a thin slab of a large grid without its
    empty cells."""
    nx = N if nx is None else nx
    who, flat, wt = smr.contributions(pos, N, L, assignment)
    ix = flat // (N * N)
    rows = (ix >= x0) & (ix < x0 + nx)
    who, flat, wt = who[rows], flat[rows] - x0 * N * N, wt[rows]
    if box is not None:
        ny, nz = box
        iy, iz = (flat // N) % N, flat % N
        assert iy.max() < ny and iz.max() < nz, "a contribution outside the reference's corner"
        flat = ((flat // (N * N)) * ny + iy) * nz + iz
        N = None
    v = np.asarray(vel, dtype=np.float64)[who]
    r = np.asarray(rho, dtype=np.float64)[who]
    shape = (nx, N, N) if box is None else (nx,) + tuple(box)
    cells = int(np.prod(shape))
    grid = lambda x: np.bincount(flat, weights=x, minlength=cells).reshape(shape)      # noqa: E731
    wr = wt * r
    return {"S": np.stack([grid(wr * v[:, i] * v[:, j]) for i, j in IJ]),
            "A": np.stack([grid(np.abs(wr) * v[:, i] * v[:, i]) for i in range(3)]),
            "P": np.stack([grid(wr * v[:, c]) for c in range(3)]), "R": grid(wr),
            "n": np.bincount(flat, minlength=cells).reshape(shape)}


def fields(m, Lcell, name):
    """[6, nx, N, N] float64 fields of one of QUANTITIES from moments()."""
    vol = Lcell ** 3
    R = m["R"]
    has = R != 0
    Rs = np.where(has, R, 1.0)
    out = []
    for c, (i, j) in enumerate(IJ):
        d = m["S"][c] - m["P"][i] * m["P"][j] / Rs
        if i == j:
            d = np.maximum(d, 0.0)
        if name == "subgrid_stress":
            out.append(np.where(has, vol * d, 0.0))
        elif name == "dispersion_tensor":
            out.append(np.where(has, d / Rs, 0.0))
        else:
            raise KeyError(name)
    return np.stack(out)


def trace(f6):
    return f6[0] + f6[1] + f6[2]


def bars(m, scale):
    """[6, nx, N, N]: the per-cell bar (n_c + 8) 2^-24 (A_ii + A_jj) / 2 of component ij, times `scale` (vol, or 1 / R)."""
    u = 2.0 ** -24
    return np.stack([(m["n"] + 8) * u * 0.5 * (m["A"][i] + m["A"][j]) * scale for i, j in IJ])


def table(f6, L, N, window=None, flavour="library"):
    """(nbins, 4) [k, P 4 pi k^2, Psum, Nsample] of the full contraction sum_ij |T_ij|^2 of the six fields: the diagonals once,
    the off-diagonals twice, each through density_ref.table; counted once."""
    tabs = [dref.table(f6[c], L, N, flavour=flavour, window=window) for c in range(6)]
    out = tabs[0].copy()
    for c in range(1, 6):
        out[:, 1] += (2.0 if c >= 3 else 1.0) * tabs[c][:, 1]
        out[:, 2] += (2.0 if c >= 3 else 1.0) * tabs[c][:, 2]
    return out
