"""float64 reference of the scalar density quantities s = rho^alpha ('density', VPS_DENSITY) and s = ln rho ('log_density',
VPS_LOG_DENSITY) and their spectra: test infrastructure, never imported by the package.  Built on tests/weighted_ref.py
(particles, grids, neighbour search) and the oracle's public functions:
    s = rho^alpha | ln rho where rho != 0,   s = 0 where rho = 0 (for every alpha, and for the logarithm)
    P = 0.5 |a FFT3(s)|^2                    (orc.scalar_power), binned like every quantity (orc.spectrum_table)
with rho the cell's density total (channel 3 of the deposited [rho v, rho] grid), the nearest particle's density (exact NN),
or mass / Lcell^3 of a gridded field."""
import numpy as np

from oracle import vps_oracle as orc

import weighted_ref as wref


def _rho(vec_grid_or_rho):
    a = np.asarray(vec_grid_or_rho, dtype=np.float64)
    return a[..., 3] if (a.ndim == 4 and a.shape[-1] == 4) else a


def density_field(vec_grid_or_rho, alpha=1.0):
    """rho^alpha (float64) of a [rho v, rho] grid (..., 4) or of a rho array; 0 where rho = 0.  alpha = 1 is rho itself."""
    rho = _rho(vec_grid_or_rho)
    return rho.copy() if alpha == 1.0 else wref.weight(rho, alpha)


def log_density_field(vec_grid_or_rho):
    """ln rho (float64), 0 where rho = 0."""
    rho = _rho(vec_grid_or_rho)
    return np.where(rho != 0, np.log(np.where(rho != 0, rho, 1.0)), 0.0)


def field(vec_grid_or_rho, which):
    """which: an exponent (float) or 'log'."""
    return log_density_field(vec_grid_or_rho) if which == "log" else density_field(vec_grid_or_rho, which)


def nn_rho(pos, dens, N, L):
    """The nearest particle's density on the library lattice (exact NN, as weighted_ref.nn_fields)."""
    ax = orc.lattice_axes_library(L, N)
    return dens.astype(np.float64)[orc.exact_nn_lattice(pos, ax, ax, ax)].reshape(N, N, N)


def slab_rho(pos, dens, N, L, x0, nx):
    """[nx][N][N] float64 density totals of the x-slab [x0, x0 + nx) (the oracle's cell rule, as weighted_ref.slab_fields)."""
    idx = orc.cell_index(pos, N, L)
    keep = (idx[:, 0] >= x0) & (idx[:, 0] < x0 + nx)
    idx = idx[keep]
    flat = ((idx[:, 0] - x0) * N + idx[:, 1]) * N + idx[:, 2]
    return np.bincount(flat, weights=dens[keep].astype(np.float64), minlength=nx * N * N).reshape(nx, N, N)


def table(f, L, N, flavour="library", kmin=None, kmax=None, kres=None, window=None):
    """(nbins, 4) [k, P 4 pi k^2, Psum, Nsample] of spctrm's layout for ONE scalar field."""
    P = orc.scalar_power(f, L, N)
    if window is not None:
        P = P * orc.window_inv2(N, window)
    return orc.spectrum_table(P, L, N, flavour, kmin, kmax, kres)


def fused_inputs(N, Np, L=1.0):
    """(pos, vel, dens) of the whole-grid legs: eight-decade densities, a fifth of the cells empty, and a tenth of the
    particles in a few y lines of ONE pencil (so that the pencil kernel's p.side[] tail runs)."""
    pos, vel, dens = wref.particles(N, Np, N, L)
    n_hot = Np // 10
    pos[:n_hot, 0] = (np.float32(1.5) + 0 * pos[:n_hot, 0]) / N
    pos[:n_hot, 1] = (np.float32(2.0) + pos[:n_hot, 1] * 6) / N
    return pos, vel, dens
