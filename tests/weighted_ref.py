"""float64 reference of the density-weighted velocity w = rho^alpha v and its spectra (BoxField.spctrm('weighted_velocity'),
VPS_WEIGHTED_VELOCITY): test infrastructure, never imported by the package.

Written from the definition, on the oracle's public functions:
    w_c = rho^alpha v_c where rho != 0,  w_c = 0 where rho = 0 (for every alpha, 0 included)
    P   = 0.5 sum_c |a FFT3(w_c)|^2     (orc.vector_power), binned like 'velocity' (orc.spectrum_table)
with v = (sum rho v) / rho and rho the cell's density total (NGP: orc.deposit_to_grid + orc.vm_from_vec_grid(zero_empty=True))
or the nearest particle's density (orc.exact_nn_lattice); for a gridded field rho = mass / Lcell^3."""
import numpy as np

from oracle import vps_oracle as orc

import helmholtz_ref as href


def eight_decade_densities(rng, n, decades=8.0):
    """float32 particle densities drawn log-uniformly over `decades` decades around 1 (so that rho^(alpha-1) is exercised far
    from rho = 1, where log2 rho = 0 hides the error of the power)."""
    return (10.0 ** ((rng.random(n) - 0.5) * decades)).astype(np.float32)


def particles(seed, Np, N, L=1.0, empty_fraction=0.2, decades=8.0):
    """(pos, vel, dens) float32: velocities with a mean flow, eight-decade densities, and about `empty_fraction` of the cells
    of an N^3 grid left empty (an x-y column pattern no particle is put into, plus the cells chance leaves empty)."""
    rng = np.random.default_rng(seed)
    pos = rng.random((Np, 3), dtype=np.float32) * np.float32(L)
    # particles that fall into the columns (ix + 2 iy) % 5 == 0 are moved one cell along x: a fifth of all cells stays empty
    if empty_fraction > 0:
        ix = np.floor(pos[:, 0].astype(np.float64) / (L / N)).astype(np.int64) % N
        iy = np.floor(pos[:, 1].astype(np.float64) / (L / N)).astype(np.int64) % N
        hit = (ix + 2 * iy) % 5 == 0
        moved = (pos[hit, 0].astype(np.float64) + L / N) % L
        pos[hit, 0] = np.minimum(moved, np.nextafter(np.float32(L), np.float32(0))).astype(np.float32)
    vel = (rng.standard_normal((Np, 3)) + np.array([0.3, -0.2, 0.1])).astype(np.float32)
    return pos, vel, eight_decade_densities(rng, Np, decades)


def weight(rho, exponent):
    """rho^exponent where rho != 0, else 0 -- float64."""
    rho = np.asarray(rho, dtype=np.float64)
    return np.where(rho != 0, np.power(np.where(rho != 0, rho, 1.0), exponent), 0.0)


def fields_from_vec_grid(vec_grid, alpha):
    """[w_x, w_y, w_z] (float64) from the deposited / resampled [rho v, rho] grid (..., 4)."""
    v, _ = orc.vm_from_vec_grid(vec_grid, 1.0, zero_empty=True)
    f = weight(vec_grid[..., 3], alpha)
    return [v[..., c] * f for c in range(3)]


def fields_from_vm(vx, vy, vz, mass, Lcell, alpha):
    """[w_x, w_y, w_z] of a gridded field: rho = mass / Lcell^3 (BoxField.get_density), 0 in empty cells."""
    rho = np.asarray(mass, dtype=np.float64) / Lcell ** 3
    f = weight(rho, alpha)
    return [np.where(rho != 0, np.asarray(c, dtype=np.float64) * f, 0.0) for c in (vx, vy, vz)]


def ngp_vec_grid(pos, vel, dens, N, L, assignment="ngp"):
    vec = orc.density_velocity_vector(vel.astype(np.float64), dens.astype(np.float64))
    if assignment != "ngp":
        return orc.deposit_assign(vec, pos, N, L, assignment)
    return orc.deposit_to_grid_fast(vec, pos, N, L) if len(pos) > 200_000 else orc.deposit_to_grid(vec, pos, N, L)


def ngp_fields(pos, vel, dens, N, L, alpha, assignment="ngp"):
    return fields_from_vec_grid(ngp_vec_grid(pos, vel, dens, N, L, assignment), alpha)


def nn_fields(pos, vel, dens, N, L, alpha):
    """Exact-NN resampling on the library lattice: w of the nearest particle."""
    ax = orc.lattice_axes_library(L, N)
    idx = orc.exact_nn_lattice(pos, ax, ax, ax)
    vec = orc.density_velocity_vector(vel.astype(np.float64), dens.astype(np.float64))[idx].reshape(N, N, N, 4)
    return fields_from_vec_grid(vec, alpha)


def slab_fields(pos, vel, dens, N, L, x0, nx, alpha):
    """[w_c][nx][N][N] float64 of the x-slab [x0, x0 + nx) of the NGP field (the oracle's cell rule)."""
    idx = orc.cell_index(pos, N, L)
    keep = (idx[:, 0] >= x0) & (idx[:, 0] < x0 + nx)
    idx = idx[keep]
    flat = ((idx[:, 0] - x0) * N + idx[:, 1]) * N + idx[:, 2]
    v64, d64 = vel[keep].astype(np.float64), dens[keep].astype(np.float64)
    n3 = nx * N * N
    rho = np.bincount(flat, weights=d64, minlength=n3)
    f = weight(rho, alpha - 1.0)
    return [(np.bincount(flat, weights=v64[:, c] * d64, minlength=n3) * f).reshape(nx, N, N) for c in range(3)]


def table(fields, L, N, flavour="library", kmin=None, kmax=None, kres=None, window=None):
    """(nbins, 4) [k, P 4 pi k^2, Psum, Nsample] of spctrm's layout; window: 'cic' / 'tsc' multiplies P by 1 / W^2."""
    P = orc.vector_power(fields[0], fields[1], fields[2], L, N)
    if window is not None:
        P = P * orc.window_inv2(N, window)
    return orc.spectrum_table(P, L, N, flavour, kmin, kmax, kres)


def helmholtz_tables(fields, L, N, **kw):
    """(total, compressive, solenoidal) through tests/helmholtz_ref.py."""
    return href.helmholtz_tables(fields[0], fields[1], fields[2], L, N, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# grids no host array can follow (2048^3): the SAME definition, the field kept as its occupied cells, the float64
# transform and the shell sums made one block at a time with torch as the calculator (as oracle/gpu_checks.py does)
# ---------------------------------------------------------------------------------------------------------------------
def sparse_cell_fields(pos, vel, dens, N, L, alpha):
    """(cells, [w_x, w_y, w_z]): the flat indices (ascending) of the NGP cells that hold particles (the oracle's cell rule)
    and the float64 w_c = (sum rho v_c) rho^(alpha - 1) of those cells; every other cell of the grid is 0."""
    idx = orc.cell_index(pos, N, L)
    flat = (idx[:, 0] * N + idx[:, 1]) * N + idx[:, 2]
    del idx
    cells, inv = np.unique(flat, return_inverse=True)
    inv = inv.ravel()
    d64 = dens.astype(np.float64)
    rho = np.bincount(inv, weights=d64, minlength=len(cells))
    f = weight(rho, alpha - 1.0)
    return cells, [np.bincount(inv, weights=vel[:, c].astype(np.float64) * d64, minlength=len(cells)) * f for c in range(3)]


def sparse_grid_shell_sums(device, cells, vals, N, L, k2_axis, thr, xrows=16, kzs=8):
    """Per-bin (Psum, counts), float64 / int64, of the vector field given by its occupied cells (sparse_cell_fields):
    P = 0.5 sum_c |a F_c|^2 with a = (L/2pi)^1.5 / N^3 (orc.vector_power) from a float64 transform -- rfft along z and fft along
    y of `xrows` x-planes at a time into ONE complex128 half spectrum, fft along x of `kzs` kz-planes at a time -- binned with
    the reference's rule restated as oracle/gpu_checks.py restates it: s = (k2x + k2y) + k2z in float64, bucketize(right=True)
    against the squared edges `thr`, Hermitian multiplicity 1 at kz = 0 and N/2, else 2.  torch on `device` is only the
    calculator (at 2048: 69 GB of spectrum + 34 GB of power)."""
    import torch
    h = N // 2
    nb = len(thr) - 1
    const = (L / (2 * np.pi)) ** 1.5 / N ** 3
    k2 = torch.as_tensor(np.asarray(k2_axis, dtype=np.float64)[:N].copy(), dtype=torch.float64, device=device)
    t = torch.as_tensor(np.asarray(thr, dtype=np.float64), dtype=torch.float64, device=device)
    cells_t = torch.as_tensor(np.asarray(cells, dtype=np.int64), device=device)
    xrows = min(xrows, N)
    assert N % xrows == 0
    bounds = np.searchsorted(cells, np.arange(0, N + 1, xrows, dtype=np.int64) * N * N)
    S = torch.empty((N, N, h + 1), dtype=torch.complex128, device=device)           # [x -> kx][ky][kz]
    P = torch.zeros((N, N, h + 1), dtype=torch.float64, device=device)
    for v in vals:
        vt = torch.as_tensor(np.asarray(v, dtype=np.float64), device=device)
        for i, x0 in enumerate(range(0, N, xrows)):
            lo, hi = int(bounds[i]), int(bounds[i + 1])
            slab = torch.zeros(xrows * N * N, dtype=torch.float64, device=device)
            slab[cells_t[lo:hi] - x0 * N * N] = vt[lo:hi]
            S[x0:x0 + xrows] = torch.fft.rfft2(slab.view(xrows, N, N))              # rfft along z, fft along y
            del slab
        for k0 in range(0, h + 1, kzs):
            T = torch.fft.fft(S[:, :, k0:k0 + kzs].contiguous(), dim=0)
            P[:, :, k0:k0 + kzs] += T.real.square() + T.imag.square()
            del T
        del vt
    del S
    SUB = 1024       # sub-bins per bin (gpu_checks.separable_shell_sums: many float64 adds to one address serialise)
    psum = torch.zeros((nb + 2) * SUB, dtype=torch.float64, device=device)
    counts = torch.zeros((nb + 2) * SUB, dtype=torch.int64, device=device)
    sxy = k2[:, None] + k2[None, :]                                                  # [kx, ky]: fl(k2x + k2y)
    for k0 in range(0, h + 1, kzs):
        kzt = torch.arange(k0, min(h + 1, k0 + kzs), device=device)
        s = sxy[:, :, None] + k2[kzt][None, None, :]
        mult = torch.where((kzt == 0) | (kzt == h), 1, 2)[None, None, :].expand(N, N, -1)
        b = torch.bucketize(s, t, right=True).reshape(-1)
        b = b * SUB + torch.arange(b.numel(), device=device) % SUB
        psum.index_add_(0, b, (P[:, :, k0:k0 + kzs] * mult * (0.5 * const * const)).reshape(-1))
        counts.index_add_(0, b, mult.reshape(-1))
        del s, b, mult
    psum = psum.view(nb + 2, SUB).sum(dim=1)
    counts = counts.view(nb + 2, SUB).sum(dim=1)
    return psum[1: nb + 1].cpu().numpy(), counts[1: nb + 1].cpu().numpy()
