"""float64 reference of the second-moment quantities (VPS_TOTAL_ENERGY, VPS_SUBGRID_ENERGY, VPS_DISPERSION) and their spectra:
test infrastructure, never imported by the package.  Per cell, over the contributions (particle p, weight w) it receives,
    S2 = sum w rho_p |v_p|^2,   P = sum w rho_p v_p,   R = sum w rho_p
from the float32 inputs converted to float64, and with vol = Lcell^3
    total_energy = vol S2,   subgrid_energy = vol max(S2 - |P|^2 / R, 0),   dispersion = max(S2 / R - |P|^2 / R^2, 0)
all 0 where R = 0.  NGP: the oracle's cell rule in the dtype of the positions, w = 1.  CIC / TSC: the base cells of
tests/small_ref.py (the oracle's float64 rule) and the weights the accumulation kernel forms from a record's six words in float32
(tests/assign_direct_ref.py: record_words, weights_from_words), multiplied in float64.  The spectra go through
tests/density_ref.py's one-scalar table."""
import numpy as np

from oracle import vps_oracle as orc

import assign_direct_ref as adr
import density_ref as dref
import small_ref as sr

QUANTITIES = ("total_energy", "subgrid_energy", "dispersion")


def contributions(pos, N, L, assignment="ngp"):
    """(particle index [m], flat cell [m], weight float64 [m]) of every (particle, offset) pair with a non-zero weight; positions
    that are not finite contribute nowhere.  flat = (ix N + iy) N + iz."""
    pos = np.asarray(pos)
    keep = np.flatnonzero(np.all(np.isfinite(pos), axis=1))
    p = pos[keep]
    if assignment == "ngp":
        idx = orc.cell_index(p, N, L)
        return keep, (idx[:, 0] * N + idx[:, 1]) * N + idx[:, 2], np.ones(len(keep))
    order = sr.ORDER[assignment]
    c0, _ = sr.assign_weights(p, N, L, assignment)
    w = adr.weights_from_words(adr.record_words(p, N, L, assignment), assignment).astype(np.float64)
    who, flat, wt = [], [], []
    for jx in range(order):
        for jy in range(order):
            for jz in range(order):
                who.append(keep)
                flat.append((((c0[:, 0] + jx) % N) * N + (c0[:, 1] + jy) % N) * N + (c0[:, 2] + jz) % N)
                wt.append(w[:, 0, jx] * w[:, 1, jy] * w[:, 2, jz])
    who, flat, wt = np.concatenate(who), np.concatenate(flat), np.concatenate(wt)
    live = wt != 0
    return who[live], flat[live], wt[live]


def moments(pos, vel, rho, N, L, assignment="ngp", x0=0, nx=None):
    """{"S2", "R", "n": [nx, N, N]; "P": [3, nx, N, N]} float64 (n: the number of contributions, int64) on the rows
    [x0, x0 + nx) (default: the whole grid).  Every term of S2 is non-negative, so S2 is also the sum of the absolute terms that
    the per-cell bars are made of."""
    nx = N if nx is None else nx
    who, flat, wt = contributions(pos, N, L, assignment)
    ix = flat // (N * N)
    rows = (ix >= x0) & (ix < x0 + nx)
    who, flat, wt = who[rows], flat[rows] - x0 * N * N, wt[rows]
    v = np.asarray(vel, dtype=np.float64)[who]
    r = np.asarray(rho, dtype=np.float64)[who]
    cells = nx * N * N
    grid = lambda x: np.bincount(flat, weights=x, minlength=cells).reshape(nx, N, N)      # noqa: E731
    wr = wt * r
    return {"S2": grid(wr * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])),
            "P": np.stack([grid(wr * v[:, c]) for c in range(3)]), "R": grid(wr),
            "n": np.bincount(flat, minlength=cells).reshape(nx, N, N)}


def quantity(m, Lcell, name):
    """[N, N, N] float64 field of one of QUANTITIES from moments()."""
    vol = Lcell ** 3
    S2, R = m["S2"], m["R"]
    if name == "total_energy":
        return vol * S2
    has = R != 0
    Rs = np.where(has, R, 1.0)
    sub = np.maximum(S2 - (m["P"] ** 2).sum(axis=0) / Rs, 0.0)
    if name == "subgrid_energy":
        return np.where(has, vol * sub, 0.0)
    if name == "dispersion":
        return np.where(has, sub / Rs, 0.0)
    raise KeyError(name)


def resolved_energy(m, Lcell):
    """The field of VPS_ENERGY from the same moments: vol |P|^2 / R, 0 where R = 0."""
    has = m["R"] != 0
    return np.where(has, Lcell ** 3 * (m["P"] ** 2).sum(axis=0) / np.where(has, m["R"], 1.0), 0.0)


def table(field, L, N, window=None, flavour="library"):
    """(nbins, 4) [k, P 4 pi k^2, Psum, Nsample] of one of the fields (density_ref.table: one scalar)."""
    return dref.table(field, L, N, flavour=flavour, window=window)
