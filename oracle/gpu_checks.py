"""Checkers for sizes no host array can follow (2048^3 float64 grids do not fit a host): size-independent properties
computed with torch float64 ON THE GPU AS A CALCULATOR -- no library call is involved in them.

Test infrastructure like the rest of oracle/: only tests/, bench.py's parity / check legs and smoke() import it; the
product path never does.  Each function restates the reference rule it follows (file:line under /root/reference).
"""
import numpy as np
import torch


def shell_counts_exact(device, N, k2_axis, thr):
    """Number of modes of the full N^3 spectrum per bin: np.histogram's rule thr[b] <= s < thr[b+1] applied to
    s = (k2x + k2y) + k2z in float64 with numpy's association (vpower/interp.py:1449-1462, 1474-1477; thr[] are the squared
    edges, vpower.device.sqrt_thresholds), counted on the |k| octant with multiplicities."""
    h = N // 2
    nb = len(thr) - 1
    k2 = torch.as_tensor(np.asarray(k2_axis)[: h + 1].copy(), dtype=torch.float64, device=device)
    t = torch.as_tensor(np.asarray(thr), dtype=torch.float64, device=device)
    w = torch.full((h + 1,), 2, dtype=torch.int64, device=device)
    w[0] = 1
    w[h] = 1
    counts = torch.zeros(nb + 2, dtype=torch.int64, device=device)
    wyz = (w[:, None] * w[None, :]).reshape(-1)
    for i in range(h + 1):
        s = ((k2[i] + k2[:, None]) + k2[None, :]).reshape(-1)
        b = torch.bucketize(s, t, right=True)            # 0: below thr[0]; nbins+1: >= thr[nbins]
        counts.index_add_(0, b, wyz * int(w[i]))
    return counts[1: nb + 1].cpu().numpy()


def ngp_moments_float64(dpos, dvel, drho, N, L, quantities, rows=128):
    """Per quantity the float64 sum and sum of squares of every component field of the NGP fields: a restatement of
    interp.py:1010-1013 (cell = (pos // Lcell) % N, scatter-add of [rho v, rho]) + 272-273 (v = rho v / rho, m = rho Lcell^3;
    empty cells 0, the rule of :329-331) + 523-525 (p = v m) + 546 (E = m |v|^2), in torch float64, one x-slab of `rows` planes
    at a time.  -> {quantity: [[sum, sum of squares] per component]}."""
    Lcell = L / N
    vol = Lcell ** 3
    lc = torch.tensor(Lcell, dtype=dpos.dtype, device=dpos.device)
    cx = (torch.floor_divide(dpos[:, 0], lc) % N).to(torch.int64)
    out = {q: [[0.0, 0.0] for _ in range(1 if q == "energy" else 3)] for q in quantities}
    for x0 in range(0, N, rows):
        sel = torch.nonzero((cx >= x0) & (cx < x0 + rows)).squeeze(1)
        p = dpos[sel]
        flat = ((cx[sel] - x0) * N + (torch.floor_divide(p[:, 1], lc) % N).to(torch.int64)) * N \
            + (torch.floor_divide(p[:, 2], lc) % N).to(torch.int64)
        del p
        d = drho[sel].double()
        n3 = rows * N * N
        rho = torch.zeros(n3, dtype=torch.float64, device=dpos.device).index_add_(0, flat, d)
        inv = torch.where(rho > 0, 1.0 / rho, torch.zeros_like(rho))
        v = []
        for c in range(3):
            a = torch.zeros(n3, dtype=torch.float64, device=dpos.device).index_add_(0, flat, d * dvel[sel, c].double())
            v.append(a * inv)
            del a
        m = rho * vol
        del rho, inv, flat, d, sel
        for q in quantities:
            if q == "velocity":
                fs = v
            elif q == "momentum":
                fs = [v[c] * m for c in range(3)]
            else:
                fs = [m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])]
            for c, f in enumerate(fs):
                out[q][c][0] += float(f.sum().item())
                out[q][c][1] += float((f * f).sum().item())
            del fs
        del v, m
    return out


def parseval_targets(moments, N):
    """sum over ALL modes except k = 0 of 0.5 |a F|^2 (2 pi / L)^3 = 0.5 sum_c (<f_c^2> - <f_c>^2): the Parseval statement of
    interp.py:1377-1378 / 1413-1414 with the k = 0 mode (which no shell holds) taken out."""
    return {q: sum(0.5 * (sq / N ** 3 - (s_ / N ** 3) ** 2) for s_, sq in comps) for q, comps in moments.items()}


def all_mode_k_range(N, L):
    """(kmin, kmax, kres) of a script-flavour binning whose shells reach the corners of the k cube: every mode but k = 0."""
    kmin = 2 * np.pi / L
    return kmin, (int(np.ceil(np.sqrt(3.0) * N / 2)) + 1) * kmin, kmin


# --------------------------------------------------------------------------- #
# Separable random fields: an exact reference spectrum at any N
# --------------------------------------------------------------------------- #
def separable_factors(N, rank=3, seed=0):
    """Factors (a, b, c), each [rank, N] float64, of the field f(x,y,z) = sum_r a_r(x) b_r(y) c_r(z).  Every factor is the
    inverse DFT of a Hermitian spectrum with random phases and magnitudes in [0.5, 1.5]: real, generic, and with no mode of
    any 1-D spectrum near zero, so that a few modes in a low shell carry a well-conditioned sum."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        spec = rng.uniform(0.5, 1.5, (rank, N)) * np.exp(2j * np.pi * rng.random((rank, N)))
        spec = 0.5 * (spec + np.conj(spec[:, (-np.arange(N)) % N]))   # Hermitian: the factor is real
        out.append(np.fft.ifft(spec, axis=1).real.copy())
    return tuple(out)


def _plane_rows(N, nx, budget=1 << 26):
    return max(1, min(nx, budget // (N * N)))


def separable_slab(device, factors, x0, nx):
    """The float32 x-slab f[x0:x0+nx, :, :] of the separable field `factors` (separable_factors) on `device`, computed in
    float64 a few planes at a time and rounded once: every element is within 2^-24 (relative) of the float64 field, far below
    every bar the field is checked against (1e-5 per mode, 2e-5 per shell)."""
    a, b, c = (torch.as_tensor(f, dtype=torch.float64, device=device) for f in factors)
    N = b.shape[1]
    bc = torch.einsum("ry,rz->ryz", b, c)                 # [rank, N, N]
    out = torch.empty((nx, N, N), dtype=torch.float32, device=device)
    step = _plane_rows(N, nx)
    for i in range(0, nx, step):
        j = min(nx, i + step)
        out[i:j] = torch.einsum("rx,ryz->xyz", a[:, x0 + i: x0 + j], bc).to(torch.float32)
    return out


def _separable_spectra(device, factors):
    """(A, B, C) = fft(a), fft(b), rfft(c) per rank term, numpy float64 DFTs moved to `device` as complex128."""
    a, b, c = factors
    return tuple(torch.as_tensor(s, dtype=torch.complex128, device=device)
                 for s in (np.fft.fft(a, axis=1), np.fft.fft(b, axis=1), np.fft.rfft(c, axis=1)))


def separable_plane(device, factors, kz, ky=None):
    """Exact spectrum plane F[ky][kx] (complex128 [N, N], numpy's sign convention) of the separable field at kz (0 <= kz <= N/2):
    F(kx, ky, kz) = sum_r A_r(kx) B_r(ky) C_r(kz).  kz: one plane, or a sequence of planes -> [len(kz), N, N]; ky: optional
    slice of the rows."""
    A, B, C = _separable_spectra(device, factors)
    if ky is not None:
        B = B[:, ky]
    if np.ndim(kz) == 0:
        return torch.einsum("r,ry,rx->yx", C[:, int(kz)], B, A)
    kzt = torch.as_tensor(np.asarray(kz, dtype=np.int64), device=device)
    return torch.einsum("rz,ry,rx->zyx", C[:, kzt], B, A)


def separable_shell_sums(device, comps, N, L, k2_axis, thr, kz=None, win=None, nyq_ky=None):
    """Per-bin (Psum, counts) of the half spectrum of the separable fields `comps` (a list of separable_factors, one per
    component), float64 / int64, the reference's binning restated exactly: P = sum over components of 0.5 |a F|^2 with
    a = (L/2pi)^1.5 / N^3 (orc.vector_power / orc.power_const), s = (k2x + k2y) + k2z in float64 with numpy's association and
    bucketize(right=True) against the squared edges `thr` (shell_counts_exact's rule), every kz plane weighted with its
    Hermitian multiplicity (1 at kz = 0 and N/2, else 2).  The spectrum is exact up to float64 rounding (products of float64
    1-D FFTs), so the sums are good to ~1e-13 relative at any N -- a 2048^3 spectrum never exists in memory: one block of kz
    planes at a time, torch on `device` only as the calculator.
    kz: optional subset of the planes 0..N/2 (one rank's share); win: optional 1/W^2 axis table (N entries, fftfreq order):
    every mode weighted with win[kx] win[ky] win[kz]; nyq_ky: optional (lo, hi) -- of the Nyquist plane kz = N/2 only the
    rows lo <= ky < hi (one rank's share of that plane)."""
    h = N // 2
    nb = len(thr) - 1
    const = (L / (2 * np.pi)) ** 1.5 / N ** 3
    k2 = torch.as_tensor(np.asarray(k2_axis, dtype=np.float64)[:N].copy(), dtype=torch.float64, device=device)
    t = torch.as_tensor(np.asarray(thr, dtype=np.float64), dtype=torch.float64, device=device)
    w = None if win is None else torch.as_tensor(np.asarray(win, dtype=np.float64), dtype=torch.float64, device=device)
    spectra = [_separable_spectra(device, f) for f in comps]
    planes = list(range(h + 1)) if kz is None else sorted(int(k) for k in kz)
    # accumulated into SUB sub-bins per bin (element i into sub-bin i % SUB): a few hundred bins take millions of float64 adds
    # per block, and on a GPU so many atomic adds to one address serialise
    SUB = 1024
    psum = torch.zeros((nb + 2) * SUB, dtype=torch.float64, device=device)
    counts = torch.zeros((nb + 2) * SUB, dtype=torch.int64, device=device)
    sxy = k2[None, :] + k2[:, None]                       # [ky, kx]: fl(k2x + k2y)
    wxy = None if w is None else w[:, None] * w[None, :]
    step = _plane_rows(N, len(planes), 1 << 24)
    for i in range(0, len(planes), step):
        blk = planes[i:i + step]
        kzt = torch.as_tensor(blk, dtype=torch.int64, device=device)
        P = torch.zeros((len(blk), N, N), dtype=torch.float64, device=device)
        for A, B, C in spectra:
            P += (const * torch.einsum("rz,ry,rx->zyx", C[:, kzt], B, A)).abs().square()
        P *= 0.5
        if w is not None:
            P *= wxy[None] * w[kzt][:, None, None]
        s = sxy[None] + k2[kzt][:, None, None]
        mult = torch.where((kzt == 0) | (kzt == h), 1, 2)[:, None, None].expand(-1, N, N)
        if nyq_ky is not None:
            rows = torch.arange(N, device=device)
            off = (kzt == h)[:, None] & ((rows < nyq_ky[0]) | (rows >= nyq_ky[1]))[None, :]
            mult = torch.where(off[:, :, None], 0, mult)
        b = torch.bucketize(s, t, right=True).reshape(-1)   # 0: below thr[0]; nb + 1: >= thr[nb]
        b = b * SUB + torch.arange(b.numel(), device=device) % SUB
        psum.index_add_(0, b, (P * mult).reshape(-1))
        counts.index_add_(0, b, mult.reshape(-1))
        del P, s, b, mult
    psum = psum.view(nb + 2, SUB).sum(dim=1)
    counts = counts.view(nb + 2, SUB).sum(dim=1)
    return psum[1: nb + 1].cpu().numpy(), counts[1: nb + 1].cpu().numpy()
