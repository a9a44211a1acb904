"""float64 references of the Helmholtz decomposition of a vector field's power spectrum (BoxField.helmholtz_spctrm,
vps_fft_x_bin_helmholtz): test infrastructure, never imported by the package.

For components f_c with F_c = numpy's full complex fftn(f_c) and k'_i = fftfreq(N) * N on every axis with the Nyquist entry
(index N/2) set to 0, per mode:
    P_tot  = 0.5 |a|^2 sum_c |F_c|^2                 (exactly what spctrm bins)
    P_comp = 0.5 |a|^2 |sum_c k'_c F_c|^2 / |k'|^2    (0 where k' = 0)
    P_sol  = P_tot - P_comp
binned with the oracle's own shell rule (oracle/vps_oracle.py: spectrum_table); the solenoidal table is the float64
difference of the two shell sums."""
import numpy as np
import torch

from oracle import vps_oracle as orc


def kprime(N):
    """Integer mode numbers of one axis, fftfreq order, with the Nyquist entry set to 0 (odd under k -> -k)."""
    k = np.fft.fftfreq(N) * N
    if N % 2 == 0:
        k[N // 2] = 0.0
    return k


def helmholtz_power(fx, fy, fz, Lbox, N):
    """(P_tot, P_comp) on the full N^3 grid, float64 (numpy fftn)."""
    a = orc.power_const(Lbox, N)
    F = [np.fft.fftn(np.asarray(f, dtype=np.float64)) * a for f in (fx, fy, fz)]
    kx, ky, kz = np.meshgrid(kprime(N), kprime(N), kprime(N), indexing="ij")
    D = kx * F[0] + ky * F[1] + kz * F[2]
    k2 = kx * kx + ky * ky + kz * kz
    with np.errstate(invalid="ignore", divide="ignore"):
        comp = np.where(k2 > 0, 0.5 * np.abs(D) ** 2 / np.where(k2 > 0, k2, 1.0), 0.0)
    tot = 0.5 * sum(np.abs(f) ** 2 for f in F)
    return tot, comp


def _derived(tab_tot, psum, flavour):
    ns = tab_tot[:, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        P = psum / ns
    if flavour == "library":
        P[ns == 0] = 0
    P = P * 4 * np.pi * tab_tot[:, 0] ** 2
    return np.column_stack((tab_tot[:, 0], P, psum, ns))


def helmholtz_tables(fx, fy, fz, Lbox, N, flavour="library", kmin=None, kmax=None, kres=None):
    """(total, compressive, solenoidal) (nbins, 4) tables [k, P * 4 pi k^2, Psum, Nsample] of spctrm's layout."""
    tot, comp = helmholtz_power(fx, fy, fz, Lbox, N)
    t_tot = orc.spectrum_table(tot, Lbox, N, flavour, kmin, kmax, kres)
    t_comp = orc.spectrum_table(comp, Lbox, N, flavour, kmin, kmax, kres)
    return t_tot, t_comp, _derived(t_tot, t_tot[:, 2] - t_comp[:, 2], flavour)


def half_spectrum_sums(fx, fy, fz, Lbox, N, edges):
    """Shell sums (tot, comp, counts) from the rfftn half spectrum kz <= N/2 with the Hermitian multiplicities
    (orc.bin_half_spectrum): the property the binning x pass relies on."""
    a = orc.power_const(Lbox, N)
    F = [np.fft.rfftn(np.asarray(f, dtype=np.float64)) * a for f in (fx, fy, fz)]
    kp = kprime(N)
    kx, ky, kz = np.meshgrid(kp, kp, kp[: N // 2 + 1], indexing="ij")
    kz = np.abs(kz)      # kz = N/2 -> 0 already; the rest are 0..N/2-1
    D = kx * F[0] + ky * F[1] + kz * F[2]
    k2 = kx * kx + ky * ky + kz * kz
    comp = np.where(k2 > 0, 0.5 * np.abs(D) ** 2 / np.where(k2 > 0, k2, 1.0), 0.0)
    tot = 0.5 * sum(np.abs(f) ** 2 for f in F)
    ps_t, ns = orc.bin_half_spectrum(tot, Lbox, N, edges)
    ps_c, _ = orc.bin_half_spectrum(comp, Lbox, N, edges)
    return ps_t, ps_c, ns


def spectral_fields(N, kind, seed=0):
    """Three real float64 fields built in k space: kind 'gradient' (F = i k' phi_hat: curl-free) or 'curl'
    (F = i k' x A_hat: divergence-free).  k' is odd, the potentials' spectra Hermitian, so the fields are real."""
    rng = np.random.default_rng(seed)
    kx, ky, kz = np.meshgrid(kprime(N), kprime(N), kprime(N), indexing="ij")
    if kind == "gradient":
        ph = np.fft.fftn(rng.standard_normal((N, N, N)))
        F = [1j * kx * ph, 1j * ky * ph, 1j * kz * ph]
    elif kind == "curl":
        A = [np.fft.fftn(rng.standard_normal((N, N, N))) for _ in range(3)]
        F = [1j * (ky * A[2] - kz * A[1]), 1j * (kz * A[0] - kx * A[2]), 1j * (kx * A[1] - ky * A[0])]
    else:
        raise ValueError(kind)
    return [np.fft.ifftn(f).real for f in F]


# ---------------------------------------------------------------------------------------------------------------------
# separable fields (oracle/gpu_checks.py: separable_factors): an exact reference at any N, the FULL spectrum plane by plane
# ---------------------------------------------------------------------------------------------------------------------
def separable_helmholtz_sums(device, comps, N, L, k2_axis, thr, win=None, budget=1 << 24):
    """Per-bin (Psum_tot, Psum_comp, counts) of the three separable fields `comps` (three separable_factors), float64 /
    int64: every kz plane 0..N-1 of the FULL spectrum F_c(kx, ky, kz) = sum_r A_r(kx) B_r(ky) C_r(kz) (float64 1-D FFTs),
    no Hermitian logic, binned by s = (k2x + k2y) + k2z in float64 against the squared edges `thr` (bucketize right=True,
    gpu_checks.shell_counts_exact's rule); win: optional 1/W^2 axis table, every mode weighted with win[kx] win[ky] win[kz].
    torch on `device` is only the calculator (a 2048^3 spectrum never exists in memory)."""
    assert len(comps) == 3
    nb = len(thr) - 1
    const = (L / (2 * np.pi)) ** 1.5 / N ** 3
    k2 = torch.as_tensor(np.asarray(k2_axis, dtype=np.float64)[:N].copy(), dtype=torch.float64, device=device)
    t = torch.as_tensor(np.asarray(thr, dtype=np.float64), dtype=torch.float64, device=device)
    kp = torch.as_tensor(kprime(N), dtype=torch.float64, device=device)
    w = None if win is None else torch.as_tensor(np.asarray(win, dtype=np.float64), dtype=torch.float64, device=device)
    spectra = [tuple(torch.as_tensor(np.fft.fft(f, axis=1), dtype=torch.complex128, device=device) for f in fac)
               for fac in comps]
    SUB = 1024     # sub-bins per bin (element i into sub-bin i % SUB): many float64 index_adds to one address serialise
    ps_t = torch.zeros((nb + 2) * SUB, dtype=torch.float64, device=device)
    ps_c = torch.zeros((nb + 2) * SUB, dtype=torch.float64, device=device)
    counts = torch.zeros((nb + 2) * SUB, dtype=torch.int64, device=device)
    sxy = k2[None, :] + k2[:, None]                         # [ky, kx]: fl(k2x + k2y)
    kxy2 = kp[None, :] ** 2 + kp[:, None] ** 2
    wxy = None if w is None else w[:, None] * w[None, :]
    step = max(1, min(N, budget // (N * N)))
    for z0 in range(0, N, step):
        kzt = torch.arange(z0, min(N, z0 + step), device=device)
        F = [torch.einsum("rz,ry,rx->zyx", C[:, kzt], B, A) * const for A, B, C in spectra]
        P = 0.5 * sum(f.abs().square() for f in F)
        D = kp[None, None, :] * F[0] + kp[None, :, None] * F[1] + kp[kzt][:, None, None] * F[2]
        del F
        kk = kxy2[None] + (kp[kzt] ** 2)[:, None, None]
        Pc = torch.where(kk > 0, 0.5 * D.abs().square() / torch.where(kk > 0, kk, torch.ones_like(kk)), torch.zeros_like(kk))
        del D, kk
        if w is not None:
            f = wxy[None] * w[kzt][:, None, None]
            P *= f
            Pc *= f
        s = sxy[None] + k2[kzt][:, None, None]
        b = torch.bucketize(s, t, right=True).reshape(-1)
        b = b * SUB + torch.arange(b.numel(), device=device) % SUB
        ps_t.index_add_(0, b, P.reshape(-1))
        ps_c.index_add_(0, b, Pc.reshape(-1))
        counts.index_add_(0, b, torch.ones_like(b))
        del P, Pc, s, b
    out = [x.view(nb + 2, SUB).sum(dim=1)[1: nb + 1].cpu().numpy() for x in (ps_t, ps_c, counts)]
    return out[0], out[1], out[2]
