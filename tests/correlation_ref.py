"""float64 numpy restatement of the two-point correlation function and of vps_fft_x modes 5 - 7 (include/vps_hip.h).

Nothing here imports the package: the lattice, the edges and the shell rule are written out again, so that the tests compare the
library against an independent statement.  TEST INFRASTRUCTURE ONLY.

  xi_grid            xi[rx][ry][rz] = <f(x) . f(x + r)> of real fields, by rfftn / irfftn
  xi_direct          the same by a direct sum over all pairs (small N)
  r_axis, default_edges, lattice_r
                     the lags r = Lcell min(i, N - i), the default edges j Lcell, and sqrt(s) of every lattice point with
                     s = (r2[a] + r2[b]) + r2[c] in the association of the binning x pass: a = the x-pass axis, c = the plane
  shells             numpy.histogram of the half lattice with Hermitian weights -> (sums, counts, absolute sums)
  correlation        the whole pipeline: (xi per shell, counts, xi0)
  line_transform, line_shells, line_power_full
                     line-level references of modes 6 / 7 and 5: numpy.fft.fft of the float32 input lines
"""
import numpy as np


def xi_grid(fields):
    out = 0.0
    for f in fields:
        f = np.asarray(f, dtype=np.float64)
        P = np.abs(np.fft.rfftn(f)) ** 2
        out = out + np.fft.irfftn(P, s=f.shape, axes=(0, 1, 2)) / f.size
    return out


def xi_direct(fields):
    N = np.asarray(fields[0]).shape[0]
    out = np.zeros((N, N, N))
    for f in fields:
        f = np.asarray(f, dtype=np.float64)
        for a in range(N):
            fa = np.roll(f, -a, axis=0)
            for b in range(N):
                fb = np.roll(fa, -b, axis=1)
                for c in range(N):
                    out[a, b, c] += np.mean(f * np.roll(fb, -c, axis=2))
    return out


def r_axis(L, N):
    Lcell = L / float(N)
    i = np.arange(N)
    return Lcell * np.minimum(i, N - i).astype(np.float64)


def default_edges(L, N):
    return (L / float(N)) * np.arange(N // 2 + 1)


def band_edges(L, N, rmin, rmax, rres):
    nb = int(np.floor((rmax - rmin) / rres + 1e-9))
    return rmin + rres * np.arange(nb + 1)


def lattice_r(L, N, planes=None):
    """sqrt(s) at [c][b][a] for the planes c (default 0 .. N/2): c the kz plane of the second transform (the lag along x of a
    field [x][y][z]), b its ky row, a the x-pass axis (the lag along z).  By the symmetry of the axis table it is also the lag
    length at xi[rx = c][ry = b][rz = a]."""
    r2 = r_axis(L, N) ** 2
    planes = np.arange(N // 2 + 1) if planes is None else np.asarray(planes)
    s = (r2[None, None, :] + r2[None, :, None]) + r2[planes][:, None, None]
    return np.sqrt(s)


def hermitian_weight(N, planes):
    planes = np.asarray(planes)
    return np.where((planes == 0) | (2 * planes == N), 1.0, 2.0)


def shells(r, values, w, edges):
    """numpy.histogram over the points r (any shape) with weights w (broadcast): -> (sum w v, sum w, sum w |v|) per shell."""
    w = np.broadcast_to(w, r.shape)
    rr = r.ravel()
    cnt = np.histogram(rr, edges, weights=w.ravel())[0]
    sm = np.histogram(rr, edges, weights=(w * values).ravel())[0]
    ab = np.histogram(rr, edges, weights=(w * np.abs(values)).ravel())[0]
    return sm, np.rint(cnt).astype(np.int64), ab


def correlation(fields, L, edges=None, subtract_mean=True):
    """-> (xi per shell [0 where a shell is empty], counts, xi0) of float32 or float64 real-space fields, all in float64."""
    fields = [np.asarray(f, dtype=np.float64) for f in fields]
    N = fields[0].shape[0]
    if subtract_mean:
        fields = [f - f.mean() for f in fields]
    edges = default_edges(L, N) if edges is None else edges
    xi = xi_grid(fields)
    planes = np.arange(N // 2 + 1)
    w = hermitian_weight(N, planes)[:, None, None]
    sm, cnt, _ = shells(lattice_r(L, N, planes), xi[: N // 2 + 1], w, edges)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(cnt > 0, sm / cnt, 0.0)
    return out, cnt, float(xi[0, 0, 0])


# ---- line level ----------------------------------------------------------------------------------------------------
def line_transform(lines):
    return np.fft.fft(np.asarray(lines).astype(np.complex128), axis=1)


def line_modes(N, nlines, line0, kz0):
    g = line0 + np.arange(nlines)
    return g % N, kz0 + g // N


def line_r(L, N, nlines, line0, kz0):
    ky, kz = line_modes(N, nlines, line0, kz0)
    r2 = r_axis(L, N) ** 2
    return np.sqrt((r2[None, :] + r2[ky][:, None]) + r2[kz][:, None])


def line_shells(F, r, N, nlines, line0, kz0, edges):
    """Modes 6 / 7 on transformed lines F [nlines][N] at the points r (line_r): (sum w Re F, sum w, sum w |Re F|) per shell."""
    _, kz = line_modes(N, nlines, line0, kz0)
    return shells(r, F.real, hermitian_weight(N, kz)[:, None], edges)


def line_power_full(F, N, nlines, line0, kz0, planes):
    """Mode 5 on transformed lines: what the call adds to the planes `planes` (a list of kz' indices of the full grid), as
    {kz': [N][N] float64}."""
    ky, kz = line_modes(N, nlines, line0, kz0)
    P = np.abs(F) ** 2
    out = {int(p): np.zeros((N, N)) for p in planes}
    mk = (N - np.arange(N)) % N
    for i in range(nlines):
        y, z = int(ky[i]), int(kz[i])
        if z in out:
            out[z][y] += P[i]
        if 0 < z < N // 2 and (N - z) in out:
            out[N - z][(N - y) % N][mk] += P[i]
    return out
