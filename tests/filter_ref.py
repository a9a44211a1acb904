"""numpy reference of the box-filter codes (VPS_FILTERED_VM = 16, VPS_FILTERED_STRESS = 17; include/vps_hip.h, "Box-filtered
fields"): test infrastructure, never imported by the package.  chans [4, N, N, N] = u_x, u_y, u_z, mass; W(i) the periodic box of
(2m+1)^3 cells around cell i; per cell p_c = mass u_c, s_ij = p_i u_j; M, P_c, S_ij their box sums; c = 1 / (2m+1)^3:
    vm      u~_c = P_c / M , mbar = M c (both 0 where the box holds no cell with mass)
    stress  tau_ij = (S_ij - P_i P_j / M) c, the diagonals clamped at 0 from below first, all six 0 in such a box
in the order xx, yy, zz, xy, xz, yz."""
import numpy as np

CODES = {"vm": 16, "stress": 17}
NCH = {"vm": 4, "stress": 6}
IJ = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
EPS = 2.0 ** -24            # one float32 rounding, relative
XCHUNK_MAX = 64             # the longest x chunk of csrc/filter.hip


def layout(N, num_cu=256):
    """(xchunk, vec) of the launch of csrc/filter.hip: 16-byte groups of 4 cells where N % 4 == 0, else 2; x chunks of at most
    64 planes, enough of them for 16 workgroups per CU, but of no less than 32 planes where N allows."""
    vec = 4 if N % 4 == 0 else 2
    tiles = -(-N // (16 * vec)) * -(-N // 16)
    lo = -(-N // XCHUNK_MAX)
    hi = max(lo, N // 32)
    nxc = max(lo, min(-(-16 * num_cu // tiles), hi))
    return -(-N // nxc), vec


def chain_max(a, xchunk, vec):
    """max of a[..., x', y, z'] over x' <= x inside the x chunk of x and z' <= z inside the group of `vec` cells of z: the
    window sums a sliding sum has passed through when it is written at (x, y, z)."""
    a = np.asarray(a, dtype=np.float64)
    N = a.shape[-1]
    out = np.maximum.accumulate(a.reshape(a.shape[:-1] + (N // vec, vec)), axis=-1).reshape(a.shape)
    for xs in range(0, a.shape[-3], xchunk):
        out[..., xs:xs + xchunk, :, :] = np.maximum.accumulate(out[..., xs:xs + xchunk, :, :], axis=-3)
    return out


def count(chans, m):
    """[N, N, N] int64: the cells with mass != 0 in the box -- 0 is what "the box holds no mass" means, exactly."""
    return box_sum((np.asarray(chans)[3] != 0).astype(np.int64), m)


def chain(m):
    """K of csrc/filter.hip: the longest chain of roundings in one box sum -- 2 in a product, 2m + 6 along z (direct sum, then
    three sliding steps), 2m + 2 * 63 along x (direct sum at the chunk's start, then two per plane), 2m along y."""
    return 6 * m + 134


def box_sum(a, m):
    """Periodic box sum over (2m+1)^3 cells of the last three axes, in the dtype of `a` (float64 for the references)."""
    out = np.asarray(a)
    if out.ndim > 3:                                   # (one field at a time: the cumulative sums of a 250^3 grid are large)
        return np.stack([box_sum(x, m) for x in out])
    for ax in range(3):
        n = out.shape[ax]
        sl = lambda a, b: tuple(slice(a, b) if k == ax else slice(None) for k in range(3))      # noqa: E731
        cs = np.cumsum(np.concatenate([out[sl(n - m, n)], out, out[sl(0, m)]], axis=ax), axis=ax)
        out = cs[sl(2 * m, n + 2 * m)].copy()                        # cs[i + 2m] - cs[i - 1], cs[-1] = 0
        out[sl(1, n)] -= cs[sl(0, n - 1)]
    return out


def terms(chans, dtype=np.float64):
    """[10, N, N, N]: mass, p_x, p_y, p_z, s_xx, s_yy, s_zz, s_xy, s_xz, s_yz per cell, every product rounded to `dtype`."""
    ch = np.asarray(chans, dtype=dtype)
    u, ms = ch[:3], ch[3]
    p = [(ms * u[c]).astype(dtype) for c in range(3)]
    return np.stack([ms] + p + [(p[i] * u[j]).astype(dtype) for i, j in IJ])


def sums64(chans, m):
    """(sums [10, N, N, N], abs [10, N, N, N]) float64: the box sums of the float32 kernel's terms (the products as float32
    forms them would differ by roundings the bars count; here they are exact float64 products of the float32 inputs) and the box
    sums of their absolute values, which the error bars are made of."""
    t = terms(np.asarray(chans, dtype=np.float32), np.float64)
    return box_sum(t, m), box_sum(np.abs(t), m)


def fields64(chans, m, what):
    s, _ = sums64(chans, m)
    return _form(s, m, what, np.float64, count(chans, m) != 0)


def _form(s, m, what, dtype, has):
    """has: where the box holds mass (from the integer count: a float sum of cumulative differences may keep a residue)."""
    c = dtype(np.float32(1.0 / (2 * m + 1) ** 3)) if dtype is np.float32 else 1.0 / (2 * m + 1) ** 3
    M = s[0]
    Ms = np.where(has, M, dtype(1))
    zero = dtype(0)
    if what == "vm":
        return np.stack([np.where(has, (s[1 + a] / Ms).astype(dtype), zero) for a in range(3)] + [np.where(has, (M * c).astype(dtype), zero)])
    out = []
    for k, (i, j) in enumerate(IJ):
        q = ((s[1 + i] * s[1 + j]).astype(dtype) / Ms).astype(dtype)
        t = (s[4 + k] - q).astype(dtype)
        if i == j:
            t = np.maximum(t, zero)
        out.append(np.where(has, (t * c).astype(dtype), zero))
    return np.stack(out)


def fields32(chans, m, what):
    """The float32 mirror for EXACT inputs (integer velocities and masses, every sum below 2^24, so that the order of the
    additions does not matter): each of product, division, subtraction, clamp and multiplication by c = (float32)(1 / (2m+1)^3)
    rounded to float32 in the header's order."""
    t = terms(chans, np.float32)
    s = box_sum(t.astype(np.float64), m)
    assert np.abs(box_sum(np.abs(t).astype(np.float64), m)).max() < 2 ** 24, "the sums must be exact in float32"
    return _form(s.astype(np.float32), m, what, np.float32, count(chans, m) != 0)


def fields32_all(chans, m):
    """{what: fields32(chans, m, what)} from ONE set of box sums."""
    t = terms(chans, np.float32)
    assert 2.0 * 9.0 * (2 * m + 1) ** 3 < 2 ** 24 and np.abs(t).max() <= 18, "the sums must be exact in float32"
    s = np.stack([box_sum(x.astype(np.int32), m).astype(np.float32) for x in t])          # (integers: exact, and half the bytes)
    has = count(chans, m) != 0
    return {what: _form(s, m, what, np.float32, has) for what in CODES}


def bars(chans, m, what, num_cu=256, extra=0):
    """Per-cell error bars of the float32 kernel against fields64.  K = chain(m) + extra (extra: roundings the caller's inputs
    already carry), e = 2^-24, A_X = sum_W |terms of X| and A^_X = chain_max(A_X) over the launch's x chunk and z group
    (layout(N, num_cu)): a rounding of a sliding sum is relative to the window sum it is made at, so
      |dX| <= K e A^_X   for X = M (A_M = M: mass >= 0), P_c, S_ij
    and with rel = |dM| / M, carried through the operations of the header, each with its own rounding:
      mbar = M c       (|dM| + 2 e M) c                                      c's rounding and the product's
      u~ = P / M       E + e (|P| / M + E),  E = (|dP| + |P| rel) / (M (1 - rel))
      X = P_i P_j      dX = D + e (|X| + D),  D = |dP_i| |P_j| + |dP_j| |P_i| + |dP_i| |dP_j|
      Q = X / M        EQ = Q0 + e (|X| / M + Q0),  Q0 = (dX + |X| rel) / (M (1 - rel))
      tau = (S - Q) c  c (E + 3 e (|S - Q| + E)),  E = |dS| + EQ              subtraction, c's rounding, the product's
    The clamp of a diagonal moves the result towards the true value.  Where rel >= 1/2 the kernel's M may be off by more than half
    of itself and nothing is claimed of a quotient: the bar is inf there (the mass bar stays finite).  In a box without mass
    every output is exactly 0: the bar is 0."""
    ch = np.asarray(chans, dtype=np.float32)
    N = ch.shape[-1]
    s, a = sums64(ch, m)
    xchunk, vec = layout(N, num_cu)
    K, c = chain(m) + extra, 1.0 / (2 * m + 1) ** 3
    has = count(ch, m) != 0
    M = np.where(has, s[0], 1.0)
    d = K * EPS * chain_max(a, xchunk, vec)                              # |dX| of the ten sums
    rel = np.where(has, d[0] / M, 0.0)
    ok = rel < 0.5
    den = M * np.where(ok, 1.0 - rel, 1.0)
    if what == "vm":
        b = []
        for k in range(3):
            P = np.abs(s[1 + k])
            E = (d[1 + k] + P * rel) / den
            b.append(np.where(ok, E + EPS * (P / M + E), np.inf))
        b.append((d[0] + 2 * EPS * s[0]) * c)
    else:
        b = []
        for k, (i, j) in enumerate(IJ):
            Pi, Pj = np.abs(s[1 + i]), np.abs(s[1 + j])
            X = Pi * Pj
            D = d[1 + i] * Pj + d[1 + j] * Pi + d[1 + i] * d[1 + j]
            dX = D + EPS * (X + D)
            Q0 = (dX + X * rel) / den
            EQ = Q0 + EPS * (X / M + Q0)
            E = d[4 + k] + EQ
            b.append(np.where(ok, c * (E + 3 * EPS * (np.abs(s[4 + k] - s[1 + i] * s[1 + j] / M) + E)), np.inf))
    return np.where(has, np.stack(b), 0.0)


def integer_chans(N, seed, holes=True):
    """Exact inputs: integer velocities |u| <= 3, masses in {0, 1, 2}; with `holes`, slabs of empty cells wide enough that whole
    boxes (up to m = 8 where N allows) hold no mass, so that the M = 0 path runs."""
    rng = np.random.default_rng(seed)
    ch = np.empty((4, N, N, N), dtype=np.float32)
    ch[:3] = rng.integers(-3, 4, (3, N, N, N))
    ch[3] = rng.integers(0, 3, (N, N, N))
    if holes:
        h = min(N - 1, 19)
        ch[3, :h, :h, :h] = 0
    return ch


def impulse_expect(p, m, N):
    """The cells of the wrapped box of half-width m around p: where the filtered field of a unit-mass impulse at p is nonzero."""
    r = np.arange(-m, m + 1)
    ix, iy, iz = np.meshgrid((p[0] + r) % N, (p[1] + r) % N, (p[2] + r) % N, indexing="ij")
    mask = np.zeros((N, N, N), dtype=bool)
    mask[ix, iy, iz] = True
    return mask
