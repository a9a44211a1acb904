"""References of the velocity-gradient fields (VPS_DIVERGENCE, VPS_VORTICITY, VPS_STRAIN_RATE; include/vps_hip.h,
"Velocity-gradient fields") and of the sub-grid flux Pi = -tau_ij S_ij: test infrastructure, never imported by the package.

Two forms of the same second-order central differences on a periodic grid, d_a u_c (i) = (u_c(i + e_a) - u_c(i - e_a)) / (2 Lcell):
  *64   np.roll differences in float64: what the fields ARE;
  *32   float32 with the header's fixed order of operations -- h = float32(1 / (2 Lcell)) rounded once, (u(+) - u(-)) * h, the
        sums in the order written there: what the kernel computes, bit for bit where every step is exact (integer u, Lcell a
        power of two).
u: (3, N, N, N), component first, axes x, y, z."""
import numpy as np

CODES = {"divergence": 12, "vorticity": 13, "strain_rate": 14}
NCH = {"divergence": 1, "vorticity": 3, "strain_rate": 6}
TENSOR_ORDER = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))          # xx, yy, zz, xy, xz, yz


def layout(N, num_cu=256):
    """(xchunk, vec) of the launch of csrc/gradient.hip (gradient_launch_q): 16-byte groups of 4 cells where N % 4 == 0, else 2;
    tiles of 16 rows by 16 groups; enough x chunks for 16 workgroups per CU, but chunks of no less than 64 planes where N allows
    -- unlike the filter's (filter_ref.layout) a chunk has no longest length."""
    vec = 4 if N % 4 == 0 else 2
    tiles = -(-N // (16 * vec)) * -(-N // 16)
    nxc = max(1, min(-(-16 * num_cu // tiles), N // 64))
    return -(-N // nxc), vec


def derivatives64(u, Lcell):
    """d[c][a] = d u_c / d x_a, float64."""
    u = np.asarray(u, dtype=np.float64)
    return [[(np.roll(u[c], -1, axis=a) - np.roll(u[c], 1, axis=a)) / (2.0 * Lcell) for a in range(3)] for c in range(3)]


def derivatives32(u, Lcell):
    u = np.asarray(u, dtype=np.float32)
    h = np.float32(1.0 / (2.0 * float(Lcell)))
    return [[(np.roll(u[c], -1, axis=a) - np.roll(u[c], 1, axis=a)) * h for a in range(3)] for c in range(3)]


def _fields(d, what, half):
    if what == "divergence":
        return np.stack([(d[0][0] + d[1][1]) + d[2][2]])
    if what == "vorticity":
        return np.stack([d[2][1] - d[1][2], d[0][2] - d[2][0], d[1][0] - d[0][1]])
    if what == "strain_rate":
        return np.stack([d[0][0], d[1][1], d[2][2], half * (d[0][1] + d[1][0]), half * (d[0][2] + d[2][0]),
                         half * (d[1][2] + d[2][1])])
    raise ValueError(what)


def fields64(u, Lcell, what):
    """(NCH, N, N, N) float64."""
    return _fields(derivatives64(u, Lcell), what, 0.5)


def fields32(u, Lcell, what):
    """(NCH, N, N, N) float32, the kernel's order of operations."""
    out = _fields(derivatives32(u, Lcell), what, np.float32(0.5))
    assert out.dtype == np.float32
    return out


def gradient64(phi, Lcell):
    """The central-difference gradient of a scalar: (3, N, N, N)."""
    phi = np.asarray(phi, dtype=np.float64)
    return np.stack([(np.roll(phi, -1, axis=a) - np.roll(phi, 1, axis=a)) / (2.0 * Lcell) for a in range(3)])


def flux64(tau, S):
    """Pi = -(tau_xx S_xx + tau_yy S_yy + tau_zz S_zz + 2 tau_xy S_xy + 2 tau_xz S_xz + 2 tau_yz S_yz), float64, and the sum of
    the absolute terms sum_ij |tau_ij S_ij| (the scale of its rounding error)."""
    tau, S = np.asarray(tau, dtype=np.float64), np.asarray(S, dtype=np.float64)
    terms = [tau[c] * S[c] * (1.0 if c < 3 else 2.0) for c in range(6)]
    return -sum(terms), sum(np.abs(t) for t in terms)


def full_tensor(six):
    """[3][3] list of the fields of a symmetric tensor given as xx, yy, zz, xy, xz, yz."""
    t = [[None] * 3 for _ in range(3)]
    for c, (i, j) in enumerate(TENSOR_ORDER):
        t[i][j] = t[j][i] = six[c]
    return t


def fields32_all(u, Lcell):
    """{what: fields32(u, Lcell, what)} from one set of derivatives."""
    d = derivatives32(u, Lcell)
    return {what: _fields(d, what, np.float32(0.5)) for what in CODES}


def impulse_expect(what, c, p, A, Lcell, N):
    """The whole output for a velocity that is A in component c at cell p = (ix, iy, iz) and 0 elsewhere, as a dict
    {(channel, ix, iy, iz): float32 value} of its nonzero elements: d_a u_c is +A h at p - e_a and -A h at p + e_a (wrapped), and
    nothing else is nonzero -- the divergence sees the pair along c, the vorticity the two pairs across c, the strain rate all
    three.  N >= 3 (the two neighbours of an axis are distinct cells)."""
    h = np.float32(1.0 / (2.0 * float(Lcell)))
    A = np.float32(A)
    out = {}
    for a in range(3):
        if what == "divergence":
            if a != c:
                continue
            ch, f = 0, np.float32(1)
        elif what == "vorticity":
            if a == c:
                continue
            ch = 3 - a - c                                   # omega_ch = d_a u_c - d_c u_a for (ch, a, c) cyclic
            f = np.float32(1 if (ch, a, c) in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1)
        else:
            ch = c if a == c else TENSOR_ORDER.index((min(a, c), max(a, c)))
            f = np.float32(1 if a == c else 0.5)
        for step, sign in ((-1, 1), (1, -1)):
            q = list(p)
            q[a] = (q[a] + step) % N
            out[(ch,) + tuple(q)] = f * (np.float32(sign) * A * h)
    return out


def integer_velocity(N, seed, amp=1024):
    """(3, N, N, N) float32 of integers in [-amp, amp]: every difference, product with a power-of-two h and sum of three is exact."""
    rng = np.random.default_rng(seed)
    return rng.integers(-amp, amp + 1, size=(3, N, N, N)).astype(np.float32)


def error_bar(u, Lcell):
    """The bar of a float32 kernel against fields64: 16 * 2^-24 * max|u| / Lcell (derived in tests/test_gpu_gradient.py)."""
    return 16.0 * 2.0 ** -24 * float(np.abs(u).max()) / float(Lcell)
