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


def ngp_fields_float64(rho, rv, vol, quantities):
    """float64 fields of the NGP cell totals rho = sum rho_p and rv[c] = sum rho_p v_pc: interp.py:272-273 (v = rho v / rho,
    m = rho Lcell^3; empty cells 0, the rule of :329-331) + 523-525 (p = v m) + 546 (E = m |v|^2); "mass": m alone.
    -> {quantity: [component fields]} in the shape of rho."""
    inv = torch.where(rho > 0, 1.0 / rho, torch.zeros_like(rho))
    v = [a * inv for a in rv]
    m = rho * vol
    out = {}
    for q in quantities:
        if q == "velocity":
            out[q] = v
        elif q == "momentum":
            out[q] = [v[c] * m for c in range(3)]
        elif q == "mass":
            out[q] = [m]
        else:
            out[q] = [m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])]
    return out


def slab_sums(cells, payloads, N, x0, rows, dtype=torch.int64):
    """Per payload (a tensor [np]) the scatter-add over the cells [np, 3] that lie in the x-rows [x0, x0 + rows): flat
    tensors of rows * N * N entries, cell (x, y, z) at ((x - x0) N + y) N + z.  dtype int64 with integer payloads is the EXACT
    NGP deposit (an integer histogram, interp.py:1013 without rounding); float64 is the reference of real-valued data."""
    cx = cells[:, 0]
    sel = torch.nonzero((cx >= x0) & (cx < x0 + rows)).squeeze(1)
    c = cells[sel].to(torch.int64)
    flat = ((c[:, 0] - x0) * N + c[:, 1]) * N + c[:, 2]
    del c
    n3 = rows * N * N
    return [torch.zeros(n3, dtype=dtype, device=cells.device).index_add_(0, flat, p[sel].to(dtype)) for p in payloads]


def exact_slab_reference(cells, rho, vel, N, x0, rows, payload=None):
    """int64 cell totals of the rows [x0, x0 + rows): [sum rho, sum rho vx, sum rho vy, sum rho vz] of integer-valued rho, vel
    -- or, payload [np, C] given, of its C integer columns."""
    if payload is not None:
        return slab_sums(cells, [payload[:, c] for c in range(payload.shape[1])], N, x0, rows)
    r = rho.to(torch.int64)
    return slab_sums(cells, [r] + [r * vel[:, c].to(torch.int64) for c in range(3)], N, x0, rows)


def float64_slab_fields(cells, rho, vel, N, L, x0, rows, quantities):
    """{quantity: [float64 component fields, flat rows * N * N]} of real-valued particles whose cells are known."""
    d = rho.double()
    sums = slab_sums(cells, [d] + [d * vel[:, c].double() for c in range(3)], N, x0, rows, torch.float64)
    return ngp_fields_float64(sums[0], sums[1:], (L / N) ** 3, quantities)


def ngp_moments_float64(dpos, dvel, drho, N, L, quantities, rows=128):
    """Per quantity the float64 sum and sum of squares of every component field of the NGP fields: a restatement of
    interp.py:1010-1013 (cell = (pos // Lcell) % N, scatter-add of [rho v, rho]) + the field rules of ngp_fields_float64, in
    torch float64, one x-slab of `rows` planes at a time.  -> {quantity: [[sum, sum of squares] per component]}."""
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
        rv = [torch.zeros(n3, dtype=torch.float64, device=dpos.device).index_add_(0, flat, d * dvel[sel, c].double())
              for c in range(3)]
        del flat, d, sel
        fields = ngp_fields_float64(rho, rv, vol, quantities)
        del rho, rv
        for q in quantities:
            for c, f in enumerate(fields[q]):
                out[q][c][0] += float(f.sum().item())
                out[q][c][1] += float((f * f).sum().item())
        del fields
    return out


# --------------------------------------------------------------------------- #
# Constructed particles: the cell of every particle is known before any position exists
# --------------------------------------------------------------------------- #
DISTRIBUTIONS = ("uniform", "clump", "half_empty", "ends")
CELL_SUM_CAP = 1 << 12      # no cell total |sum rho v_c| may pass it: float32 sums stay exact, z transforms far below 0.25
CLUMP_PER_CELL = 400        # 400 particles x (rho <= 3) x (|v| <= 3) = 3600: room for ~50 background particles per cell
ENDS_CELLS = 32             # "ends": 2 x 16 cells (y, z) of the first and of the last bucket


def ends_count(n, per_cell=CLUMP_PER_CELL):
    """Particles the "ends" distribution can hold under CELL_SUM_CAP (2 * ENDS_CELLS cells, per_cell each)."""
    return min(int(n), 2 * ENDS_CELLS * per_cell)


# (N, box length, position dtype) of every leg of tests/test_gpu_gridding_matrix.py; tests/test_gridding_reference_cpu.py checks
# the constructed cells against the oracle at each of them
GRIDDING_MATRIX = ((48, 1.0, "float32"), (96, 2.5, "float32"), (250, 2.5, "float32"), (384, 1.0, "float64"),
                   (500, 1.0, "float32"), (512, 1.0, "float32"), (512, 1.0, "float64"), (768, 2.5, "float64"),
                   (1024, 1.0, "float64"), (2048, 1.0, "float32"), (4096, 1.0, "float32"))


def matrix_geometry(N, dtype=None):
    """(L, torch dtype) of the matrix's legs at N (the first entry of GRIDDING_MATRIX, or the one with `dtype`)."""
    for n, L, dt in GRIDDING_MATRIX:
        if n == N and dtype in (None, dt):
            return L, getattr(torch, dt)
    raise KeyError((N, dtype))


def constructed_particles(device, n, N, L, dtype=torch.float32, dist="uniform", seed=0, wrap=1.0 / 16, chunk=1 << 24,
                          per_cell=CLUMP_PER_CELL):
    """-> (cells int32 [n, 3], pos `dtype` [n, 3], rho float32 [n], vel float32 [n, 3]) on `device`, made a chunk at a time.
    rho is an integer in 1..3, every vel component one in -3..3.  A position is (cell + offset) Lcell + k L in float64, rounded
    once to `dtype`, with offset in [0.25, 0.75] per axis: the rounding (|pos| <= 3 L: below 2^-11 cells in float32 at
    N = 4096) and the float32 quotient pos // fl(Lcell) (below 1e-3 cells off for any N, L) stay far inside the cell, so that
    (pos // Lcell) % N is `cells` BY CONSTRUCTION (tests/test_gridding_reference_cpu.py checks every particle against the
    oracle).  k = 0, except for a share `wrap` of the particles: k in {-2, -1, 1, 2}, positions outside [0, L) whose stored
    cell is the wrapped one.
    dist: "uniform"; "clump": 30 % of the particles (at most CLUMP_PER_CELL per cell, dealt out evenly) in the 2 x 16 x N
    cells at x = N/3, y = 16 floor(N/48) -- a handful of pencils / bricks -- over a uniform background; "half_empty": uniform in
    x < N/2 only; "ends": only the cells x = 0, y < 2, z < 16 and x = N - 1, y >= N - 2, z >= N - 16, dealt out evenly
    (n <= ends_count(n)).  per_cell: the clump's / the ends' particles per cell (above CLUMP_PER_CELL the cap no longer
    holds: for checks of the positions alone)."""
    if dist not in DISTRIBUTIONS:
        raise ValueError(dist)
    if dist == "ends" and n > ends_count(n, per_cell):
        raise ValueError("ends: at most %d particles" % ends_count(n, per_cell))
    if dist in ("clump", "ends") and N < 48:
        raise ValueError("N >= 48")
    cells = torch.empty((n, 3), dtype=torch.int32, device=device)
    pos = torch.empty((n, 3), dtype=dtype, device=device)
    rho = torch.empty((n,), dtype=torch.float32, device=device)
    vel = torch.empty((n, 3), dtype=torch.float32, device=device)
    ncl = 2 * 16 * N
    nclump = min(int(0.3 * n), per_cell * ncl) if dist == "clump" else 0
    cx0, cy0 = N // 3, (N // 48) * 16
    Lcell = L / N
    for k, i0 in enumerate(range(0, n, chunk)):
        i1 = min(n, i0 + chunk)
        m = i1 - i0
        g = torch.Generator(device=device)
        g.manual_seed(1000003 * seed + k)
        c = torch.randint(0, N, (m, 3), generator=g, device=device, dtype=torch.int64)
        if dist == "half_empty":
            c[:, 0] = torch.randint(0, N // 2, (m,), generator=g, device=device, dtype=torch.int64)
        elif dist == "clump" and i0 < nclump:
            j = torch.arange(i0, min(i1, nclump), device=device, dtype=torch.int64) % ncl
            c[: j.numel()] = torch.stack((cx0 + j // (16 * N), cy0 + (j // N) % 16, j % N), dim=1)
        elif dist == "ends":
            i = torch.arange(i0, i1, device=device, dtype=torch.int64)
            j = (i // 2) % ENDS_CELLS
            last = (i % 2) == 1
            c = torch.stack((torch.where(last, N - 1, 0), torch.where(last, N - 2, 0) + j // 16,
                             torch.where(last, N - 16, 0) + j % 16), dim=1)
        off = 0.25 + 0.5 * torch.rand((m, 3), generator=g, device=device, dtype=torch.float64)
        shift = torch.zeros((m, 3), dtype=torch.float64, device=device)
        if wrap > 0:
            kk = torch.randint(0, 4, (m, 3), generator=g, device=device, dtype=torch.int64)
            kk = torch.where(kk < 2, kk - 2, kk - 1).double()                 # -2, -1, 1, 2
            shift = torch.where(torch.rand((m, 1), generator=g, device=device, dtype=torch.float64) < wrap, kk * L, shift)
        pos[i0:i1] = ((c.double() + off) * Lcell + shift).to(dtype)
        cells[i0:i1] = c.to(torch.int32)
        rho[i0:i1] = torch.randint(1, 4, (m,), generator=g, device=device, dtype=torch.int64).float()
        vel[i0:i1] = torch.randint(-3, 4, (m, 3), generator=g, device=device, dtype=torch.int64).float()
        del c, off, shift
    return cells, pos, rho, vel


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


# --------------------------------------------------------------------------- #
# Exact nearest neighbours at any particle count: brute force for a few points, a local search with a proof for a slab
# --------------------------------------------------------------------------- #
NN_UNCERTIFIED_CAP = 4096   # lattice points per run that nn_slab_reference may leave to nn_brute_force (asserted by the tests)
NN_BALL_PARTICLES = 50      # uniform-background particles expected inside the certified radius (nn_search_k)


def _axis(a, device):
    return torch.as_tensor(np.asarray(a, dtype=np.float64).copy(), dtype=torch.float64, device=device)


def _dist2(qx, qy, qz, px, py, pz):
    """((qx-px)^2 + (qy-py)^2) + (qz-pz)^2 in float64, every step an op of its own (orc.exact_nn_lattice's association)."""
    dx = qx - px
    dx = dx * dx
    dy = qy - py
    dy = dy * dy
    dx = dx + dy
    del dy
    dz = qz - pz
    dz = dz * dz
    return dx + dz


def nn_brute_force(pos, queries, batch=32, chunk=1 << 21):
    """Exact nearest particle of every query point (float64 [nq, 3]): the minimum of the squared distance over ALL particles, then
    the lowest index among those equal to it -- orc.exact_nn_lattice's rule (interp.py:1027-1037), in torch on pos.device.
    `batch` queries against `chunk` particles at a time (temporaries of batch * chunk float64: half a GB; ones of many GB were
    several times slower per pair on the device); the chunks ascend, so a later chunk takes over only with a strictly smaller
    distance and the lowest index keeps every tie.  -> (idx int64 [nq], best float64)."""
    n = pos.shape[0]
    q = queries.to(torch.float64)
    idx = torch.full((q.shape[0],), n, dtype=torch.int64, device=pos.device)
    best = torch.full((q.shape[0],), float("inf"), dtype=torch.float64, device=pos.device)
    big = torch.tensor(n, dtype=torch.int64, device=pos.device)
    for j in range(0, n, chunk):
        p = pos[j:j + chunk].double()
        px, py, pz = (p[:, c].contiguous()[None, :] for c in range(3))
        ar = torch.arange(j, j + p.shape[0], dtype=torch.int64, device=pos.device)[None, :]
        for i in range(0, q.shape[0], batch):
            b = q[i:i + batch]
            d = _dist2(b[:, 0:1], b[:, 1:2], b[:, 2:3], px, py, pz)
            m = d.amin(dim=1)
            first = torch.where(d == m[:, None], ar, big).amin(dim=1)
            less = m < best[i:i + batch]
            idx[i:i + batch] = torch.where(less, first, idx[i:i + batch])
            best[i:i + batch] = torch.where(less, m, best[i:i + batch])
            del d
    return idx, best


def lattice_points(axes, x0, nx, flat):
    """float64 [n, 3] coordinates of the slab's lattice points `flat` (((ix - x0) ny + iy) nz + iz), GATHERED from the axes."""
    ax, ay, az = axes
    ny, nz = ay.numel(), az.numel()
    return torch.stack((ax[x0 + flat // (ny * nz)], ay[(flat // nz) % ny], az[flat % nz]), dim=1)


def _nearest_index(a, p):
    """Index of the point of the monotonic axis `a` nearest to every p (a point half way goes to either side)."""
    if a.numel() == 1:
        return torch.zeros(p.shape, dtype=torch.int64, device=p.device)
    asc = bool(a[-1] > a[0])
    s = a if asc else a.flip(0)
    if not bool((s[1:] > s[:-1]).all()):
        raise ValueError("lattice axes must be strictly monotonic")
    j = torch.searchsorted((s[:-1] + s[1:]) * 0.5, p.contiguous())
    return j if asc else (a.numel() - 1) - j


def nn_gap_min(axes):
    """Smallest distance between neighbouring points over the three axes (axes of one point do not count)."""
    return min(float((a[1:] - a[:-1]).abs().min()) for a in axes if a.numel() > 1)


def nn_search_k(nbar, gap_min, want=NN_BALL_PARTICLES):
    """Smallest k with nbar (4 pi / 3) ((k + 1/2) gap_min)^3 >= want: the certified radius then holds `want` particles of a
    uniform background of number density nbar on average -- a point without one inside has probability exp(-want)."""
    k = 0
    while nbar * (4 * np.pi / 3) * ((k + 0.5) * gap_min) ** 3 < want:
        k += 1
    return k


def nn_slab_reference(pos, axes, x0, nx, k, budget=1 << 25):
    """Exact nearest particle of the lattice points axes[0][x0:x0+nx] x axes[1] x axes[2] (float64 tensors on pos.device,
    strictly monotonic, any spacing) by a LOCAL search: every particle finds the lattice index nearest to it per axis
    (searchsorted) and offers its float64 distance (_dist2, axis values gathered) to the (2k+1)^3 lattice points around it;
    scatter_reduce(amin) keeps the minimum, a second pass the lowest particle index among the distances equal to it.
    -> (idx int64, best float64, certified bool), flat over the slab; idx = np where no particle reached the point.
    Proof of `certified`: a lattice point more than k indices from a particle's nearest point on some axis is at least
    (k + 1/2) gap_min from it on that axis (the particle is no farther than half a gap beyond its nearest point's neighbour, the
    lattice point k whole gaps farther), so best < ((k + 1/2) gap_min (1 - 1e-6))^2 proves that no particle outside the search
    wins or ties.  Every other point is for nn_brute_force.  Distances are non-negative, so their int64 bit patterns order
    as they do: the minimum is taken on those (integer atomics), in three rounds of growing share so that the particles of a
    clump do not all contend for the same few words."""
    dev = pos.device
    ax, ay, az = axes
    ny, nz = ay.numel(), az.numel()
    n = pos.shape[0]
    nq = nx * ny * nz
    jx = _nearest_index(ax, pos[:, 0].double())
    near = torch.nonzero((jx >= x0 - k) & (jx < x0 + nx + k)).squeeze(1)
    jx = jx[near]
    p = pos[near].double()
    jy = _nearest_index(ay, p[:, 1])
    jz = _nearest_index(az, p[:, 2])
    o = torch.arange(-k, k + 1, dtype=torch.int64, device=dev)
    oy, oz = (t.reshape(-1) for t in torch.meshgrid(o, o, indexing="ij"))
    step = max(1, budget // oy.numel())
    inf_bits = int(np.array(np.inf).view(np.int64))
    best = torch.full((nq,), inf_bits, dtype=torch.int64, device=dev)
    idx = torch.full((nq,), n, dtype=torch.int64, device=dev)

    def offers():
        """(flat lattice point, distance bits, particle) of every offer, a block at a time."""
        for dx in range(-k, k + 1):
            ix = jx + dx
            sel = torch.nonzero((ix >= x0) & (ix < x0 + nx)).squeeze(1)
            for i in range(0, sel.numel(), step):
                s = sel[i:i + step]
                iy = jy[s][:, None] + oy[None, :]
                iz = jz[s][:, None] + oz[None, :]
                ok = (iy >= 0) & (iy < ny) & (iz >= 0) & (iz < nz)
                iy.clamp_(0, ny - 1)
                iz.clamp_(0, nz - 1)
                ps = p[s]
                d = _dist2(ax[ix[s]][:, None], ay[iy], az[iz], ps[:, 0:1], ps[:, 1:2], ps[:, 2:3])
                flat = ((ix[s] - x0)[:, None] * ny + iy) * nz + iz
                who = near[s][:, None].expand(-1, oy.numel())
                yield flat[ok], d[ok].view(torch.int64), who[ok]

    for flat, bits, _ in offers():
        for stride in (256, 16, 1):
            f, b = flat[::stride], bits[::stride]
            keep = b < best[f]
            best.scatter_reduce_(0, f[keep], b[keep], "amin", include_self=True)
    for flat, bits, who in offers():
        eq = bits == best[flat]
        idx.scatter_reduce_(0, flat[eq], who[eq], "amin", include_self=True)
    best = best.view(torch.float64)
    bound = ((k + 0.5) * nn_gap_min(axes) * (1 - 1e-6)) ** 2
    return idx, best, best < bound


def nn_settle(pos, axes, x0, nx, idx, best, certified, cap=NN_UNCERTIFIED_CAP):
    """Finishes nn_slab_reference in place: every uncertified point -- none is skipped -- gets nn_brute_force's answer.
    -> number of uncertified points; more than `cap` of them is an error of the test's set-up (AssertionError) raised before
    anything is brute-forced."""
    open_ = torch.nonzero(~certified).squeeze(1)
    assert open_.numel() <= cap, "%d uncertified lattice points (cap %d): k is too small for these particles" % (open_.numel(), cap)
    if open_.numel():
        i, b = nn_brute_force(pos, lattice_points(axes, x0, nx, open_))
        idx[open_] = i
        best[open_] = b
    return int(open_.numel())


def nn_uniform_axis(N):
    """N points from half a step inside the unit box to half a step BEYOND it on the high side, step 1 / (N - 1): the shape of
    the library lattice (orc.lattice_axes_library) with points of its own."""
    h = 1.0 / (N - 1)
    return (np.arange(N, dtype=np.float64) + 0.5) * h


def nn_jittered_axis(N, seed, amp=0.3):
    """nn_uniform_axis with every point moved by up to +-amp steps: strictly increasing (gaps >= (1 - 2 amp) steps), not uniform."""
    h = 1.0 / (N - 1)
    return nn_uniform_axis(N) + np.random.default_rng(seed).uniform(-amp, amp, N) * h


def nn_matrix_particles(device, n, dtype, axes, x0, nx, seed, box_steps=10, ndup=1000, nlattice=8):
    """-> (pos `dtype` [n, 3] on `device`, nbar) for the slab axes[0][x0:x0+nx] of a lattice over the unit box, from a seeded
    generator: uniform in [0, 1)^3, then
      * the first tenth of the particles in a Gaussian clump, sigma = 0.01, centred in the slab (clipped to the box);
      * an empty box of box_steps lattice steps a side starting at the slab's first row, away from the clump (its particles are
        moved half the unit box up in y, modulo 1);
      * the last ndup particles are copies of the first ndup particles (beyond the clump's) whose x lies in the slab: exact ties,
        which the lower index must win;
      * nlattice particles exactly on lattice points of the slab (as exactly as `dtype` holds them).
    nbar: number density of the uniform part, 0.9 n."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    ax, ay, az = (_axis(a, device) for a in axes)
    pos = torch.rand((n, 3), generator=g, device=device, dtype=torch.float64)
    nclump = n // 10
    xs = torch.sort(ax[x0:x0 + nx]).values
    centre = torch.stack(((xs[0] + xs[-1]) * 0.5, ay[ay.numel() // 2], az[az.numel() // 2]))
    pos[:nclump] = (centre[None, :] + 0.01 * torch.randn((nclump, 3), generator=g, device=device, dtype=torch.float64)).clamp_(0.0, 1.0 - 1e-9)
    hx, hy, hz = (float((a[-1] - a[0]).abs()) / max(a.numel() - 1, 1) for a in (ax, ay, az))
    steps = torch.tensor([hx, hy, hz], dtype=torch.float64, device=device)
    lo = torch.stack((xs[0], torch.sort(ay).values[ay.numel() // 5], torch.sort(az).values[az.numel() // 5])) - 0.25 * steps
    hi = lo + box_steps * steps
    inside = ((pos >= lo[None, :]) & (pos < hi[None, :])).all(dim=1)
    pos[:, 1] = torch.where(inside, torch.remainder(pos[:, 1] + 0.5, 1.0), pos[:, 1])
    for j in range(min(nlattice, n - nclump - min(ndup, n // 8))):
        pos[nclump + j] = torch.stack((ax[x0 + (nx // 2 + j) % nx], ay[(3 * ay.numel()) // 4 + j % 3], az[(3 * az.numel()) // 4 - j % 5]))
    ndup = min(ndup, n // 8)
    if ndup:
        src = torch.nonzero((pos[nclump:n - ndup, 0] >= xs[0]) & (pos[nclump:n - ndup, 0] <= xs[-1])).squeeze(1)[:ndup] + nclump
        pos[n - src.numel():] = pos[src]
    return pos.to(dtype), 0.9 * n


# The legs of tests/test_gpu_nn_matrix.py: the smallest particle counts that reach each cell-list geometry (plan: what
# vps_nn_plan must say), a lattice over the unit box ("uniform": nn_uniform_axis, "library": orc.lattice_axes_library(1, N),
# "jittered": nn_jittered_axis), slabs (x0, nx) and the option sets every slab is searched under.
# tests/test_nn_reference_cpu.py runs every leg's set-up at a scaled-down particle count with the same nbar h^3.
NN_MATRIX = (
    # groups of 8192 cells (gshift 13, from 3.2e6 particles on): two rounds of the sort's level-2 counter scan (4096 counters each)
    dict(name="3.3e6 whole 64", n=3_300_000, dtype="float32", lattice=("uniform", 64), slabs=((0, 64),),
         runs=({},), plan=dict(M=130, gshift=13, ngroups=269, sorted=1, lds_fine=32832)),
    dict(name="7e6 whole 192", n=7_000_000, dtype="float32", lattice=("uniform", 192), slabs=((0, 192),),
         runs=({}, {"nn_column": 0}, {"nn_query_centric": 1}),
         plan=dict(M=167, gshift=14, ngroups=285, sorted=1, lds_fine=65600)),
    dict(name="1.4e7 float64 256", n=14_000_000, dtype="float64", lattice=("uniform", 256), slabs=((0, 16), (120, 16), (240, 16)),
         runs=({},), plan=dict(M=210, gshift=15, ngroups=283, sorted=1, lds_fine=131136)),
    dict(name="2.7e7 320", n=27_000_000, dtype="float32", lattice=("uniform", 320), slabs=((0, 16), (120, 16), (240, 16), (304, 16)),
         runs=({},), plan=dict(M=262, gshift=15, ngroups=549, sorted=1, lds_fine=131136)),
    dict(name="5e7 384", n=50_000_000, dtype="float32", lattice=("uniform", 384), slabs=((0, 16), (184, 16), (368, 16)),
         runs=({},), plan=dict(M=321, gshift=15, ngroups=1010, sorted=1, lds_fine=131136)),
    dict(name="5e7 library 1024", n=50_000_000, dtype="float32", lattice=("library", 1024), slabs=((0, 8), (504, 8), (1016, 8)),
         runs=({}, {"nn_column": 0}), plan=dict(M=321, gshift=15, ngroups=1010, sorted=1, lds_fine=131136)),
    dict(name="5e7 jittered 384", n=50_000_000, dtype="float32", lattice=("jittered", 384), slabs=((184, 4),),
         runs=({},), plan=dict(M=321, gshift=15, ngroups=1010, sorted=1, lds_fine=131136)),
    dict(name="1e8 448", n=100_000_000, dtype="float32", lattice=("uniform", 448), slabs=((0, 8), (216, 8), (440, 8)),
         runs=({},), plan=dict(M=405, gshift=15, ngroups=2028, sorted=1, lds_fine=131136)),
    dict(name="1.05e8 448", n=105_000_000, dtype="float32", lattice=("uniform", 448), slabs=((0, 8), (216, 8), (440, 8)),
         runs=({},), plan=dict(M=412, ngroups=2135, sorted=0, lds_fine=0)),
)


def nn_matrix_axes(lattice, seed=0):
    """The three float64 numpy axes of a leg's lattice."""
    kind, N = lattice
    if kind == "uniform":
        return [nn_uniform_axis(N)] * 3
    if kind == "library":
        from oracle import vps_oracle as orc
        return [orc.lattice_axes_library(1.0, N)] * 3
    if kind == "jittered":
        return [nn_jittered_axis(N, seed + a) for a in range(3)]
    raise ValueError(kind)


def nn_search_kind(lattice, opts):
    """The search vps_nn_resample must report for a leg's lattice under `opts`: the column kernel wherever the lattice is
    uniform and about as fine as the particles are dense (every leg here: mean spacing / step <= 2.8 against a cutoff near 3)."""
    if lattice[0] == "jittered" or opts.get("nn_query_centric"):
        return "ring"
    return "scatter" if opts.get("nn_column") == 0 else "column"


# --------------------------------------------------------------------------- #
# Custom k ranges: the table of tests/test_gpu_krange_matrix.py and the host-side rules it holds the library to
# --------------------------------------------------------------------------- #
# name -> (flavour, (kmin, kmax, kres) in units of kf = 2 pi / L as a function of h = N / 2).  What each row reaches:
#   deep    most planes without a kept row (cut -1): whole tiles and planes skipped
#   band    modes below the first edge, the float guess clamped at both ends, generic edges
#   zero    first edge exactly 0 (np.histogram counts the k = 0 mode in bin 0), every edge on an integer multiple of kf
#   corner  all_mode_k_range: nothing cut, a packed scope whose slots all fall back to N rows
#   fine    several shells per kx step, nbins ~ 0.68 N
#   many    nbins ~ N, every bin well filled: LDS offsets far from the default
#   wide    2 bins of millions of modes each: partial counts and the reduction
K_RANGES = {
    "deep": ("script", lambda h: (1.0, float(round(0.3 * h)), 1.0)),
    "band": ("library", lambda h: (0.25 * h, 0.6 * h, 1.7)),
    "zero": ("library", lambda h: (0.5, float(h), 1.0)),
    "corner": ("script", None),
    "fine": ("library", lambda h: (1.0, 0.5 * h, 0.37)),
    "many": ("script", lambda h: (0.25 * h, 0.5 * h, 0.13)),
    "wide": ("script", lambda h: (0.3 * h, 0.8 * h, 0.5 * h)),
}


def k_range(name, N, L):
    """(flavour, kmin, kmax, kres) of row `name` of K_RANGES on an N^3 grid of box length L."""
    flavour, f = K_RANGES[name]
    if f is None:
        return (flavour,) + tuple(all_mode_k_range(N, L))
    kf = 2 * np.pi / L
    return (flavour,) + tuple(x * kf for x in f(N // 2))


def k_range_edges(name, N, L):
    """(centres, edges) of the row with the reference's own numpy expressions (orc.edges_library: interp.py:1472-1473,
    orc.edges_script: parallel_optimized.py:178-180), or None where np.arange leaves centres and edges inconsistent."""
    from oracle import vps_oracle as orc
    flavour, kmin, kmax, kres = k_range(name, N, L)
    centers, edges = (orc.edges_library if flavour == "library" else orc.edges_script)(kmin, kmax, kres)
    return (centers, edges) if len(edges) == len(centers) + 1 else None


K_ROUTE_ROWS = ("deep", "zero", "fine")     # the rows BoxField.spctrm / helmholtz_spctrm are given (library flavour there)


def k_range_box(name, N):
    """Box length of the row at N: 1, or 2.5 where np.arange leaves the library flavour's centres and edges inconsistent at 1
    -- asked of the library-flavour rows and of K_ROUTE_ROWS, which the user-facing routes bin with the library flavour
    whatever the table says (`deep` takes 2.5 at N = 192; at 2.5 it would fail at N = 1024)."""
    from oracle import vps_oracle as orc
    for L in (1.0, 2.5):
        flavour, kmin, kmax, kres = k_range(name, N, L)
        if flavour == "library" or name in K_ROUTE_ROWS:
            centers, edges = orc.edges_library(kmin, kmax, kres)
            if len(edges) != len(centers) + 1:
                continue
        if k_range_edges(name, N, L) is not None:
            return L
    raise AssertionError((name, N))


def expected_binning_mode(N, k2_axis, thr, edges):
    """The binning mode include/vps_hip.h documents for vps_set_binning, restated: 0 general shell walk, 1 mirrored kx with
    float64 k^2 sums, 2 integer shells.  Mirrored kx needs an even N, k2[N - i] == k2[i], k2 non-decreasing up to N/2 and the
    double-precision guess (sqrt(thr[i]) - edges[0]) / spacing within 1e-3 of i at every threshold (spacing = the mean bin
    width).  Integer shells need, on top, k2[i] = i^2 k2[1] to 1e-12 and no thr[b] / k2[1] within 1e-9 (relative, floor 1) of an
    integer (a threshold ON a mode: float64 rounding decides)."""
    k2 = np.asarray(k2_axis, dtype=np.float64)
    thr = np.asarray(thr, dtype=np.float64)
    nb = len(thr) - 1
    h = N // 2
    inv = nb / (float(edges[-1]) - float(edges[0]))
    if N % 2 or any(k2[N - i] != k2[i] for i in range(1, h)) or np.any(np.diff(k2[: h + 1]) < 0):
        return 0
    if np.any(np.abs((np.sqrt(thr) - float(edges[0])) * inv - np.arange(nb + 1)) >= 1e-3):
        return 0
    i2 = np.arange(h + 1, dtype=np.float64) ** 2
    if not (k2[0] == 0.0 and k2[1] > 0 and np.all(np.abs(k2[: h + 1] - i2 * k2[1]) <= 1e-12 * i2 * k2[1])):
        return 1
    q = thr / k2[1]
    pos = q[q > 0]
    if np.any(pos >= 4.0e9) or np.any(np.abs(pos - np.rint(pos)) <= 1e-9 * np.maximum(pos, 1.0)):
        return 1
    return 2


def row_cut(N, k2_axis, thr):
    """The row cut of a binning-only scope (include/vps_hip.h: vps_set_bin_only), restated: per plane kz = 0..N/2 the largest
    |ky| with a mode inside the last edge -- not fl(k2[ky] + k2[kz]) >= thr[nbins] -- rounded up to 16 k + 15 and capped at
    N/2; -1 for a plane no shell reaches.  (The library keeps one from N = 128 on, under the mirrored-kx modes.)"""
    k2 = np.asarray(k2_axis, dtype=np.float64)
    h = N // 2
    out = np.full(h + 1, -1, dtype=np.int64)
    for kz in range(h + 1):
        ok = np.nonzero(~((k2[: h + 1] + k2[kz]) >= thr[-1]))[0]
        if len(ok):
            out[kz] = min(int(ok[-1]) | 15, h)
    return out


def slot_cuts(kcut, N, G, C):
    """[chunk][slot] -> the cuts of the G planes that share the slot: slot j of rank r in chunk c is plane c G nkc + j G + r
    (nkc = N / 2 / G / C; include/vps_hip.h: vps_fft_y)."""
    nkc = N // 2 // G // C
    return [[[int(kcut[c * G * nkc + j * G + r]) for r in range(G)] for j in range(nkc)] for c in range(C)]


def slot_rows(cuts, N):
    """Rows a packed slot carries: 2 kc + 1 with kc = the largest cut of its planes, floored at 0 -- or all N rows."""
    kc = max(max(cuts), 0)
    return N if 2 * kc + 1 >= N else 2 * kc + 1


def packed_block(kcut, N, nx, G, C, chunk):
    """Elements of one destination's block of a packed chunk: the rows of its slots times nx, plus (last chunk) the rank's
    N / G rows of the Nyquist plane."""
    rows = sum(slot_rows(s, N) for s in slot_cuts(kcut, N, G, C)[chunk])
    return rows * nx + ((N // G) * nx if chunk == C - 1 else 0)


def slot_mix(kcut, N, G, C):
    """Counts of the slot kinds the packed layout has to get right -> dict(mixed: a dead plane (-1) next to live ones,
    dead: every plane dead, unequal: live planes with different cuts, full: slots of N rows, slots: all)."""
    out = dict(mixed=0, dead=0, unequal=0, full=0, slots=0)
    for chunk in slot_cuts(kcut, N, G, C):
        for s in chunk:
            out["slots"] += 1
            live = [c for c in s if c >= 0]
            out["dead"] += not live
            out["mixed"] += bool(live) and len(live) < len(s)
            out["unequal"] += len(set(s)) > 1
            out["full"] += slot_rows(s, N) == N
    return out


# The legs of tests/test_gpu_krange_matrix.py; tests/test_separable_reference.py asserts what every (N, row) is there for
K_WHOLE = {64: tuple(K_RANGES), 128: tuple(K_RANGES), 192: tuple(K_RANGES), 250: tuple(K_RANGES), 256: tuple(K_RANGES),
           1024: ("deep", "zero", "many", "wide")}
K_HELMHOLTZ = {128: tuple(K_RANGES), 192: tuple(K_RANGES), 250: tuple(K_RANGES), 1024: ("deep", "zero")}
K_WINDOW = {256: ("deep", "band"), 1024: ("deep", "band")}
K_SLABS = ((128, 4, 2), (192, 4, 3), (250, 5, 5), (256, 8, 2), (1024, 16, 2))      # (N, ranks, kz chunks)
K_SLAB_ROWS = ("deep", "band", "zero", "corner")
# rows whose edges fall on integer multiples of kf: integer shells must be refused (mode 1); every other (row, N) takes mode 2.
# `deep` at N = 128, L = 1: (19 kf - kf) / kf = 17.999999999999996, so the script flavour's int() gives 18 bins over 19 kf
# (the reference's quirk Q2) and edge 9 sits on 10 kf
K_MODE1 = {("zero", N) for N in (64, 128, 192, 250, 256, 1024)} | {("band", 250), ("many", 64), ("many", 128), ("deep", 128)}
