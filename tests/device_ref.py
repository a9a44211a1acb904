"""Device-resident mirrors of the whole-grid kernels, for grids that numpy cannot follow (10^9 cells): test infrastructure, never
imported by the package.  The float32 mirrors of tests/gradient_ref.py (fields32) and tests/filter_ref.py (fields32_all) restated
in torch, on whatever device the input lives on, for the EXACT input schemes of those files:
  gradient   integer velocities |u| <= 1024 and a power-of-two Lcell: every difference, product with h and sum is exact;
  filter     integer |u| <= 3, masses in {0, 1, 2}, a cube of empty cells that holds whole boxes: the box sums are integers below
             2^24, formed here in int64 (exact in any order), then the float32 roundings of the header in its order -- the product
             P_i P_j, the division by M, the subtraction, the clamp of the diagonals, the scaling by c = (float32)(1 / (2m+1)^3),
             and exact zeros where the integer count of cells with mass is 0.
Everything works ONE X-SLAB AT A TIME: at most `slab` output planes (64 unless asked otherwise) and the wrapped halo of 1 plane
(gradient) or m planes (filter) on each side, copied out of the grid plane range by plane range.  Every torch op sees a fresh
tensor of far fewer than 2^31 elements, or a contiguous one-channel view of that many planes of the grid, whose start is a pointer
the host forms in 64 bits: nothing here rests on how torch itself indexes a tensor of 2^31 elements or more.  The helpers that
walk a whole tensor (fill, count_nan, checksum) take its flat view in pieces of 2^26 elements for the same reason.
Values compare as float32 VALUES (-0 == +0, as np.array_equal does in the small-grid tests; NaN differs from everything, so an
element left at the poison counts).  tests/test_device_ref_cpu.py holds these mirrors to the numpy ones on the CPU,
tests/test_gpu_large_grids.py on the GPU."""
import numpy as np
import torch

import filter_ref as fr
import gradient_ref as gr

SLAB = 64                  # output planes of a slab
PIECE = 1 << 26            # elements of a piece of a flat walk
LIMIT = 1 << 31            # no tensor an op sees has this many elements


GRADIENT_N = (16, 18, 96)                                          # the small cases of the mirrors, on the CPU and on the GPU
FILTER_NM = ((6, 2), (18, 8), (34, 8), (64, 4))


def slab_heights(N):
    """Slab heights that do not divide N, that exceed it or equal the default, and N itself."""
    return (5, 64, N)


def whole(N, slab, slab_of):
    """The slabs of slab_of(x0, x1), joined along x: [NCH, N, N, N] numpy."""
    return torch.cat([slab_of(x0, x1) for x0, x1 in slabs(N, slab)], dim=1).numpy()


def slabs(N, slab=SLAB):
    """[(x0, x1)]: the x ranges of the slabs of an N^3 grid."""
    return [(x0, min(x0 + slab, N)) for x0 in range(0, N, slab)]


def planes(field, a, b):
    """The planes a .. b - 1 of field [N, N, N], every index wrapped (a may be negative, b beyond N), as a NEW tensor
    [b - a, N, N]: copies of contiguous plane ranges, joined."""
    N = field.shape[0]
    assert field.dim() == 3 and a < b and (b - a) * N * N < LIMIT
    parts = []
    while a < b:
        s = a % N
        n = min(b - a, N - s)
        parts.append(field[s:s + n])
        a += n
    return torch.cat(parts)


# ------------------------------------------------------------------ generators ----
def _fill(N, seed, device, slab, plane_of):
    """[4, N, N, N] float32 on `device`, slab by slab; plane x is plane_of(generator seeded by (seed, x)) -> [4, N, N]: the
    tensor does not depend on the slab height."""
    ch = torch.empty((4, N, N, N), dtype=torch.float32, device=device)
    g = torch.Generator(device=device)
    for x0, x1 in slabs(N, slab):
        buf = torch.empty((4, x1 - x0, N, N), dtype=torch.float32, device=device)
        for x in range(x0, x1):
            g.manual_seed(int(seed) * 1_000_003 + x)
            buf[:, x - x0] = plane_of(g, x)
        for c in range(4):
            ch[c, x0:x1].copy_(buf[c])
    return ch


def integer_velocity(N, seed, device, slab=SLAB, amp=1024):
    """The gradient's exact inputs (gradient_ref.integer_velocity): integers in [-amp, amp], random per cell -- a read displaced
    by any number of elements meets another value in all but 1 / (2 amp + 1) of the cells.  The mass channel is NaN: it is not
    read, and would show."""
    def plane_of(g, x):
        p = torch.empty((4, N, N), dtype=torch.float32, device=device)
        p[:3] = torch.randint(-amp, amp + 1, (3, N, N), generator=g, device=device, dtype=torch.int32)
        p[3] = float("nan")
        return p
    return _fill(N, seed, device, slab, plane_of)


def integer_chans(N, seed, device, slab=SLAB):
    """The filter's exact inputs (filter_ref.integer_chans): integer velocities |u| <= 3, masses in {0, 1, 2}, and the cube of
    min(N - 1, 19) empty cells at the origin, which holds whole boxes up to m = 8 where N allows."""
    hole = min(N - 1, 19)

    def plane_of(g, x):
        p = torch.empty((4, N, N), dtype=torch.float32, device=device)
        p[:3] = torch.randint(-3, 4, (3, N, N), generator=g, device=device, dtype=torch.int32)
        p[3] = torch.randint(0, 3, (N, N), generator=g, device=device, dtype=torch.int32)
        if x < hole:
            p[3, :hole, :hole] = 0
        return p
    return _fill(N, seed, device, slab, plane_of)


# ------------------------------------------------------------------ gradient ----
def _need(what, c, a):
    return c == a if what == "divergence" else c != a if what == "vorticity" else True


def gradient_slab(ch, Lcell, what, x0, x1):
    """[NCH, x1 - x0, N, N] float32: gradient_ref.fields32(ch[:3], Lcell, what) on the planes x0 .. x1 - 1 -- h rounded to float32
    once, d = (u(+) - u(-)) * h by wrapped index, the sums in the order of gradient_ref._fields."""
    assert ch.dtype == torch.float32 and what in gr.CODES
    h = float(np.float32(1.0 / (2.0 * float(Lcell))))              # (a float32 value: the product rounds once, in float32)
    d = {}
    for c in range(3):
        if not any(_need(what, c, a) for a in range(3)):
            continue
        u = planes(ch[c], x0 - 1, x1 + 1)
        mid = u[1:-1]
        if _need(what, c, 0):
            d[c, 0] = (u[2:] - u[:-2]) * h
        for a in (1, 2):
            if _need(what, c, a):
                d[c, a] = (torch.roll(mid, -1, dims=a) - torch.roll(mid, 1, dims=a)) * h
        del u, mid
    if what == "divergence":
        out = [(d[0, 0] + d[1, 1]) + d[2, 2]]
    elif what == "vorticity":
        out = [d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]]
    else:
        out = [d[0, 0], d[1, 1], d[2, 2], 0.5 * (d[0, 1] + d[1, 0]), 0.5 * (d[0, 2] + d[2, 0]), 0.5 * (d[1, 2] + d[2, 1])]
    out = torch.stack(out)
    assert out.dtype == torch.float32 and out.numel() < LIMIT
    return out


# ------------------------------------------------------------------ filter ----
def _box_axis(t, m, dim, wrap):
    """Sums of 2m + 1 consecutive entries of the int64 tensor t along dim: periodic (same length) with wrap, else over the
    entries given (2m shorter: the halo is already there)."""
    if wrap:
        n = t.shape[dim]
        t = torch.cat([t.narrow(dim, n - m, m), t, t.narrow(dim, 0, m)], dim)
    n = t.shape[dim] - 2 * m
    cs = torch.cumsum(t, dim)
    out = cs.narrow(dim, 2 * m, n).clone()                         # cs[i + 2m] - cs[i - 1], cs[-1] = 0
    if n > 1:
        out.narrow(dim, 1, n - 1).sub_(cs.narrow(dim, 0, n - 1))
    return out


def _box_sum(t, m):
    """[h + 2m, N, N] (a slab with its x halo) -> [h, N, N] int64 box sums; exact."""
    t = t.to(torch.int64)
    assert t.numel() < LIMIT
    return _box_axis(_box_axis(_box_axis(t, m, 0, False), m, 1, True), m, 2, True)


def filter_sums(ch, m, x0, x1, stress=True):
    """(s, has) of the planes x0 .. x1 - 1: s = the float32 box sums M, P_x, P_y, P_z and (with `stress`) S_xx, S_yy, S_zz, S_xy,
    S_xz, S_yz as a list of [h, N, N] tensors in the order of filter_ref.terms, has = the integer count of cells with mass in
    the box != 0.  The per-cell products are float32 (exact: small integers), the sums int64, their conversion to float32 exact
    (below 2^24: asserted from the inputs' range, as filter_ref.fields32_all does)."""
    assert ch.dtype == torch.float32 and 2.0 * 9.0 * (2 * m + 1) ** 3 < 2 ** 24
    u = [planes(ch[c], x0 - m, x1 + m) for c in range(3)]
    ms = planes(ch[3], x0 - m, x1 + m)
    assert float(ms.abs().max()) <= 2 and max(float(x.abs().max()) for x in u) <= 3, "not the exact input scheme"
    p = [ms * u[c] for c in range(3)]
    s = [_box_sum(ms, m).float()] + [_box_sum(x, m).float() for x in p]
    if stress:
        s += [_box_sum(p[i] * u[j], m).float() for i, j in fr.IJ]
    has = _box_sum(ms != 0, m) != 0
    return s, has


def filter_form(s, has, m, what):
    """[NCH, h, N, N] float32: filter_ref._form in float32 -- one rounding per operation, in the header's order."""
    c = float(np.float32(1.0 / (2 * m + 1) ** 3))
    M = s[0]
    Ms = torch.where(has, M, torch.ones_like(M))
    zero = torch.zeros_like(M)
    if what == "vm":
        out = [torch.where(has, s[1 + a] / Ms, zero) for a in range(3)] + [torch.where(has, M * c, zero)]
    else:
        assert what == "stress"
        out = []
        for k, (i, j) in enumerate(fr.IJ):
            t = s[4 + k] - (s[1 + i] * s[1 + j]) / Ms
            if i == j:
                t = torch.maximum(t, zero)
            out.append(torch.where(has, t * c, zero))
    out = torch.stack(out)
    assert out.dtype == torch.float32 and out.numel() < LIMIT
    return out


def filter_slab(ch, m, what, x0, x1):
    """[NCH, x1 - x0, N, N] float32: filter_ref.fields32_all(ch, m)[what] on the planes x0 .. x1 - 1."""
    s, has = filter_sums(ch, m, x0, x1, stress=what == "stress")
    return filter_form(s, has, m, what)


# ------------------------------------------------------------------ checker ----
def compare(got, ref_slab, x0):
    """The number of elements of got[:, x0 : x0 + h] that differ from ref_slab [NCH, h, N, N]; got: the whole output
    [NCH, N, N, N].  One channel at a time: got[k, x0 : x0 + h] is contiguous."""
    h = ref_slab.shape[1]
    assert got.shape[0] == ref_slab.shape[0] and got.shape[2:] == ref_slab.shape[2:] and x0 + h <= got.shape[1]
    n = torch.zeros((), dtype=torch.int64, device=got.device)
    for k in range(ref_slab.shape[0]):
        n += (got[k, x0:x0 + h] != ref_slab[k]).sum()
    return int(n)


def first_difference(got, ref_slab, x0):
    """(channel, x, y, z, linear element offset in got) of the first differing element of the slab, None if there is none."""
    h, N = ref_slab.shape[1], got.shape[2]
    for k in range(ref_slab.shape[0]):
        ne = (got[k, x0:x0 + h] != ref_slab[k]).reshape(-1)
        if bool(ne.any()):
            i = int(torch.nonzero(ne)[0])
            x, y, z = x0 + i // (N * N), i // N % N, i % N
            return k, x, y, z, ((k * N + x) * N + y) * N + z
    return None


def describe(got, ref_slab, x0):
    """The message of a failed slab: where the first difference is, as a multiple of 2^31 elements as well."""
    k, x, y, z, off = first_difference(got, ref_slab, x0)
    return ("slab x = %d..%d: %d elements differ; the first in channel %d at (%d, %d, %d), element offset %d = %.6f * 2^31, got %r, "
            "expected %r" % (x0, x0 + ref_slab.shape[1] - 1, compare(got, ref_slab, x0), k, x, y, z, off, off / 2.0 ** 31,
                             float(got[k, x, y, z]), float(ref_slab[k, x - x0, y, z])))


def _pieces(t):
    assert t.is_contiguous()
    flat = t.view(-1)
    for i in range(0, flat.numel(), PIECE):
        yield flat[i:i + PIECE]


def fill(t, value):
    """Every element of the contiguous tensor t <- value, piece by piece."""
    for p in _pieces(t):
        p.fill_(value)


def count_nan(t):
    """The number of NaN in the whole contiguous tensor t, piece by piece."""
    n = torch.zeros((), dtype=torch.int64, device=t.device)
    for p in _pieces(t):
        n += torch.isnan(p).sum()
    return int(n)


def checksum(t):
    """A tuple of ints, one per piece of the float32 tensor t: the sum of its elements' bit patterns.  Any single changed
    element changes it."""
    assert t.dtype == torch.float32
    return tuple(int(p.view(torch.int32).sum(dtype=torch.int64)) for p in _pieces(t))
