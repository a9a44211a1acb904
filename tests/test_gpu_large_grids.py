"""The two whole-grid kernels -- the stencil of csrc/gradient.hip (VPS_DIVERGENCE, VPS_VORTICITY, VPS_STRAIN_RATE) and the box
filter of csrc/filter.hip (VPS_FILTERED_VM, VPS_FILTERED_STRESS) -- on grids whose element offsets pass 2^31 and 2^32, against
the device-resident mirrors of tests/device_ref.py, every element of every output.  These kernels take whole grids only, so no
thin slab of a large grid reaches them: the grid itself has to be large.

a. The mirrors run ON THE GPU at the small sizes of tests/test_device_ref_cpu.py and are held to the numpy mirrors: this is what
   licenses their float32 products and division on the device (they are float32 throughout; no step had to be formed in float64).

b. The kernels at the smallest even N that cross each boundary, one size per store width (16-byte groups where N % 4 == 0, else
   8-byte), asserted from the arithmetic in _boundaries():
     N     store    input 4 N^3 elements            6-channel output           codes          x chunks, 256 CUs: gradient / filter
     896   16-byte  2.88e9: past 2^31 elements and  4.32e9: past 2^32          all five       6 of 150 planes   / 14 of 64
     898    8-byte  2^32 bytes, below 2^32 elements (892 and 894: below)       all five       3 of 300          / 15 of 60
     1028  16-byte  4.35e9: past 2^32 elements      6.52e9                     strain, stress 4 of 257          / 17 of 61
     1026   8-byte  (1024: the last is 2^32 - 1)    6.48e9                     strain, stress 2 of 513          / 17 of 61
   Per channel (channel k starts at element k N^3): at 896 / 898 the input channel 2 crosses 2^31 elements and channel 3 lies
   past it, all below 2^32; the output channel 2 crosses 2^31, channels 3 .. 5 lie past it and channel 5 crosses 2^32; the
   1- and 3-channel outputs of the divergence and the vorticity stay below 2^32 (the vorticity's third channel crosses 2^31),
   and so does the filter's 4-channel VM.  At 1026 / 1028 every channel is longer than 2^30 elements: channel 1 of the input
   and of the output crosses 2^31, channel 3 crosses 2^32, and the output channels 4, 5 lie past 2^32 altogether.  Half-width
   m = 8 throughout: the widest halo, the longest region walk, the most planes read ahead of a chunk.
   The chunk layouts are asserted from gradient_ref.layout / filter_ref.layout: the gradient marches x chunks of 150 to 513 planes
   here (the small-grid tests reach 84), the filter launches 14 to 17 chunks per tile column.
   Per case: the output is filled with NaN, the kernel runs on the whole grid, and then (1) the whole output holds no NaN, (2)
   every slab of 64 planes equals the mirror -- the message names the first differing slab, channel and element offset, so that a
   2^31 or 2^32 pattern is legible -- (3) the checksum of the input is unchanged, (4) for VM both the M = 0 path and the other one
   occurred.  One more case at 896 holds BoxField.scale_flux to the composition of the three kernels (flux_contraction and
   _from_device on tensors past 2^31 elements).
   Memory: the input, one output and the slab temporaries, 45 GiB at 1028 (60 GiB for the scale-flux case); with less free memory
   a case FAILS and says so -- a skip would hide it for good.

What the sensitivity of (2) rests on is tests/test_device_ref_cpu.py (the checker sees swapped planes, a shifted channel, one
poisoned element); no kernel was built with narrowed offsets to see these cases fail.

Found (one MI355X, 256 CUs, 288 GB): NO element differed and none was left unwritten, at any of the four sizes and for any
code; the inputs were untouched; the layouts were the ones of the table; the device mirrors equal the numpy mirrors at every
small case.  Neither kernel was changed.
Measured wall time per case, s (poison, launch and synchronise, NaN scan, mirror and compare of every slab, checksum), against
the one to three seconds that had been supposed:
  gradient 896: 0.05 / 0.09 / 0.14 (divergence / vorticity / strain rate)   898: 0.05 / 0.09 / 0.15   1028: 0.21   1026: 0.22
  filter   896: 0.31 / 0.61 (VM / stress)   898: 0.36 / 0.64   1028: 0.94   1026: 0.94
  of which the kernel: strain rate 6 ms (896), 14 ms (898), 17 ms (1028), 23 ms (1026); stress 27 / 37 / 43 / 55 ms
  an input: 0.04 - 0.07 s; scale_flux at 896: 2.6 s for the two routes (the host copy of Pi), 0.06 s to compare
  the small mirror cases: 0.4 s at most.  The first case that asks the driver for a larger block than any before it waits 3 - 4 s
  for the allocation (seen at 1026: gradient input, stress output); with that the whole file takes 20 s.
  The filter's sums are NOT shared between VM and stress: no case is near the 10 s at which that was to be the first cut.
Run on an MI355X:  python -m pytest tests/test_gpu_large_grids.py -q -m gpu -s"""
import ctypes
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import device_ref as dr  # noqa: E402
import filter_ref as fr  # noqa: E402
import gradient_ref as gr  # noqa: E402

FILTER_NM, GRADIENT_N, slab_heights, whole = dr.FILTER_NM, dr.GRADIENT_N, dr.slab_heights, dr.whole

M = 8                       # the filter's half-width at every large size
LCELL = 0.25                # a power of two: h = 2 exactly
GIB = 2 ** 30
# x chunk and cells per group of the two launches on the 256 CUs of an MI355X: (gradient, filter)
LAYOUT_256 = {896: ((150, 4), (64, 4)), 898: ((300, 2), (60, 2)), 1028: ((257, 4), (61, 4)), 1026: ((513, 2), (61, 2))}
GRADIENT_CASES = [(896, w) for w in gr.CODES] + [(898, w) for w in gr.CODES] + [(1028, "strain_rate"), (1026, "strain_rate")]
# (896 last: the scale-flux case after it takes the same input)
FILTER_CASES = [(898, w) for w in fr.CODES] + [(1028, "stress"), (1026, "stress")] + [(896, w) for w in fr.CODES]


@pytest.fixture(scope="module")
def K():
    from vpower import device
    return device.default_kernels()


def _cus(K):
    info = (ctypes.c_int64 * 4)()
    assert K.lib.vps_device_info(K.ctx, info) == 0
    return int(info[0])


def _need_memory(nbytes, label):
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    if free < nbytes:
        pytest.fail("%s needs %.1f GiB of device memory and %.1f GiB of %.1f GiB are free: the case did NOT run"
                    % (label, nbytes / GIB, free / GIB, total / GIB))


class Inputs:
    """The input of one (scheme, N) at a time, with its checksum: generated when first asked for, let go of when another is."""

    def __init__(self, device):
        self.device, self.key, self.ch, self.sum = device, None, None, None

    def get(self, scheme, N):
        if self.key != (scheme, N):
            self.drop()
            _need_memory((4 * 4 * N ** 3) + 1 * GIB, "the input at N = %d" % N)
            t0 = time.perf_counter()
            make = dr.integer_velocity if scheme == "gradient" else dr.integer_chans
            self.ch = make(N, seed=N, device=self.device)
            self.sum = dr.checksum(self.ch)
            self.key = (scheme, N)
            torch.cuda.synchronize()
            print("\n[%s input N=%d: generated and summed in %.2f s]" % (scheme, N, time.perf_counter() - t0), end=" ")
        return self.ch, self.sum

    def drop(self):
        self.key = self.ch = self.sum = None
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def inputs(K):
    held = Inputs(K.device)
    yield held
    held.drop()


# ------------------------------------------------------------------ a. the mirrors on the device ----
@pytest.mark.parametrize("N", GRADIENT_N)
def test_gradient_mirror_on_the_device_equals_the_numpy_mirror(K, N):
    ch = dr.integer_velocity(N, seed=N, device=K.device)
    ref = gr.fields32_all(ch[:3].cpu().numpy(), LCELL)
    for what in gr.CODES:
        for slab in slab_heights(N):
            got = whole(N, slab, lambda x0, x1: dr.gradient_slab(ch, LCELL, what, x0, x1).cpu())
            assert np.array_equal(got, ref[what]), (what, N, slab, int(np.sum(got != ref[what])))
        assert np.abs(ref[what]).max() > 0


@pytest.mark.parametrize("N,m", FILTER_NM)
def test_filter_mirror_on_the_device_equals_the_numpy_mirror(K, N, m):
    ch = dr.integer_chans(N, seed=100 * N + m, device=K.device)
    refs = fr.fields32_all(ch.cpu().numpy(), m)
    for what in fr.CODES:
        for slab in slab_heights(N):
            got = whole(N, slab, lambda x0, x1: dr.filter_slab(ch, m, what, x0, x1).cpu())
            assert np.array_equal(got, refs[what]), (what, N, m, slab, int(np.sum(got != refs[what])))
        assert np.abs(refs[what]).max() > 0
    assert (refs["vm"][3] == 0).any() and (refs["vm"][3] > 0).any()
    # ... and the kernel agrees with the device mirror here, as it does with the numpy one (tests/test_gpu_filter.py)
    for what in fr.CODES:
        assert dr.compare(K.box_filter(ch, N, m, what), dr.filter_slab(ch, m, what, 0, N), 0) == 0, what


# ------------------------------------------------------------------ b. the kernels at large N ----
def _boundaries(N):
    """The arithmetic of the table in the module docstring."""
    n3 = N ** 3
    assert N % 2 == 0 and (N % 4 == 0) == (N in (896, 1028))
    if N < 1024:
        assert 2 ** 31 < 4 * n3 < 2 ** 32 <= 16 * n3 and 3 * n3 > 2 ** 31 > 2 * n3           # input: elements, bytes, channel 2
        assert 6 * n3 > 2 ** 32 > 5 * n3                                                     # output: channel 5 crosses 2^32
        assert 6 * (N - 4) ** 3 < 2 ** 32 and 6 * 894 ** 3 < 2 ** 32       # the next smaller N of this store width, and of any
    else:
        assert 4 * n3 > 2 ** 32 > 3 * n3 and 2 * n3 > 2 ** 31 > n3 > 2 ** 30                 # channel 3 crosses 2^32, channel 1 2^31
        assert 4 * (N - 4) ** 3 <= 2 ** 32 == 4 * 1024 ** 3                # the next smaller N of this store width; 1024 fits


def _layouts(K, N):
    """((xchunk, vec) of the gradient launch, of the filter launch) for this device; on 256 CUs the table of the docstring."""
    cus = _cus(K)
    got = (gr.layout(N, cus), fr.layout(N, cus))
    assert cus != 256 or got == LAYOUT_256[N], (N, cus, got)
    assert got[0][1] == got[1][1] == (4 if N % 4 == 0 else 2) and got[1][0] <= fr.XCHUNK_MAX and got[0][0] >= 64, (N, cus, got)
    return got


def _run_case(K, inputs, scheme, N, what, call, mirror):
    """Poison, launch, scan, compare slab by slab; -> the mirror's slabs are dropped as they go.  Prints the wall times."""
    _boundaries(N)
    lay = _layouts(K, N)
    nch = (gr.NCH if scheme == "gradient" else fr.NCH)[what]
    ch, before = inputs.get(scheme, N)
    _need_memory(4 * nch * N ** 3 + 4 * GIB, "%s at N = %d" % (what, N))
    t0 = time.perf_counter()
    out = torch.empty((nch, N, N, N), dtype=torch.float32, device=K.device)
    dr.fill(out, float("nan"))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    got = call(ch, out)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert got.data_ptr() == out.data_ptr()
    nan = dr.count_nan(out)
    t3 = time.perf_counter()
    bad, seen = None, [False, False]
    for x0, x1 in dr.slabs(N):
        ref = mirror(ch, x0, x1)
        if dr.compare(out, ref, x0):
            bad = dr.describe(out, ref, x0)
            break
        if what == "vm":
            seen[0] |= bool((ref[3] == 0).any())
            seen[1] |= bool((ref[3] > 0).any())
        del ref
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    after = dr.checksum(ch)
    del out, got
    torch.cuda.empty_cache()
    t5 = time.perf_counter()
    print("\n[%s N=%d: x chunk %d (gradient) / %d (filter), %d cells per group; poison %.2f s, kernel and sync %.3f s, NaN scan "
          "%.2f s, mirror and compare %.2f s, checksum %.2f s; %.2f s in all]"
          % (what, N, lay[0][0], lay[1][0], lay[0][1], t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t5 - t0), end=" ")
    assert nan == 0, "%s N=%d: %d elements of the output were never written" % (what, N, nan)
    assert bad is None, "%s N=%d: %s" % (what, N, bad)
    assert after == before, "%s N=%d: the input changed" % (what, N)
    if what == "vm":
        assert seen == [True, True], "the M = 0 path and the other one: %r" % (seen,)


@pytest.mark.parametrize("N,what", GRADIENT_CASES)
def test_gradient_kernel_past_2_31_and_2_32_elements(K, inputs, N, what):
    _run_case(K, inputs, "gradient", N, what, lambda ch, out: K.velocity_gradient(ch, N, LCELL, what, out=out),
              lambda ch, x0, x1: dr.gradient_slab(ch, LCELL, what, x0, x1))


@pytest.mark.parametrize("N,what", FILTER_CASES)
def test_filter_kernel_past_2_31_and_2_32_elements(K, inputs, N, what):
    _run_case(K, inputs, "filter", N, what, lambda ch, out: K.box_filter(ch, N, M, what, out=out),
              lambda ch, x0, x1: dr.filter_slab(ch, M, what, x0, x1))


def test_scale_flux_at_896_is_the_composition_of_the_three_kernels(K, inputs):
    """BoxField.scale_flux on a device-backed field of 896^3 cells against flux_contraction of box_filter('stress') and
    velocity_gradient(box_filter('vm'), 'strain_rate') called by hand, value for value (as _check_surface of
    tests/test_gpu_filter.py does at 32): tau and S are tensors of 4.3e9 elements, their channels 2 .. 5 past 2^31."""
    from vpower import device as D
    from vpower import interp
    N = 896
    _boundaries(N)
    ch, before = inputs.get("filter", N)
    _need_memory(4 * (6 + 4 + 6 + 1 + 1) * N ** 3 + 2 * GIB, "scale_flux at N = %d" % N)
    t0 = time.perf_counter()
    t = K.box_filter(ch, N, M, "stress")
    S = K.velocity_gradient(K.box_filter(ch, N, M, "vm"), N, LCELL, "strain_rate")
    want = D.flux_contraction(t, S)
    del t, S
    box = interp.BoxField._from_device(ch, LCELL)
    assert box.Nsize == N and box._gradient_chans(K) is ch
    flux = box.scale_flux(M)
    t1 = time.perf_counter()
    assert flux.shape == (N, N, N) and flux.dtype == np.float32
    differ = 0
    for x0, x1 in dr.slabs(N):
        differ += dr.compare(want[None], torch.from_numpy(flux[None, x0:x1]).to(K.device), x0)
    t2 = time.perf_counter()
    nonzero = int(torch.count_nonzero(want))
    del want
    torch.cuda.empty_cache()
    print("\n[scale_flux N=%d m=%d: both routes %.2f s, compare %.2f s]" % (N, M, t1 - t0, t2 - t1), end=" ")
    # (Pi is 0 only where a box holds no mass: inside the empty cube, 6e-5 of the cells)
    assert differ == 0 and not np.isnan(flux).any() and nonzero > 0.99 * N ** 3
    assert dr.checksum(ch) == before
