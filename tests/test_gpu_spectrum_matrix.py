"""Shell-sum parity of the binning x pass at every FFT size and in every x-pass variant, on generic data, against a reference
that is exact at any N.

The fields are separable random fields of rank 3 (oracle/gpu_checks.py: separable_factors), whose spectrum is a sum of
products of float64 1-D FFTs: `separable_shell_sums` gives the float64 shell sums and counts of the whole grid (or of one
rank's planes) and `separable_plane` every mode, a block of kz planes at a time, at sizes whose float64 3-D spectrum would
not fit a host (tests/test_separable_reference.py pins both to the oracle).  Legs:
  a. every N the device FFT supports is in the matrix;
  b. PowerPipeline.spectrum on the whole grid, both binning flavours, every x-pass variant, counts bit for bit, Psum within
     PSUM_RTOL; a CIC window table at 1024 and 2048;
  c. the x pass in write mode on every line of the grid against every exact mode, Nyquist plane included;
  d. the slab decomposition emulated on one GPU through the production calls (z pass per sender slab, chunked + packed y
     pass, x pass of the received blocks), every receiver -- or, at 4096, one receiver fed by eight senders' slabs;
  e. the rank-count limit of the segmented x pass: 16 ranks work at 1024 and 2048 (leg d), 32 are refused up front."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import gpu_checks as chk  # noqa: E402

PSUM_RTOL = 2e-5   # Psum per bin vs the float64 reference
MODE_RTOL = 1e-5   # per mode: max |got - exact| / rms of the plane, the bar of the thin-slab tests
RANK = 3           # rank of the separable fields: lines are not proportional to each other

BINNED = (16, 32, 64, 96, 128, 192, 250, 256, 384, 500, 512, 768, 1000, 1024, 1536, 2000, 2048)
PER_MODE = (384, 500, 512, 768, 1000, 1024, 1536, 2000, 2048)
WINDOW = (1024, 2048)
SLABS = ((2048, 8, 2), (1536, 8, 2), (2000, 8, 5), (1024, 16, 2), (2048, 16, 2))   # (N, ranks, kz chunks): every receiver
ONE_RECEIVER = ((4096, 8, 4, 3),)                                                  # (N, ranks, kz chunks, receiver)
# (name, options, binning mode it must select: 0 general shell walk, 1 mirrored kx float64, 2 integer shells)
VARIANTS = (("default", {}, 2), ("no_int_binning", {"no_int_binning": 1}, 1), ("no_pair_binning", {"no_pair_binning": 1}, 2),
            ("no_fast_binning", {"no_fast_binning": 1}, 0), ("x_wg_per_cu=1", {"x_wg_per_cu": 1}, 2))


@pytest.fixture(scope="module")
def K():
    from vpower import device
    k = device.default_kernels()
    torch.cuda.reset_peak_memory_stats()
    yield k
    print("\ntest_gpu_spectrum_matrix: peak device memory %.1f GB" % (torch.cuda.max_memory_allocated() / 1e9))


def _free(K):
    K._work.clear()
    torch.cuda.empty_cache()


def _factors(N, ncomp, salt):
    return [chk.separable_factors(N, RANK, seed=1000 * N + 10 * salt + i) for i in range(ncomp)]


def _box(N):
    """Box length 1, or 2.5 where the library flavour's np.arange edges come out inconsistent at L = 1 (N = 96, 768: the
    reference's own binning fails there, as PowerPipeline does; at L = 2.5 the same happens to N = 250, 500, 1000)."""
    from vpower import device
    for L in (1.0, 2.5):
        kmin = 2 * np.pi / L
        try:
            device.bin_edges(kmin, np.pi / (L / N), kmin, "library")     # PowerPipeline's default k range
            return L
        except Exception:
            pass
    raise AssertionError(N)


def _pipeline(K, N, flavour="library", deconvolve=None, comm=None):
    from vpower import device
    return device.PowerPipeline(N, _box(N), kernels=K, comm=comm if comm is not None else device.SlabComm(enabled=False),
                                flavour=flavour, deconvolve=deconvolve)


def _check_table(tab, ref_ps, ref_ns, what):
    assert np.array_equal(tab[:, 3], ref_ns), what
    bad = np.abs(tab[:, 2] - ref_ps) > PSUM_RTOL * np.abs(ref_ps)
    assert not bad.any(), (what, np.nonzero(bad)[0][:8], np.max(np.abs(tab[:, 2] - ref_ps) / np.maximum(ref_ps, 1e-300)))


# ------------------------------------------------------------------------------------------------------ a. size guard ----
def test_matrix_covers_every_supported_size(K):
    sizes = [N for N in range(8, 4097) if K.fft_supported(N)]
    covered = set(BINNED) | set(PER_MODE) | {s[0] for s in SLABS} | {s[0] for s in ONE_RECEIVER}
    assert set(sizes) <= covered, sorted(set(sizes) - covered)
    assert set(BINNED) == {N for N in sizes if N <= 2048}       # leg b: every size up to C4's
    assert set(PER_MODE) == {N for N in sizes if 384 <= N <= 2048}


# --------------------------------------------------------------- b. binned parity on the whole grid, every x-pass variant ----
@pytest.mark.parametrize("N", BINNED)
def test_whole_grid_shell_sums_every_variant(K, N):
    from vpower import _ffi
    ncomp = 3 if N <= 1024 else 1           # three: the fft_x_bin_multi launch of C2 / C4 velocity; one from 1536 on (memory)
    comps = _factors(N, ncomp, 0)
    fields = [chk.separable_slab(K.device, f, 0, N) for f in comps]
    for flavour in ("library", "script"):
        pipe = _pipeline(K, N, flavour)
        counts = chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr)
        ref_ps, ref_ns = chk.separable_shell_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
        assert np.array_equal(ref_ns, counts)
        for name, opts, mode in VARIANTS:
            try:
                for k_, v_ in opts.items():
                    _ffi.set_option(k_, v_)
                pipe.prepare()
                assert K.binning_mode() == mode, (flavour, name, K.binning_mode())
                tab = pipe.finish(*pipe.accumulate(fields))
            finally:
                for k_ in opts:
                    _ffi.set_option(k_, None)
            _check_table(tab, ref_ps, counts, (N, flavour, name))
    if N in WINDOW:                          # 1/W^2 of CIC applied by the x pass (vps_set_window)
        pipe = _pipeline(K, N, "library", deconvolve="cic")
        ref_ps, ref_ns = chk.separable_shell_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr, win=pipe.window)
        _check_table(pipe.finish(*pipe.accumulate(fields)), ref_ps, ref_ns, (N, "cic"))
    del fields
    _free(K)


# ---------------------------------------------------------------------- c. every mode of the x pass at full line length ----
@pytest.mark.parametrize("N", PER_MODE)
def test_every_mode_of_the_write_x_pass(K, N):
    f = _factors(N, 1, 1)[0]
    field = chk.separable_slab(K.device, f, 0, N)
    spec, nyq = K.fft_zy(field, N, N)                    # [N/2][ky][x], [ky][x]
    del field
    _free(K)
    h = N // 2
    out = K.empty((h * N, N), torch.complex64)
    K.fft_x_write(spec, N, h * N, 1, 0, out)             # [kz][ky][kx]
    del spec
    outn = K.empty((N, N), torch.complex64)
    K.fft_x_write(nyq, N, N, 1, 0, outn)
    del nyq
    got = out.view(h, N, N)
    step = max(1, (1 << 24) // (N * N))
    worst = (0.0, -1)
    for k0 in range(0, h + 1, step):
        planes = list(range(k0, min(h + 1, k0 + step)))
        ex = chk.separable_plane(K.device, f, planes)
        g = torch.stack([(got[k] if k < h else outn) for k in planes]).to(torch.complex128)
        rel = (g - ex).abs().amax(dim=(1, 2)) / ex.abs().square().mean(dim=(1, 2)).sqrt()
        i = int(torch.argmax(rel))
        if float(rel[i]) > worst[0]:
            worst = (float(rel[i]), planes[i])
        del ex, g
    assert worst[0] < MODE_RTOL, (N, "kz", worst[1], worst[0])
    del out, outn, got
    _free(K)


# --------------------------------------------------- d. slab decomposition emulated on one GPU, production calls ----
def _nan_buffer(K, n):
    return torch.full((n,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=K.device)


@pytest.mark.parametrize("N,G,C", SLABS)
def test_emulated_slab_exchange_every_receiver(K, N, G, C):
    """vps_fft_z per sender slab -> vps_fft_y chunk by chunk into NaN-filled send buffers, packed rows inside binning_only()
    -> the all-to-all played by slicing -> vps_fft_x_bin_chunk on every receiver; shell sums of all ranks against the exact
    whole-grid reference.  G = 16: the largest rank count the segmented x pass of N = 1024 / 2048 takes."""
    nx = N // G
    f = _factors(N, 1, 2)[0]
    zimgs = []
    for g in range(G):
        slab = chk.separable_slab(K.device, f, g * nx, nx)
        zimgs.append(K.fft_z(slab, N, nx))
        del slab
    pipe = _pipeline(K, N)
    pipe.prepare()
    counts = chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr)
    ref_ps, ref_ns = chk.separable_shell_sums(K.device, [f], N, pipe.Lbox, pipe.k2, pipe.thr)
    assert np.array_equal(ref_ns, counts)
    psum, ns = pipe.new_accumulators()
    for c in range(C):
        with K.binning_only():
            packed = K.y_packed(N)
            blk = K.chunk_block(N, nx, G, C, c, packed)
            sends = [K.fft_y_chunk(z, N, nx, G, C, c, out=_nan_buffer(K, G * blk)) for z in zimgs]
        assert packed
        for h in range(G):
            recv = torch.cat([sends[g][h * blk:(h + 1) * blk] for g in range(G)])
            K.fft_x_bin_chunk([recv], N, nx, G, C, c, h, packed, psum, ns)
            del recv
        del sends
    _check_table(pipe.finish(psum, ns), ref_ps, counts, (N, G, C))
    del zimgs
    _free(K)


@pytest.mark.parametrize("N,G,C,r", ONE_RECEIVER)
def test_emulated_slab_exchange_one_receiver_at_4096(K, N, G, C, r):
    """C5's layout: receiver r of G ranks, each sender's block cut from that sender's OWN slab of the separable field
    (generated and transformed one slab at a time); the receiver's kz planes and Nyquist rows against the exact reference."""
    nx, nky = N // G, N // G
    nkc = N // 2 // G // C
    f = _factors(N, 1, 3)[0]
    pipe = _pipeline(K, N)
    pipe.prepare()
    kept = [[None] * G for _ in range(C)]              # kept[c][g]: sender g's block for receiver r in chunk c
    packed = None
    for g in range(G):
        slab = chk.separable_slab(K.device, f, g * nx, nx)
        z = K.fft_z(slab, N, nx)
        del slab
        for c in range(C):
            with K.binning_only():
                packed = K.y_packed(N)
                blk = K.chunk_block(N, nx, G, C, c, packed)
                out = K.fft_y_chunk(z, N, nx, G, C, c, out=_nan_buffer(K, G * blk))
            kept[c][g] = out[r * blk:(r + 1) * blk].clone()
            del out
        del z
        _free(K)
    assert packed
    psum, ns = pipe.new_accumulators()
    for c in range(C):
        recv = torch.cat(kept[c])
        kept[c] = None
        K.fft_x_bin_chunk([recv], N, nx, G, C, c, r, packed, psum, ns)
        del recv
    tab = pipe.finish(psum, ns)
    planes = [c * G * nkc + j * G + r for c in range(C) for j in range(nkc)] + [N // 2]
    ref_ps, ref_ns = chk.separable_shell_sums(K.device, [f], N, pipe.Lbox, pipe.k2, pipe.thr, kz=planes,
                                              nyq_ky=(r * nky, (r + 1) * nky))
    _check_table(tab, ref_ps, ref_ns, (N, G, C, r))
    _free(K)


# ------------------------------------------------------------------------------------- e. the rank-count limit ----
def test_more_ranks_than_the_x_pass_takes_are_refused_up_front(K):
    """32 ranks at N = 1024, 2048, 4096 (segments of 32, 64, 128 points, shorter than the plans' 64, 128, 256 lanes per line):
    PowerPipeline refuses them when it is built, and vps_fft_x_bin_chunk at its entry -- no x-pass kernel runs.  (Leg d runs
    16 ranks at 1024 and 2048 through the same calls.)"""
    from vpower import device, _ffi
    for N in (1024, 2048, 4096):
        G = 2 * device.x_max_ranks(N)
        assert G == 32
        comm = device.SlabComm(enabled=False)
        comm.world, comm.rank = G, 0
        with pytest.raises(Exception, match="at most 16 ranks"):
            _pipeline(K, N, comm=comm)
        pipe = _pipeline(K, N)
        pipe.prepare()
        psum, ns = pipe.new_accumulators()
        recv = K.zeros((16,), torch.complex64)        # never read: the call is refused before anything is enqueued
        K.timing(True)
        try:
            with pytest.raises(_ffi.VpsError, match="at most 16 ranks"):
                K.fft_x_bin_chunk([recv], N, N // G, G, 1, 0, 0, False, psum, ns)
            K.sync()
            assert len(K.timing_list("fft_x")) == 0
        finally:
            K.timing(False)
        assert not psum.any() and not ns.any()
