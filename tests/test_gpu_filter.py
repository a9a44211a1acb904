"""The box-filter codes of vps_field_algebra_out (VPS_FILTERED_VM = 16, VPS_FILTERED_STRESS = 17: csrc/filter.hip) against the
references of tests/filter_ref.py: bit equal on exact inputs at every tile and chunk shape; impulses at the corners and faces;
random fields within the derived bar; on guarded memory; behind a busy side stream; their refusals; and the public surface,
BoxField.filtered / subfilter_stress / scale_flux / scale_flux_profile.  Every case fails on a library without the codes
("vps_field_algebra: quantity 16").
Run on an MI355X:  python -m pytest tests/test_gpu_filter.py -q -m gpu -s"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import filter_ref as fr  # noqa: E402
import gradient_ref as gr  # noqa: E402
import guarded as gd  # noqa: E402
import stream_probe as sp  # noqa: E402

WHATS = ("vm", "stress")
CACHE = {}


@pytest.fixture(scope="module")
def K():
    from vpower import device
    yield device.default_kernels()
    CACHE.clear()


def _cus(K):
    """The CU count the launch sizes its x chunks by (vps_device_info), for the chunk layout of tests/filter_ref.py: bars."""
    info = (ctypes.c_int64 * 4)()
    assert K.lib.vps_device_info(K.ctx, info) == 0
    return int(info[0])


def _dev(K, ch):
    return torch.from_numpy(np.ascontiguousarray(ch, dtype=np.float32)).to(K.device)


# ------------------------------------------------------------------ exact inputs ----
@pytest.mark.parametrize("N,m", [(4, 1), (6, 1), (6, 2), (16, 1), (18, 8), (34, 8), (64, 4), (96, 8), (250, 1), (250, 8)])
def test_bit_equal_on_exact_inputs(K, N, m):
    """Integer velocities |u| <= 3, masses in {0, 1, 2} with a cube of empty cells that holds whole boxes (M = 0): every box sum
    is an integer below 2^24 (17^3 * 2 * 9 < 2^17), exact in any order of additions, and the product P_i P_j, the division, the
    subtraction, the clamp and the scaling are single float32 roundings in the header's order: the kernel and the float32 mirror
    agree bit for bit.  4, 6, 18 and 34 are N = 2m + 2; 4 .. 34 are below one 64-cell tile; 6, 18, 34 and 250 have N % 4 = 2
    (8-byte stores, 32-cell tiles); 34, 96 and 250 leave remainder tiles in y and in z; 96 and 250 have more than one x chunk,
    and so has (64, 4): the launch takes chunks of at most 64 planes and, where the tiles are few, of no less than 32 -- N / 32
    chunks at most -- so 64 planes with four tiles are marched as two chunks of 32 and the running sum restarts at x = 32."""
    ch = fr.integer_chans(N, seed=100 * N + m)
    d = _dev(K, ch)
    keep = d.clone()
    refs = fr.fields32_all(ch, m)
    for what in WHATS:
        ref = refs[what]
        got = K.box_filter(d, N, m, what)
        assert got.shape == (fr.NCH[what], N, N, N) and got.dtype == torch.float32
        got = got.cpu().numpy()
        assert np.array_equal(got, ref), "%s N=%d m=%d: %d elements differ" % (what, N, m, int(np.sum(got != ref)))
        assert np.abs(ref).max() > 0
        if what == "vm":
            assert (ref[3] == 0).any() and (ref[3] > 0).any()                  # the M = 0 path ran, and the other one
    assert torch.equal(d, keep)                                                # the input is only read


@pytest.mark.parametrize("m", [1, 3])
def test_impulses_at_corners_and_face_centres(K, m):
    """One unit-mass cell with u = (1, 2, 3) at each of the 8 corners and the 6 face centres of a 16^3 grid: u~ = (1, 2, 3) and
    mbar = c exactly on the wrapped box around it and 0 elsewhere; the stress is 0 everywhere (one cell has no dispersion)."""
    N = 16
    h = N // 2
    corners = [(x, y, z) for x in (0, N - 1) for y in (0, N - 1) for z in (0, N - 1)]
    faces = [(0, h, h), (N - 1, h, h), (h, 0, h), (h, N - 1, h), (h, h, 0), (h, h, N - 1)]
    c = np.float32(1.0 / (2 * m + 1) ** 3)
    ch = torch.zeros((4, N, N, N), dtype=torch.float32, device=K.device)
    for p in corners + faces:
        for a in range(3):
            ch[(a,) + p] = a + 1.0
        ch[(3,) + p] = 1.0
        mask = fr.impulse_expect(p, m, N)
        vm = K.box_filter(ch, N, m, "vm").cpu().numpy()
        for a in range(3):
            assert np.array_equal(vm[a], np.where(mask, np.float32(a + 1), np.float32(0))), (p, a)
        assert np.array_equal(vm[3], np.where(mask, c, np.float32(0))), p
        assert not K.box_filter(ch, N, m, "stress").cpu().numpy().any(), p
        ch[(slice(None),) + p] = 0.0


# ------------------------------------------------------------------ random fields ----
@pytest.mark.parametrize("N,m", [(64, 1), (64, 4), (64, 8), (96, 1), (96, 4), (96, 8)])
def test_random_fields_within_the_derived_bar(K, N, m):
    """Every channel within the per-cell bar of tests/filter_ref.py: bars -- K 2^-24 max sum_W |terms| of each box sum, the
    maximum over the window sums the sliding sums have passed through when the cell is written (the cells x' <= x of its x chunk
    and z' <= z of its group of four), carried through the quotient (u~), and through the product, the quotient and the
    subtraction (tau) -- of the float64 reference.  K = 6m + 134 is the longest rounding chain of the kernel as built
    (csrc/filter.hip): 2 roundings in a product p_i u_j; 2m additions of the direct z sum and 2 * 3 of the sliding steps in a
    group of four cells; 2m additions of the direct x sum at the start of a chunk and 2 per plane for the at most 63 further
    planes of a chunk; 2m additions along y."""
    rng = np.random.default_rng(1000 * N + m)
    ch = (rng.standard_normal((4, N, N, N)) + np.array([2.0, -1.0, 0.5, 0.0])[:, None, None, None]).astype(np.float32)
    ch[3] = np.exp(0.5 * rng.standard_normal((N, N, N))).astype(np.float32)
    d = _dev(K, ch)
    for what in WHATS:
        got = K.box_filter(d, N, m, what).double().cpu().numpy()
        ref, bar = fr.fields64(ch, m, what), fr.bars(ch, m, what, num_cu=_cus(K))
        worst = float(np.max(np.abs(got - ref) / bar))
        print("%s N=%d m=%d: worst error %.4f of the bar (K = %d)" % (what, N, m, worst, fr.chain(m)))
        assert np.isfinite(got).all() and np.isfinite(bar).all() and worst <= 1.0, (what, N, m, worst)


def _against_bars(K, ch, m, label):
    """Both codes of the float field ch against the float64 reference: exact zeros in every box without mass, every other cell
    within its bar (inf where the bar claims nothing of a quotient); -> the fraction of cells with a finite bar per code."""
    N = ch.shape[1]
    d = _dev(K, ch)
    empty = fr.count(ch, m) == 0
    finite = {}
    for what in WHATS:
        got = K.box_filter(d, N, m, what).double().cpu().numpy()
        ref, bar = fr.fields64(ch, m, what), fr.bars(ch, m, what, num_cu=_cus(K))
        assert not got[:, empty].any() and not np.signbit(got[:, empty]).any(), "%s %s: an empty box is not exactly 0" % (label, what)
        assert np.isfinite(got).all(), (label, what)
        err = np.abs(got - ref)
        assert np.all(err <= bar), "%s %s: worst %.3g of the bar" % (label, what, float(np.max(err[bar > 0] / bar[bar > 0])))
        fin = np.isfinite(bar) & ~empty[None]
        finite[what] = float(fin.mean())
        print("%s %s: worst error %.4f of the bar over the %.3f of the cells with a finite, nonzero bar; %.3f of the boxes empty"
              % (label, what, float(np.max(err[fin] / bar[fin])), finite[what], float(empty.mean())))
    return finite


@pytest.mark.parametrize("N,m", [(64, 2), (96, 4), (34, 1)])
def test_voids_wider_than_the_box_are_exactly_zero(K, N, m):
    """A float field (velocity mean 2, log-normal mass) with mass only in slabs along x, along y and along z, the rest empty: a
    box that leaves the mass behind along x (inside a chunk) or along z (inside a group of cells) carries the rounding residue
    of what left in its float sums of M and P, and only the exact count of cells with mass tells that it is empty.  Every
    channel of both codes is exactly 0 (and not -0) in every such box; next to the voids every cell is within its bar.
    (34: 8-byte groups of two cells.)"""
    rng = np.random.default_rng(50 * N + m)
    ch = (rng.standard_normal((4, N, N, N)) + np.array([2.0, 2.0, 2.0, 0.0])[:, None, None, None]).astype(np.float32)
    mass = np.exp(0.5 * rng.standard_normal((N, N, N))).astype(np.float32)
    keep = np.zeros((N, N, N), dtype=bool)
    q = N // 4
    keep[2:q] = True                    # massive planes, then a void along x that the chunk marches into
    keep[:, 1:3, :] = True              # a thin sheet in y
    keep[q + 1, :, 5:7] = True          # and a bar that leaves the box along z inside a group
    keep[3 * q:, 3 * q:, 3 * q:] = False
    ch[3] = np.where(keep, mass, 0)
    empty = fr.count(ch, m) == 0
    assert 0.05 < empty.mean() < 0.95
    finite = _against_bars(K, ch, m, "voids N=%d m=%d" % (N, m))
    assert all(abs(f - (1.0 - empty.mean())) < 1e-12 for f in finite.values())      # a finite bar in every box that holds mass


@pytest.mark.parametrize("N,m", [(64, 4), (96, 2)])
def test_strong_contrast_within_the_true_bar_and_the_chunks_restart(K, N, m):
    """Mass 1e6 times larger in the planes x = 20, 21 than elsewhere.  While the heavy planes are in the box the sums are
    relative to them; after they have left, the running x sum keeps their rounding residue until the chunk ends -- the bar of
    those cells is made of the heavy window sum (tests/filter_ref.py: chain_max) and claims nothing of a quotient where the
    residue may exceed half of M.  A NEW chunk starts from a direct sum: from its first plane whose box no longer holds the
    heavy planes the bars are those of a smooth field again, finite everywhere, and the kernel has to meet them -- which it
    does only if the launch really took the chunks of filter_ref.layout (for N = 64: two chunks of 32 planes; asserted)."""
    rng = np.random.default_rng(70 * N + m)
    ch = (rng.standard_normal((4, N, N, N)) + np.array([2.0, -1.0, 0.5, 0.0])[:, None, None, None]).astype(np.float32)
    ch[3] = np.exp(0.5 * rng.standard_normal((N, N, N))).astype(np.float32)
    ch[3, 20:22] *= np.float32(1e6)
    xchunk, _ = fr.layout(N, _cus(K))
    assert xchunk == 32 and 21 + m + 1 < xchunk
    _against_bars(K, ch, m, "contrast N=%d m=%d" % (N, m))
    for what in WHATS:
        bar = fr.bars(ch, m, what, num_cu=_cus(K))
        tail = bar[:, 21 + m + 1:xchunk]                      # the heavy planes have left, the chunk goes on: the residue stays
        fresh = bar[:, xchunk:N - m]                          # the next chunks: no heavy plane in any box they pass
        assert np.isfinite(fresh).all(), what
        assert np.mean(~np.isfinite(tail) | (tail > 1e3 * np.median(fresh))) > 0.9, what


# ------------------------------------------------------------------ guarded memory ----
@pytest.mark.parametrize("N,m", [(16, 1), (250, 8)])
def test_guarded_exact_size_buffers(K, N, m):
    """The four input channels are exactly 16 N^3 bytes and the output exactly 4 NCH N^3 poisoned bytes, each between 1 MiB
    guards (tests/guarded.py): no guard is touched, no output element keeps the poison, and the fields are the exact ones."""
    ch = fr.integer_chans(N, seed=7000 + N)
    refs = fr.fields32_all(ch, m)
    G = gd.guarded_kernels()
    try:
        d = G.empty((4, N, N, N), torch.float32)
        d.copy_(torch.from_numpy(ch))
        for what in WHATS:
            got = G.box_filter(d, N, m, what)
            torch.cuda.synchronize()
            rep = G.check()
            assert gd.guard_findings(rep) == [], (what, gd.guard_findings(rep))
            out = gd.report_of(rep, got)
            assert out.nbytes == 4 * fr.NCH[what] * N ** 3 and len(out.poison) == 0, (what, out)
            assert np.array_equal(got.cpu().numpy(), refs[what]), what
            if what == WHATS[0]:
                assert gd.report_of(rep, d).nbytes == 16 * N ** 3
    finally:
        G.release()
        G.close()
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ stream contract ----
@pytest.mark.parametrize("what", WHATS)
def test_side_stream_behind_the_blocker(K, what):
    """box_filter on a side stream behind the blocker of tests/stream_probe.py, the true channels swapped in on that stream: the
    call returns with the blocker pending and gives the bits of the reference of the TRUE data."""
    N, m = 64, 2
    if "blocker" not in CACHE:
        CACHE["blocker"] = sp.Blocker(K.device)
    chs = [fr.integer_chans(N, seed=s) for s in (21, 22)]                    # true, decoy
    refs = [[fr.fields32(ch, m, what)] for ch in chs]
    true, decoy = _dev(K, chs[0]), _dev(K, chs[1])
    bufs = [decoy.clone()]
    case = sp.Case("box_filter-%s" % what, bufs, [true], lambda: [K.box_filter(bufs[0], N, m, what)],
                   refs[0], refs[1], ["exact"])
    sp.run_case(case, CACHE["blocker"])


# ------------------------------------------------------------------ refusals ----
def test_refusals_name_the_quantity_and_enqueue_nothing(K):
    from vpower import _ffi
    from vpower import device as D
    lib = K.lib
    N, L, n, lc = 32, 1.0, 1000, 0.5
    rng = np.random.default_rng(0)
    pos = K.to_device(rng.random((n, 3)).astype(np.float32))
    vel = K.to_device(rng.standard_normal((n, 3)).astype(np.float32))
    rho = K.to_device((rng.random(n) + 0.5).astype(np.float32))
    rhov = K.density_velocity_vector(vel, rho)
    host = fr.integer_chans(N, seed=3)
    chans = _dev(K, host)
    chans0 = chans.clone()
    nan = float("nan")
    big = torch.full((10, N, N, N), nan, dtype=torch.float32, device=K.device)
    out = big[:6]
    spec = torch.full((3, N // 2, N, N, 2), nan, dtype=torch.float32, device=K.device)
    nyq = torch.full((3, N, N, 2), nan, dtype=torch.float32, device=K.device)
    zimg = torch.full((4 * K.zimage_elems(N, N), 2), nan, dtype=torch.float32, device=K.device)
    work = K.workspace("refusals", max(lib.vps_deposit_assign_workspace_bytes(n, 4, N, 3), lib.vps_deposit_fft_zy_workspace_bytes_shared(n, N, N),
                                       lib.vps_nn_workspace_bytes(n, 0, N ** 3), lib.vps_deposit_workspace_bytes(n, 4, N, N)))
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731
    ax = np.ascontiguousarray((np.arange(N) + 0.5) / N)
    names = {D.FILTERED_VM: "VPS_FILTERED_VM", D.FILTERED_STRESS: "VPS_FILTERED_STRESS"}
    assert sorted(names) == [16, 17]
    VM, F = D.FLAG_INPUT_IS_VM, D.FLAG_FILTER
    K._stream()

    def refused(rc, q, code=-1):
        msg = lib.vps_last_error(K.ctx).decode()
        assert rc == code and "quantity %d" % q in msg and names[q] in msg, (q, rc, msg)
        torch.cuda.synchronize()
        for buf in (big, spec, nyq, zimg):
            assert bool(torch.isnan(buf).all()), "a refused call wrote something"
        assert torch.equal(chans, chans0)
        return msg

    for q, name in names.items():
        nch = D.NCOMP[q]
        ok = VM | F(2)
        assert lib.vps_deposit_fft_zy_supported(K.ctx, N, q) == 0 and lib.vps_deposit_fft_zy_supported(K.ctx, 64, q) == 0
        # the in-place form, a null out_dev, a null chans_dev
        refused(lib.vps_field_algebra(K.ctx, q, ok, lc, p(chans), N ** 3), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, p(chans), N ** 3, None), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, None, N ** 3, p(out)), q)
        # overlapping buffers: the output starting inside the channels, the channels starting inside the output, the same buffer
        refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, p(chans), N ** 3, p(chans, 4 * 3 * N ** 3)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, p(big, 4 * (nch - 1) * N ** 3), N ** 3, p(big)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, p(chans), N ** 3, p(chans)), q)
        # buffers off the 16-byte boundary (either one)
        refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, p(chans, 8), N ** 3, p(out)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, p(chans), N ** 3, p(out, 4)), q)
        # without VPS_FLAG_INPUT_IS_VM; any flag bit other than it and the filter field; m = 0
        for flags in (F(2), 0, ok | D.FLAG_REFERENCE_MOMENTUM_BUG, ok | D.FLAG_REUSE_SORT, ok | D.FLAG_SHARE_ENERGY, ok | 0x10, ok | 0x70,
                      ok | D.FLAG_ASSIGN("cic"), ok | D.FLAG_ASSIGN("tsc"), ok | 0x300, ok | 0x400, ok | 0x800, ok | 0x1000000,
                      ok | (1 << 30), VM, VM | F(0)):
            refused(lib.vps_field_algebra_out(K.ctx, q, flags, lc, p(chans), N ** 3, p(out)), q)
        # 2m + 1 > N (at N = 32 only beyond the kernel's plan, so on a 4^3 and a 16^3 grid as well)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM | F(16), lc, p(chans), N ** 3, p(out)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM | F(2), lc, p(chans), 4 ** 3, p(out)), q)
        refused(lib.vps_field_algebra_out(K.ctx, q, VM | F(8), lc, p(chans), 16 ** 3, p(out)), q)
        # an ncell that is not the cube of an even N >= 4
        for ncell in (N ** 3 - 4, N ** 3 + 4, N ** 3 - 1, 2 * N * N, 8, 27, 125, 31 ** 3, 0, -64):
            refused(lib.vps_field_algebra_out(K.ctx, q, ok, lc, p(chans), ncell, p(out)), q)
        for bad_lc in (0.0, -0.5, float("nan"), float("inf")):
            refused(lib.vps_field_algebra_out(K.ctx, q, ok, bad_lc, p(chans), N ** 3, p(out)), q)
        # beyond the LDS plan: VPS_ERR_UNSUPPORTED, and the message names the largest half-width taken
        for mm in (9, 12, 15):
            msg = refused(lib.vps_field_algebra_out(K.ctx, q, VM | F(mm), lc, p(chans), N ** 3, p(out)), q, code=-3)
            assert "largest half-width taken is 8" in msg
        # every other entry point that takes a quantity
        refused(lib.vps_nn_resample_quantity(K.ctx, p(pos), 0, p(rhov), n, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N, _ffi.as_dp(ax), N,
                                             0, N, L / N, q, 0, p(out), None, p(work)), q)
        refused(lib.vps_deposit_fft_zy(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(spec), p(nyq), p(work)), q)
        refused(lib.vps_deposit_fft_z(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        refused(lib.vps_deposit_fft_z_slab(K.ctx, p(pos), 0, p(vel), p(rho), n, n, N, L, 0, N, q, 0, p(zimg), p(work)), q)
        for flags in (0, VM, ok, D.FLAG_ASSIGN("cic")):
            refused(lib.vps_deposit_field(K.ctx, p(pos), 0, p(vel), p(rho), n, N, L, 0, N, q, flags, p(out), p(work)), q)
        # ... and the context is usable: an exact call right after gives the right answer
        what = {16: "vm", 17: "stress"}[q]
        for mm in (2, 8):
            assert np.array_equal(K.box_filter(chans, N, mm, what).cpu().numpy(), fr.fields32(host, mm, what))
    # the existing refusals stay: 15 is no quantity, the gradient codes take VPS_FLAG_INPUT_IS_VM alone
    rc = lib.vps_field_algebra_out(K.ctx, 15, VM, lc, p(chans), N ** 3, p(out))
    assert rc == -1 and "quantity 15" in lib.vps_last_error(K.ctx).decode()
    rc = lib.vps_field_algebra_out(K.ctx, 18, VM | F(1), lc, p(chans), N ** 3, p(out))
    assert rc == -1 and "quantity 18" in lib.vps_last_error(K.ctx).decode()
    for flags in (VM | F(1), VM | 0x400):
        rc = lib.vps_field_algebra_out(K.ctx, D.STRAIN_RATE, flags, lc, p(chans), N ** 3, p(out))
        assert rc == -1 and "VPS_STRAIN_RATE" in lib.vps_last_error(K.ctx).decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(big).all()) and torch.equal(chans, chans0)
    with pytest.raises(ValueError, match="contiguous"):
        K.box_filter(chans, N, 1, "stress", out=big[:6, :, :, ::2])


# ------------------------------------------------------------------ public surface ----
def _particles(N, L, n, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) * L).astype(np.float32)
    vel = (rng.standard_normal((n, 3)) + np.array([1.0, -2.0, 0.5])).astype(np.float32)
    dens = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    return pos, vel, dens


def _host_chans(box):
    return np.stack([box.vx, box.vy, box.vz, box.mass]).astype(np.float32)


def _check_surface(K, box, label):
    N, m = box.Nsize, 2
    k = K
    ch_dev = box._gradient_chans(k)
    ch = ch_dev.cpu().numpy()
    f = box.filtered(m)
    got_vm = f._chans.cpu().numpy()
    assert type(f) is type(box) and f.Nsize == N and f.Lcell == box.Lcell and got_vm.shape == (4, N, N, N)
    assert np.all(np.abs(got_vm - fr.fields64(ch, m, "vm")) <= fr.bars(ch, m, "vm", num_cu=_cus(K))), label
    tau = box.subfilter_stress(m)
    assert tau.shape == (6, N, N, N) and tau.dtype == np.float32
    assert np.all(np.abs(tau - fr.fields64(ch, m, "stress")) <= fr.bars(ch, m, "stress", num_cu=_cus(K))), label
    assert f.spctrm("velocity") is not None
    assert f.divergence().shape == (N, N, N)
    # scale_flux is the composition of the three kernels, bit for bit
    from vpower import device as D
    t = k.box_filter(ch_dev, N, m, "stress")
    S = k.velocity_gradient(k.box_filter(ch_dev, N, m, "vm"), N, box.Lcell, "strain_rate")
    want = D.flux_contraction(t, S).cpu().numpy()
    flux = box.scale_flux(m)
    assert flux.shape == (N, N, N) and flux.dtype == np.float32 and np.array_equal(flux, want), label
    prof = box.scale_flux_profile([1, m])
    assert prof.shape == (2, 3) and prof.dtype == np.float64
    assert prof[1, 0] == (2 * m + 1) * box.Lcell and prof[0, 0] == 3 * box.Lcell
    assert prof[1, 1] == np.mean(flux.astype(np.float64)) or abs(prof[1, 1] - flux.astype(np.float64).mean()) <= 1e-12 * abs(flux).max()
    assert abs(prof[1, 2] - np.sqrt(np.mean(flux.astype(np.float64) ** 2))) <= 1e-10 * abs(flux).max()
    print("%s: mean Pi_l %.6g, rms %.6g at l = %g" % (label, prof[1, 1], prof[1, 2], prof[1, 0]))


def test_surface_on_every_kind_of_field(K):
    from vpower import interp
    N, L = 32, 2.0
    pos, vel, dens = _particles(N, L, 60_000, seed=5)
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    rng = np.random.default_rng(6)
    v = rng.standard_normal((N, N, N, 3)).astype(np.float32).astype(np.float64)
    mass = (rng.random((N, N, N)) + 0.5).astype(np.float32).astype(np.float64)
    _check_surface(K, interp.BoxField(v, mass, L / N), "host-built")
    _check_surface(K, gp.ann_interp_to_field(N), "neighbour-backed")
    box = gp.deposit_to_field(N)
    _check_surface(K, box, "particle-backed")
    assert box.subgrid_stress().shape == (6, N, N, N)                     # the particles are kept


def test_filtered_sparse_ngp_field_has_a_velocity_wherever_the_box_holds_mass(K):
    """A sparse NGP deposit (three quarters of the cells empty, and a corner cube without any particle): after filtered(2) a cell
    has a nonzero velocity exactly where its box holds a particle -- decided by the integer count of the reference, not by the
    sign of the filtered mass -- and is exactly 0 in all four channels where it holds none."""
    from vpower import interp
    N, L = 32, 1.0
    pos, vel, dens = _particles(N, L, 8000, seed=8)
    inside = np.all(pos < 0.375 * L, axis=1)                               # a 12^3 cube of cells without particles
    pos, vel, dens = pos[~inside], vel[~inside], dens[~inside]
    gp = interp.GasParticles(pos, dens * (L / N) ** 3, dens, vel, L)
    box = gp.deposit_to_field(N)
    ch = box._gradient_chans(K).cpu().numpy()
    assert (ch[3] == 0).mean() > 0.5
    f = box.filtered(2)._chans.cpu().numpy()
    holds = fr.count(ch, 2) != 0
    assert 0.01 < (~holds).mean() < 0.2
    assert np.all(np.any(f[:3, holds] != 0, axis=0)) and np.all(f[3, holds] > 0)
    assert not f[:, ~holds].any()


def test_law_of_total_variance_on_the_device(K):
    """96 -> 32, w = 3, one particle at every fine-cell centre: tau of the coarse deposit (subgrid_stress at N = 32) equals
    w^3 sum_W tau_fine + w^6 tau_l at the box centres, tau_fine = subgrid_stress at N = 96 (zero: one particle per cell) and
    tau_l = subfilter_stress(1) of the 96^3 field.  Bar per coarse cell and component: the sum of the derived bars of the three
    features -- the coarse deposit's (n + 8) 2^-24 (A_ii + A_jj) / 2 vol_c (tests/stress_ref.py: bars, n = 27), the fine
    deposit's (exactly 0 here: one contribution per cell) and w^6 times the filter's (tests/filter_ref.py: bars, K = 140 and 8
    more: the filter's inputs are the fine deposit's float32 channels, u_c = P_c / R by a hardware reciprocal and a product, 3
    roundings at most, and mass = R vol, 2; a term mass u_i u_j carries them once each: 2 + 3 + 3)."""
    from vpower import interp
    import stress_ref as sref
    Nf, w, L = 96, 3, 3.0
    Nc, lf = Nf // w, L / Nf
    g = ((np.arange(Nf) + 0.5) * lf).astype(np.float32)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(11)
    vel = (rng.standard_normal(pos.shape) + np.array([1.0, -0.5, 0.25])).astype(np.float32)
    dens = (rng.random(len(pos)) + 0.5).astype(np.float32)
    gp = interp.GasParticles(pos, dens * lf ** 3, dens, vel, L)
    fine, coarse = gp.deposit_to_field(Nf), gp.deposit_to_field(Nc)
    tau_c, tau_f = coarse.subgrid_stress().astype(np.float64), fine.subgrid_stress().astype(np.float64)
    tau_l = fine.subfilter_stress(1).astype(np.float64)
    ch = fine._gradient_chans(K).cpu().numpy()
    centre = (slice(None), slice(1, None, w), slice(1, None, w), slice(1, None, w))
    rebuilt = w ** 3 * fr.box_sum(tau_f, 1)[centre] + w ** 6 * tau_l[centre]
    mc = sref.moments(pos, vel, dens, Nc, L)
    bar = sref.bars(mc, (L / Nc) ** 3) + w ** 6 * fr.bars(ch, 1, "stress", num_cu=_cus(K), extra=8)[centre]
    worst = float(np.max(np.abs(rebuilt - tau_c) / bar))
    print("law of total variance 96 -> 32: worst %.4f of the summed bars; max |tau_c| %.4g" % (worst, np.abs(tau_c).max()))
    assert not tau_f.any() and np.abs(tau_c).max() > 0 and worst <= 1.0
