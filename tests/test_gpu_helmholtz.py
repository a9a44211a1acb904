"""The Helmholtz decomposition on the device (vps_fft_x_bin_helmholtz, vps_fft_x_bin_chunk_helmholtz, PowerPipeline.*_helmholtz,
BoxField.helmholtz_spctrm, parallel_optimized.py --helmholtz) against the float64 references of tests/helmholtz_ref.py.

Legs (modelled on tests/test_gpu_spectrum_matrix.py):
  a. every N of that module's BINNED list has a leg here;
  b. whole-grid tables of separable fields at every N, both flavours, every binning variant (mode asserted), against the
     full-spectrum separable reference: counts bit for bit, Psum of total and compressive within 2e-5, the solenoidal
     difference within 2e-5 of the total; a CIC window at 1024;
  c. gradient and curl fields at 512: the part that must vanish is <= 1e-5 of the total per shell;
  d. the slab exchange emulated on one GPU through the production chunk calls, every receiver; 32 ranks and LibraryComm
     refused before anything is enqueued;
  e. BoxField.helmholtz_spctrm on particle-, grid- and neighbour-backed fields against spctrm;
  f. the CLI with --helmholtz."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import helmholtz_ref as hr  # noqa: E402
from oracle import gpu_checks as chk  # noqa: E402
from test_gpu_spectrum_matrix import BINNED, VARIANTS, _box  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSUM_RTOL = 2e-5
RANK = 3
WINDOW = (1024,)
SLABS = ((512, 4, 2), (2048, 8, 2), (1024, 16, 2))     # (N, ranks, kz chunks): every receiver
HELM_N = BINNED
TOTAL_RTOL = 1e-7  # total of the decomposition vs the plain spectrum of the same grid (float32 contraction order, see leg b)


@pytest.fixture(scope="module")
def K():
    from vpower import device
    k = device.default_kernels()
    yield k


def _free(K):
    K._work.clear()
    torch.cuda.empty_cache()


def _factors(N, salt):
    return [chk.separable_factors(N, RANK, seed=7000 * N + 10 * salt + i) for i in range(3)]


def _pipeline(K, N, flavour="library", deconvolve=None, comm=None):
    from vpower import device
    return device.PowerPipeline(N, _box(N), kernels=K, comm=comm if comm is not None else device.SlabComm(enabled=False),
                                flavour=flavour, deconvolve=deconvolve)


def _check(tabs, ref, what):
    ps_t, ps_c, ns = ref
    tot, comp, sol = tabs
    for t in tabs:
        assert np.array_equal(t[:, 3], ns), what
    for t, r, name in ((tot, ps_t, "total"), (comp, ps_c, "compressive")):
        bad = np.abs(t[:, 2] - r) > PSUM_RTOL * np.abs(r)
        assert not bad.any(), (what, name, np.nonzero(bad)[0][:8], np.max(np.abs(t[:, 2] - r) / np.maximum(np.abs(r), 1e-300)))
    bad = np.abs(sol[:, 2] - (ps_t - ps_c)) > PSUM_RTOL * ps_t
    assert not bad.any(), (what, "solenoidal", np.nonzero(bad)[0][:8])


def _spectra(K, comps, N):
    """z/y passes of the three separable fields one at a time (a 2048^3 field is freed before the next is made)."""
    spec = K.empty((3, N // 2, N, N), torch.complex64)
    nyq = K.empty((3, N, N), torch.complex64)
    for i, f in enumerate(comps):
        field = chk.separable_slab(K.device, f, 0, N)
        K.fft_zy(field, N, N, spec=spec[i], nyq=nyq[i])
        del field
    _free(K)
    return spec, nyq


# ------------------------------------------------------------------------------------------------------ a. size guard ----
def test_every_binned_size_has_a_leg(K):
    sizes = [N for N in range(8, 2049) if K.fft_supported(N)]
    assert set(HELM_N) == set(sizes), sorted(set(sizes) ^ set(HELM_N))
    assert {s[0] for s in SLABS} <= set(sizes)


# --------------------------------------------------------------- b. whole grid, both flavours, every x-pass variant ----
@pytest.mark.parametrize("N", HELM_N)
def test_whole_grid_decomposition_every_variant(K, N):
    from vpower import _ffi
    comps = _factors(N, 0)
    spec, nyq = _spectra(K, comps, N)
    for flavour in ("library", "script"):
        pipe = _pipeline(K, N, flavour)
        ref = hr.separable_helmholtz_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
        assert np.array_equal(ref[2], chk.shell_counts_exact(K.device, N, pipe.k2, pipe.thr))
        for name, opts, mode in VARIANTS:
            try:
                for k_, v_ in opts.items():
                    _ffi.set_option(k_, v_)
                pipe.prepare()
                assert K.binning_mode() == mode, (flavour, name, K.binning_mode())
                tabs = pipe.finish_helmholtz(*pipe.accumulate_spectra_helmholtz(spec, nyq))
            finally:
                for k_ in opts:
                    _ffi.set_option(k_, None)
            _check(tabs, ref, (N, flavour, name))
            # the total is what the plain vector launch bins: the same |F|^2 sums up to float32 rounding (the decomposition
            # is a kernel of its own, whose float32 multiply-adds the compiler may contract differently; measured ~1e-9)
            if name == "default":
                plain = pipe.finish(*pipe.accumulate_spectra(spec, nyq))
                assert np.array_equal(plain[:, 3], tabs[0][:, 3])
                assert np.allclose(plain[:, 2], tabs[0][:, 2], rtol=TOTAL_RTOL, atol=0), (N, flavour)
    if N in WINDOW:
        pipe = _pipeline(K, N, "library", deconvolve="cic")
        ref = hr.separable_helmholtz_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr, win=pipe.window)
        _check(pipe.finish_helmholtz(*pipe.accumulate_spectra_helmholtz(spec, nyq)), ref, (N, "cic"))
    del spec, nyq
    _free(K)


# -------------------------------------------------------------------------------- c. gradient and curl fields ----
@pytest.mark.parametrize("kind", ["gradient", "curl"])
def test_gradient_and_curl_fields_at_512(K, kind):
    N, L = 512, 1.0
    # built spectrally on the device: F = i k' phi_hat (gradient) or i k' x A_hat (curl), real because k' is odd
    g = torch.Generator(device=K.device).manual_seed(3)
    kp = torch.as_tensor(hr.kprime(N), dtype=torch.float32, device=K.device)
    kx, ky, kz = kp[:, None, None], kp[None, :, None], kp[None, None, : N // 2 + 1]
    fields = []
    if kind == "gradient":
        ph = torch.fft.rfftn(torch.randn((N, N, N), generator=g, device=K.device))
        for kc in (kx, ky, kz):
            fields.append(torch.fft.irfftn(1j * kc * ph, s=(N, N, N)).contiguous())
        del ph
    else:
        A = [torch.fft.rfftn(torch.randn((N, N, N), generator=g, device=K.device)) for _ in range(3)]
        for a, b, ka, kb in ((2, 1, ky, kz), (0, 2, kz, kx), (1, 0, kx, ky)):
            fields.append(torch.fft.irfftn(1j * (ka * A[a] - kb * A[b]), s=(N, N, N)).contiguous())
        del A
    torch.cuda.empty_cache()
    pipe = device_pipe = _pipeline(K, N)
    tot, comp, sol = pipe.spectrum_helmholtz(fields)
    del device_pipe
    leak = sol if kind == "gradient" else comp
    keep = comp if kind == "gradient" else sol
    full = tot[:, 3] > 0
    assert (np.abs(leak[full, 2]) <= 1e-5 * tot[full, 2]).all(), np.max(np.abs(leak[full, 2]) / tot[full, 2])
    assert np.allclose(keep[full, 2], tot[full, 2], rtol=1e-5)
    del fields
    _free(K)


# --------------------------------------------------- d. slab decomposition emulated on one GPU, production calls ----
def _nan_buffer(K, n):
    return torch.full((n,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=K.device)


@pytest.mark.parametrize("N,G,C", SLABS)
def test_emulated_slab_exchange_every_receiver(K, N, G, C):
    """vps_fft_z per sender slab and component -> vps_fft_y chunk by chunk into NaN-filled send buffers (packed rows) -> the
    all-to-all played by slicing -> vps_fft_x_bin_chunk_helmholtz on every receiver, against the whole-grid reference."""
    nx = N // G
    comps = _factors(N, 2)
    pipe = _pipeline(K, N)
    pipe.prepare()
    ref = hr.separable_helmholtz_sums(K.device, comps, N, pipe.Lbox, pipe.k2, pipe.thr)
    zimgs = [[None] * G for _ in range(3)]
    for i, f in enumerate(comps):
        for g in range(G):
            slab = chk.separable_slab(K.device, f, g * nx, nx)
            zimgs[i][g] = K.fft_z(slab, N, nx)
            del slab
    _free(K)
    psum, ns, pcomp = pipe.new_accumulators(helmholtz=True)
    for c in range(C):
        with K.binning_only():
            packed = K.y_packed(N)
            blk = K.chunk_block(N, nx, G, C, c, packed)
            sends = [[K.fft_y_chunk(z, N, nx, G, C, c, out=_nan_buffer(K, G * blk)) for z in zc] for zc in zimgs]
        assert packed
        for h in range(G):
            recv = [torch.cat([s[g][h * blk:(h + 1) * blk] for g in range(G)]) for s in sends]
            K.fft_x_bin_chunk_helmholtz(recv, N, nx, G, C, c, h, packed, psum, ns, pcomp)
            del recv
        del sends
    _check(pipe.finish_helmholtz(psum, ns, pcomp), ref, (N, G, C))
    del zimgs
    _free(K)


def test_refusals_before_anything_is_enqueued(K):
    """32 ranks at 2048 (the chunk form's limit, as vps_fft_x_bin_chunk), ncomp != 3, and LibraryComm: refused up front."""
    from vpower import device, _ffi
    N, G = 2048, 32
    pipe = _pipeline(K, N)
    pipe.prepare()
    psum, ns, pcomp = pipe.new_accumulators(helmholtz=True)
    recv = K.zeros((16,), torch.complex64)        # never read
    K.timing(True)
    try:
        with pytest.raises(_ffi.VpsError, match="at most 16 ranks"):
            K.fft_x_bin_chunk_helmholtz([recv] * 3, N, N // G, G, 1, 0, 0, False, psum, ns, pcomp)
        with pytest.raises(_ffi.VpsError, match="ncomp must be 3"):
            K.fft_x_bin_helmholtz([recv] * 2, N, 1, 0, 0, 1, N, psum, ns, pcomp)
        with pytest.raises(_ffi.VpsError, match="ncomp must be 3"):
            K.fft_x_bin_chunk_helmholtz([recv] * 2, N, N // 8, 8, 1, 0, 0, False, psum, ns, pcomp)
        K.sync()
        assert len(K.timing_list("fft_x")) == 0
    finally:
        K.timing(False)
    assert not psum.any() and not ns.any() and not pcomp.any()

    class _FakeLibraryComm(device.LibraryComm):      # (no RCCL communicator is made: the refusal comes first)
        def __init__(self):
            self.rank, self.world, self.enabled, self.force, self.backend, self.k = 0, 1, True, True, "library", K
    pipe = _pipeline(K, 64, comm=_FakeLibraryComm())
    fields = [K.zeros((64, 64, 64), torch.float32) for _ in range(3)]
    K.timing(True)
    try:
        with pytest.raises(Exception, match="LibraryComm"):
            pipe.accumulate_helmholtz(fields)
        with pytest.raises(Exception, match="LibraryComm"):
            pipe.accumulate_zimages_helmholtz(fields)
        K.sync()
        assert all(n == 0 for n, _ in K.timing_get().values())
    finally:
        K.timing(False)


# ---------------------------------------------------------------------------------- e. BoxField.helmholtz_spctrm ----
def _synth(N, Np, seed):
    from helpers import synth
    return synth(seed, Np)


def _agree(spec, tabs, rtol):
    tot = tabs[0]
    assert np.array_equal(np.asarray(spec.Nsample), np.asarray(tot.Nsample))
    for t in tabs:
        assert np.array_equal(np.asarray(t.Nsample), np.asarray(tot.Nsample))
        assert np.array_equal(np.asarray(t.k), np.asarray(tot.k))
    ok = np.asarray(tot.Nsample) > 0
    a, b = np.asarray(spec.Psum)[ok], np.asarray(tot.Psum)[ok]
    assert np.all(np.abs(a - b) <= rtol * np.abs(a)), np.max(np.abs(a - b) / np.abs(a))
    ps = [np.asarray(t.Psum) for t in tabs]
    assert np.allclose(ps[1] + ps[2], ps[0], rtol=1e-12, atol=0)
    assert (ps[1][ok] > 0).all() and (ps[2][ok] > 0).all()


@pytest.mark.parametrize("N", [64, 128])
def test_boxfield_particle_backed(K, N):
    from vpower import interp
    pos, vel, mass, dens = _synth(N, 200000, 21)
    gp = interp.GasParticles(pos, mass, dens, vel, 1.0)
    bf = gp.deposit_to_field(N)
    for q in ("velocity", "momentum"):
        tabs = bf.helmholtz_spctrm(q)
        _agree(bf.spctrm(q), tabs, 2e-6)
    # momentum's decomposition leaves the energy field behind: spctrm('energy') right after it runs no deposit of its own
    bf = gp.deposit_to_field(N)
    bf.helmholtz_spctrm("momentum")
    K.timing(True)
    try:
        e = bf.spctrm("energy")
        z_launches = len(K.timing_list("fft_z"))
    finally:
        K.timing(False)
    bf2 = gp.deposit_to_field(N)
    e2 = bf2.spctrm("energy")
    assert z_launches == 0
    assert np.array_equal(np.asarray(e.Nsample), np.asarray(e2.Nsample))
    assert np.allclose(np.asarray(e.Psum), np.asarray(e2.Psum), rtol=2e-6)
    with pytest.raises(Exception, match="Unrecognized physical quantity name"):
        bf.helmholtz_spctrm("energy")


def test_boxfield_momentum_bug_compat(K):
    from vpower import interp
    N = 64
    pos, vel, mass, dens = _synth(N, 100000, 22)
    gp = interp.GasParticles(pos, mass, dens, vel, 1.0)
    try:
        interp.REFERENCE_COMPAT["momentum_bug"] = True
        bf = gp.deposit_to_field(N)
        _agree(bf.spctrm("momentum"), bf.helmholtz_spctrm("momentum"), 2e-6)
        g = interp.BoxField(bf.get_v(), bf.mass, bf.Lcell)
        _agree(g.spctrm("momentum"), g.helmholtz_spctrm("momentum"), TOTAL_RTOL)
    finally:
        interp.REFERENCE_COMPAT["momentum_bug"] = False


@pytest.mark.parametrize("N", [64, 256])
def test_boxfield_grid_backed_against_fftn_reference(K, N):
    from vpower import interp
    rng = np.random.default_rng(N)
    v = rng.standard_normal((N, N, N, 3)).astype(np.float32).astype(np.float64)
    m = np.exp(0.3 * rng.standard_normal((N, N, N))).astype(np.float32).astype(np.float64)
    bf = interp.BoxField(v, m, 1.0 / N)
    for q in ("velocity", "momentum"):
        tabs = bf.helmholtz_spctrm(q)
        _agree(bf.spctrm(q), tabs, TOTAL_RTOL)
        if N == 64:
            f = [v[..., c] for c in range(3)] if q == "velocity" else [v[..., c] * m for c in range(3)]
            ref = hr.helmholtz_tables(*f, 1.0, N, "library")
            for t, r in zip(tabs, ref):
                assert np.array_equal(np.asarray(t.Nsample), r[:, 3])
                assert np.allclose(np.asarray(t.Psum), r[:, 2], rtol=2e-5, atol=2e-5 * ref[0][:, 2])


def test_boxfield_neighbour_backed(K):
    from vpower import interp
    N = 64
    pos, vel, mass, dens = _synth(N, 50000, 23)
    gp = interp.GasParticles(pos, mass, dens, vel, 1.0)
    bf = gp.ann_interp_to_field(N)
    tabs = bf.helmholtz_spctrm("velocity")          # first spectrum: the search writes the fields directly
    _agree(bf.spctrm("velocity"), tabs, 2e-6)
    _agree(bf.spctrm("momentum"), bf.helmholtz_spctrm("momentum"), 2e-6)


# --------------------------------------------------------------------------------------------------------- f. CLI ----
def test_cli_helmholtz_writes_three_tables(K, tmp_path):
    from helpers import synth
    pos, vel, mass, dens = synth(31, 100000)
    snap = tmp_path / "snap.npz"
    np.savez(snap, Coordinates=pos, Masses=mass, Density=dens, Velocities=vel)
    script = os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts", "parallel_optimized.py")
    outs = {}
    for flag in ((), ("--helmholtz",)):
        d = tmp_path / ("h" if flag else "p")
        d.mkdir()
        r = subprocess.run([sys.executable, script, "-i", str(snap), "-N", "64", "-o", str(d), "-f", *flag],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[bool(flag)] = d
    h, p = outs[True], outs[False]
    for name in ("Pk.txt", "Pk_compressive.txt", "Pk_solenoidal.txt"):
        assert (h / name).exists(), name
    assert not (p / "Pk_compressive.txt").exists()
    a, b = np.loadtxt(h / "Pk.txt"), np.loadtxt(p / "Pk.txt")
    assert a.shape == b.shape and np.allclose(a, b, rtol=1e-6, equal_nan=True)
    c, s = np.loadtxt(h / "Pk_compressive.txt"), np.loadtxt(h / "Pk_solenoidal.txt")
    assert c.shape == a.shape == s.shape
    ok = a[:, 3] > 0
    assert np.allclose(c[ok, 2] + s[ok, 2], a[ok, 2], rtol=1e-6)
