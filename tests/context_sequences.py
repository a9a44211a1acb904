"""Steps, orders and the transition list of tests/test_gpu_context_state.py and tests/test_context_state_cpu.py: ONE context
that lives through a sequence of different configurations.  TEST INFRASTRUCTURE ONLY, never imported by the package.

A STEP is a configuration, a call and its float64 reference (computed up front, never changed).  `call(K)` runs the step on the
kernel set K -- vpower.device.HipKernels, or the stateless numpy stand-ins tests/oracle_kernels.py / helmholtz_kernels.py --
and yields (label, result, facts) per library call it makes; `check` compares a result with the step's own reference.  `facts`
are host-side observations of the context at that call (binning mode, window, packing, N, nbins, ...): the coverage guard
asserts that the ordered pairs (facts of the previous call, facts of this call) cover REQUIRED below.

`covering_orders` turns the steps of a leg into orders, each run on a FRESH context: every step is the first call of some
order, and every step follows every other step that shares a cache key with it (`Step.keys`) in some order.

References: oracle.gpu_checks (separable fields: exact at any N), helmholtz_ref, correlation_ref, weighted_ref, density_ref.
"""
import contextlib

import numpy as np
import torch

import correlation_ref as cref
import density_ref as dref
import helmholtz_ref as hr
import weighted_ref as wref
from oracle import gpu_checks as chk

PSUM_RTOL = 2e-5     # DESIGN.md section 5 (tests/test_gpu_spectrum_matrix.py: PSUM_RTOL): Psum per bin vs the float64 reference
MODE_RTOL = 1e-5     # tests/test_gpu_spectrum_matrix.py: per mode, max |got - exact| / rms of the plane
FIELD_RTOL = 1e-5    # tests/test_gpu_weighted.py, test_gpu_density.py: fields against the reference fields, of their max
IMAGE_RTOL = 1e-5    # the same files: z/y images, of their rms
XI_EXACT_BAR = 2e-5  # tests/test_gpu_correlation.py: |xi - xi_ref| <= 2e-5 xi(0) per shell (the shell-sum bar against xi(0))
RANK = 3             # rank of the separable fields (tests/test_gpu_spectrum_matrix.py)


class HostOnly:
    """Stands where PowerPipeline wants a kernel set when only its host-side tables are asked for."""

    def fft_supported(self, N):
        return True


def is_hip(K):
    return hasattr(K, "lib")


@contextlib.contextmanager
def options(K, opts):
    """Process-wide library options for the duration of the block (nothing to set on the numpy stand-ins)."""
    if not opts or not is_hip(K):
        yield
        return
    from vpower import _ffi
    try:
        for k_, v_ in opts.items():
            _ffi.set_option(k_, v_)
        yield
    finally:
        for k_ in opts:
            _ffi.set_option(k_, None)


def default_box(N):
    """tests/test_gpu_spectrum_matrix.py: _box -- 1, or 2.5 where the library flavour's np.arange edges are inconsistent at 1."""
    from vpower import device
    for L in (1.0, 2.5):
        kmin = 2 * np.pi / L
        try:
            device.bin_edges(kmin, np.pi / (L / N), kmin, "library")
            return L
        except Exception:
            pass
    raise AssertionError(N)


def host_pipeline(N, flavour="library", krange=None, deconvolve=None, K=None):
    """PowerPipeline of the default k range (box of default_box) or of a row of gpu_checks.K_RANGES (its flavour and box)."""
    from vpower import device
    k = K if K is not None else HostOnly()
    comm = device.SlabComm(enabled=False)
    if krange is None:
        return device.PowerPipeline(N, default_box(N), kernels=k, comm=comm, flavour=flavour, deconvolve=deconvolve)
    L = chk.k_range_box(krange, N)
    flavour, kmin, kmax, kres = chk.k_range(krange, N, L)
    return device.PowerPipeline(N, L, kernels=k, comm=comm, flavour=flavour, kmin=kmin, kmax=kmax, kres=kres, deconvolve=deconvolve)


_FIELDS = {}


def factors(N, ncomp=3):
    return [chk.separable_factors(N, RANK, seed=7000 * N + i) for i in range(ncomp)]


def fields(dev, N):
    """(factors, float32 tensors on dev) of the three separable components at N, made once per device and size."""
    key = (str(dev), N)
    if key not in _FIELDS:
        comps = factors(N)
        _FIELDS[key] = (comps, [chk.separable_slab(dev, f, 0, N) for f in comps])
    return _FIELDS[key]


def release():
    _FIELDS.clear()


def fft_keys(N):
    """fft_tables is keyed by complex length: the z pass of N takes NC = N / 2, the y and x passes NC = N."""
    return {("fft", N // 2), ("fft", N)}


def expected_mode(pipe_or_tables, opts, N=None, edges=None):
    if opts.get("no_fast_binning"):
        return 0
    if N is None:
        p = pipe_or_tables
        mode = chk.expected_binning_mode(p.N, p.k2, p.thr, p.edges)
    else:
        k2, thr = pipe_or_tables
        mode = chk.expected_binning_mode(N, k2, thr, edges)
    return min(mode, 1) if opts.get("no_int_binning") else mode


def observed_mode(K, expected):
    return K.binning_mode() if hasattr(K, "binning_mode") else expected


def psum_ok(got_ps, got_ns, ref_ps, ref_ns, what):
    assert np.array_equal(np.asarray(got_ns, dtype=np.float64), np.asarray(ref_ns, dtype=np.float64)), (what, "shell counts")
    err = np.abs(got_ps - ref_ps)
    bad = err > PSUM_RTOL * np.abs(ref_ps)
    assert not bad.any(), (what, "Psum", np.nonzero(bad)[0][:8], float(np.max(err / np.maximum(np.abs(ref_ps), 1e-300))))


class Step:
    kind = "?"
    cpu = True          # the numpy stand-ins implement the call

    def __init__(self, tag, N):
        self.tag, self.N = tag, N
        self.keys = set(fft_keys(N))
        self.ref = None

    def facts(self, **kw):
        f = dict(kind=self.kind, tag=self.tag, N=self.N)
        f.update(kw)
        return f

    def __repr__(self):
        return "%s(%s, N=%d)" % (type(self).__name__, self.tag, self.N)


# ----------------------------------------------------------------------------------------------- whole-grid spectra ----
class PipeStep(Step):
    """PowerPipeline.spectrum of the three separable components under `opts`; window: None | 'cic' | 'tsc' | 'ones' (a table
    of ones, valid at every N, through the same vps_set_window)."""
    kind = "spectrum"

    def __init__(self, tag, N, flavour="library", krange=None, window=None, opts=None):
        super().__init__(tag, N)
        self.flavour, self.krange, self.window, self.opts = flavour, krange, window, dict(opts or {})
        self.keys |= {"bin", "xpart", "win"}
        self.cpu = window is None

    def pipeline(self, K=None):
        p = host_pipeline(self.N, self.flavour, self.krange, None if self.window in (None, "ones") else self.window, K)
        if self.window == "ones":
            p.window = np.ones(self.N, dtype=np.float32)
        return p

    def host(self):
        p = self.pipeline()
        self.nbins, self.mode = p.nbins, expected_mode(p, self.opts)
        return p

    def make_ref(self, dev):
        p = self.host()
        comps = factors(self.N)
        counts = chk.shell_counts_exact(dev, self.N, p.k2, p.thr)
        ps, ns = chk.separable_shell_sums(dev, comps, self.N, p.Lbox, p.k2, p.thr, win=p.window)
        assert np.array_equal(ns, counts) and counts.sum() > 0, self
        self.ref = (ps, counts)

    def expected_facts(self):
        self.host()
        return [self.facts(nbins=self.nbins, mode=self.mode, window=self.window, opts=tuple(sorted(self.opts)))]

    def call(self, K):
        pipe = self.pipeline(K)
        with options(K, self.opts):
            tab = pipe.spectrum(fields(getattr(K, "device", "cpu"), self.N)[1])
            mode = observed_mode(K, self.mode)
        yield "", (tab[:, 2].copy(), tab[:, 3].copy()), self.facts(nbins=pipe.nbins, mode=mode, window=self.window,
                                                                   opts=tuple(sorted(self.opts)))

    def check(self, label, got, what):
        psum_ok(got[0], got[1], self.ref[0], self.ref[1], what)


class RawStep(Step):
    """vps_set_binning called directly with tables of the test's own making, then the z/y passes and the binning x pass into
    accumulators that sit in FRONT of a zeroed tail: a call that bins with more shells than it was given shows there.
    how = 'asym': the default tables with ONE k2 entry moved (k2[N-1] != k2[1]: not mirrored, the general shell walk);
          'prefix': the default axis and the first nbins / 4 + 1 thresholds of the default tables -- the same N, k2, edge0 and
                    spacing, a bit-equal prefix of the thresholds and FEWER bins: what a shortcut that forgot nbins would skip;
          'toggle': the default tables once, then three calls with no upload in between under no_int_binning 0, 1, 0."""
    kind = "raw"
    TAIL = 512

    def __init__(self, tag, N, how):
        super().__init__(tag, N)
        self.how = how
        self.keys |= {"bin", "xpart", "win"}

    def host(self):
        p = host_pipeline(self.N)
        n, k2, thr, e0, inv = p._binning
        k2 = np.array(k2, dtype=np.float64)
        thr = np.array(thr, dtype=np.float64)
        if self.how == "asym":
            k2[self.N - 1] = k2[1] * 1.03
        if self.how == "prefix":
            thr = thr[: max(2, p.nbins // 4) + 1].copy()
        self.tables = (n, k2, thr, e0, inv)
        self.const, self.Lbox = p.const, p.Lbox
        self.nbins = len(thr) - 1
        assert self.nbins + self.TAIL >= p.nbins
        edges = p.edges[: self.nbins + 1]
        base = expected_mode((k2, thr), {}, self.N, edges)
        self.modes = [base, min(base, 1), base] if self.how == "toggle" else [base]
        assert base == (0 if self.how == "asym" else 2), (self, base)

    def make_ref(self, dev):
        self.host()
        n, k2, thr, e0, inv = self.tables
        self.ref = chk.separable_shell_sums(dev, factors(self.N), self.N, self.Lbox, k2, thr)
        assert self.ref[1].sum() > 0
        if self.how != "asym":
            assert np.array_equal(self.ref[1], chk.shell_counts_exact(dev, self.N, k2, thr))

    def expected_facts(self):
        self.host()
        labels = ["int on", "int off", "int on again"] if self.how == "toggle" else [""]
        return [self.facts(nbins=self.nbins, mode=m, window=None, sub=l) for m, l in zip(self.modes, labels)]

    def _bin(self, K):
        N, h = self.N, self.N // 2
        buf = K.zeros((2 * (self.nbins + self.TAIL),), torch.float64)
        psum, tail_p = buf[: self.nbins], buf[self.nbins: self.nbins + self.TAIL]
        ns_all = buf[self.nbins + self.TAIL:].view(torch.int64)
        ns, tail_n = ns_all[: self.nbins], ns_all[self.nbins:]
        done = [K.fft_zy(f, N, N) for f in fields(getattr(K, "device", "cpu"), N)[1]]
        K.fft_x_bin_multi([d[0] for d in done], N, h * N, 0, 0, 1, h * N * N, psum, ns)
        K.fft_x_bin_multi([d[1] for d in done], N, N, 0, h, 1, N * N, psum, ns)
        out = buf.cpu()
        beyond = bool(tail_p.cpu().any()) or bool(tail_n.cpu().any())
        return out[: self.nbins].numpy() * (0.5 * self.const ** 2), ns.cpu().numpy().astype(np.float64), beyond

    def call(self, K):
        K.set_binning(*self.tables)
        if hasattr(K, "set_window"):
            K.set_window(self.N, None)
        ef = self.expected_facts()
        if self.how != "toggle":
            yield "", self._bin(K), dict(ef[0], mode=observed_mode(K, self.modes[0]))
            return
        for i, off in enumerate((0, 1, 0)):
            with options(K, {"no_int_binning": 1} if off else {}):
                got = self._bin(K)
                yield ef[i]["sub"], got, dict(ef[i], mode=observed_mode(K, self.modes[i]))

    def check(self, label, got, what):
        assert not got[2], (what, "shells beyond the %d bins of the tables were written" % self.nbins)
        psum_ok(got[0], got[1], self.ref[0], self.ref[1], what)


class WriteStep(Step):
    """fft_zy + the x pass in write mode on every line of one component, every mode against gpu_checks.separable_plane."""
    kind = "write"
    cpu = False

    def __init__(self, tag, N):
        super().__init__(tag, N)

    def make_ref(self, dev):
        self.ref = factors(self.N)[0]

    def expected_facts(self):
        return [self.facts()]

    def call(self, K):
        N, h = self.N, self.N // 2
        spec, nyq = K.fft_zy(fields(K.device, N)[1][0], N, N)
        out = K.empty(((h + 1) * N, N), torch.complex64)
        K.fft_x_write(spec, N, h * N, 1, 0, out[: h * N])
        K.fft_x_write(nyq, N, N, 1, 0, out[h * N:])
        yield "", out.view(h + 1, N, N), self.facts()

    def check(self, label, got, what):
        N, h = self.N, self.N // 2
        step = max(1, (1 << 23) // (N * N))
        for k0 in range(0, h + 1, step):
            planes = list(range(k0, min(h + 1, k0 + step)))
            ex = chk.separable_plane(got.device, self.ref, planes)
            g = got[planes[0]: planes[-1] + 1].to(torch.complex128)
            rel = (g - ex).abs().amax(dim=(1, 2)) / ex.abs().square().mean(dim=(1, 2)).sqrt()
            i = int(torch.argmax(torch.nan_to_num(rel, nan=float("inf"))))
            assert float(rel[i]) < MODE_RTOL, (what, "kz", planes[i], float(rel[i]))


class WindowMismatchStep(Step):
    """A window for N2 is set (the CIC pipeline of N2 prepared), then the binning tables of N alone: the binning x pass at N is
    refused with VPS_ERR_ARG ("vps_set_window was called for N=N2") and enqueues nothing."""
    kind = "window-mismatch"
    cpu = False

    def __init__(self, tag, N, N2):
        super().__init__(tag, N)
        self.N2 = N2
        self.keys |= fft_keys(N2) | {"bin", "win"}

    def make_ref(self, dev):
        self.ref = ()

    def expected_facts(self):
        return [self.facts(window="cic", win_N=self.N2)]

    def call(self, K):
        from vpower import _ffi
        host_pipeline(self.N2, deconvolve="cic", K=K).prepare()
        pipe = host_pipeline(self.N, K=K)
        K.set_binning(*pipe._binning)
        N, h = self.N, self.N // 2
        spec, _ = K.fft_zy(fields(K.device, N)[1][0], N, N)
        psum, ns = pipe.new_accumulators()
        K.timing(True)
        try:
            try:
                K.fft_x_bin_multi([spec], N, h * N, 0, 0, 1, h * N * N, psum, ns)
                refused = None
            except _ffi.VpsError as e:
                refused = str(e)
            K.sync()
            launches = len(K.timing_list("fft_x"))
        finally:
            K.timing(False)
        yield "", (refused, launches, bool(psum.any()) or bool(ns.any())), self.expected_facts()[0]

    def check(self, label, got, what):
        refused, launches, touched = got
        assert refused is not None and "(-1)" in refused and "vps_set_window was called for N=%d, not %d" % (self.N2, self.N) in refused, (what, refused)
        assert launches == 0 and not touched, (what, launches, touched)


# ----------------------------------------------------------------------------------------------- emulated slab exchange ----
class ExchangeStep(Step):
    """The slab decomposition emulated through the production calls: fft_z per sender slab, the chunked y pass into NaN-filled
    send buffers (inside binning_only() if `scope`: packed rows), the all-to-all played by slicing, fft_x_bin_chunk per
    receiver into that receiver's own accumulators; every receiver against separable_shell_sums(kz=, nyq_ky=)."""
    kind = "exchange"

    def __init__(self, tag, N, G, C, krange=None, scope=True):
        super().__init__(tag, N)
        self.G, self.C, self.krange, self.scope = G, C, krange, scope
        self.keys |= {"bin", "xpart", "win", "ypack"}

    def pipeline(self, K=None):
        return host_pipeline(self.N, "library", self.krange, None, K)

    def planes(self, r):
        nkc = self.N // 2 // self.G // self.C
        return [c * self.G * nkc + j * self.G + r for c in range(self.C) for j in range(nkc)] + [self.N // 2]

    def host(self):
        p = self.pipeline()
        self.nbins = p.nbins
        self.mode = expected_mode(p, {})
        # the stand-ins pack from N = 16 on; the library keeps a row cut from N = 128 on, under the mirrored-kx modes
        self.packed_hip = bool(self.scope and self.N >= 128 and self.mode > 0)
        return p

    def make_ref(self, dev):
        p = self.host()
        f = factors(self.N)[:1]
        nky = self.N // self.G
        self.ref = [chk.separable_shell_sums(dev, f, self.N, p.Lbox, p.k2, p.thr, kz=self.planes(r), nyq_ky=(r * nky, (r + 1) * nky))
                    for r in range(self.G)]
        whole = chk.shell_counts_exact(dev, self.N, p.k2, p.thr)
        assert np.array_equal(sum(r[1] for r in self.ref), whole) and whole.sum() > 0, self

    def expected_facts(self):
        self.host()
        return [self.facts(nbins=self.nbins, mode=self.mode, window=None, scope=self.scope,
                           exch=(self.G, self.C, bool(self.scope)))]

    def call(self, K):
        N, G, C = self.N, self.G, self.C
        nx = N // G
        dev = getattr(K, "device", "cpu")
        pipe = self.pipeline(K)
        pipe.prepare()
        field = fields(dev, N)[1][0]
        zimgs = [K.fft_z(field[g * nx:(g + 1) * nx].contiguous(), N, nx) for g in range(G)]
        accs = [pipe.new_accumulators() for _ in range(G)]
        packed_seen = set()
        for c in range(C):
            with (K.binning_only() if self.scope else contextlib.nullcontext()):
                packed = K.y_packed(N)
                blk = K.chunk_block(N, nx, G, C, c, packed)
                sends = []
                for z in zimgs:
                    out = torch.full((G * blk,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=dev) if is_hip(K) else None
                    sends.append(K.fft_y_chunk(z, N, nx, G, C, c, out=out))
            packed_seen.add(bool(packed))
            for h in range(G):
                recv = torch.cat([s[h * blk:(h + 1) * blk] for s in sends])
                K.fft_x_bin_chunk([recv], N, nx, G, C, c, h, packed, accs[h][0], accs[h][1])
        assert len(packed_seen) == 1
        packed = packed_seen.pop()
        if is_hip(K):
            assert packed == self.packed_hip, (self, packed)
        got = [(a[0].cpu().numpy() * (0.5 * pipe.const ** 2), a[1].cpu().numpy().astype(np.float64)) for a in accs]
        yield "", got, self.facts(nbins=pipe.nbins, mode=observed_mode(K, self.mode), window=None, scope=self.scope,
                                  exch=(G, C, bool(self.scope)))

    def check(self, label, got, what):
        for r, (g, ref) in enumerate(zip(got, self.ref)):
            psum_ok(g[0], g[1], ref[0], ref[1], (what, "receiver", r))


class ScopeExceptionStep(Step):
    """binning_only() left by an exception raised inside the `with`; the un-scoped z/y passes that follow must write every row:
    NaN-prefilled outputs, then the write-mode x pass, every mode of every plane against gpu_checks.separable_plane."""
    kind = "scope-exception"
    cpu = False

    def __init__(self, tag, N, krange="deep"):
        super().__init__(tag, N)
        self.krange = krange
        self.keys |= {"bin", "win", "ypack"}
        self._write = WriteStep(tag, N)

    def make_ref(self, dev):
        self._write.make_ref(dev)
        self.ref = self._write.ref

    def expected_facts(self):
        return [self.facts(scope=False, left_by="exception")]

    def call(self, K):
        N, h = self.N, self.N // 2
        host_pipeline(N, "library", self.krange, None, K).prepare()      # a deep cut: most rows would be skipped inside the scope

        class Boom(Exception):
            pass
        try:
            with K.binning_only():
                assert K.y_packed(N)
                raise Boom()
        except Boom:
            pass
        assert not K.y_packed(N)
        nan = complex(float("nan"), float("nan"))
        spec = torch.full((h, N, N), nan, dtype=torch.complex64, device=K.device)
        nyq = torch.full((N, N), nan, dtype=torch.complex64, device=K.device)
        K.fft_zy(fields(K.device, N)[1][0], N, N, spec=spec, nyq=nyq)
        out = K.empty(((h + 1) * N, N), torch.complex64)
        K.fft_x_write(spec, N, h * N, 1, 0, out[: h * N])
        K.fft_x_write(nyq, N, N, 1, 0, out[h * N:])
        yield "", out.view(h + 1, N, N), self.expected_facts()[0]

    def check(self, label, got, what):
        self._write.check(label, got, what)


# ------------------------------------------------------------------------------- Helmholtz and the real-space lattice ----
class HelmholtzStep(Step):
    kind = "helmholtz"

    def __init__(self, tag, N):
        super().__init__(tag, N)
        self.keys |= {"bin", "xpart", "win"}

    def host(self):
        p = host_pipeline(self.N)
        self.nbins, self.mode = p.nbins, expected_mode(p, {})
        return p

    def make_ref(self, dev):
        p = self.host()
        self.ref = hr.separable_helmholtz_sums(dev, factors(self.N), self.N, p.Lbox, p.k2, p.thr)
        assert np.array_equal(self.ref[2], chk.shell_counts_exact(dev, self.N, p.k2, p.thr))

    def expected_facts(self):
        self.host()
        return [self.facts(nbins=self.nbins, mode=self.mode, window=None)]

    def call(self, K):
        pipe = host_pipeline(self.N, K=K)
        tabs = pipe.finish_helmholtz(*pipe.accumulate_helmholtz(fields(getattr(K, "device", "cpu"), self.N)[1]))
        yield "", tabs, self.facts(nbins=pipe.nbins, mode=observed_mode(K, self.mode), window=None)

    def check(self, label, tabs, what):
        ps_t, ps_c, ns = self.ref                       # tests/test_gpu_helmholtz.py: _check
        tot, comp, sol = tabs
        for t in tabs:
            assert np.array_equal(t[:, 3], ns), (what, "shell counts")
        for t, r, name in ((tot, ps_t, "total"), (comp, ps_c, "compressive")):
            bad = np.abs(t[:, 2] - r) > PSUM_RTOL * np.abs(r)
            assert not bad.any(), (what, name, np.nonzero(bad)[0][:8])
        bad = np.abs(sol[:, 2] - (ps_t - ps_c)) > PSUM_RTOL * ps_t
        assert not bad.any(), (what, "solenoidal", np.nonzero(bad)[0][:8])


class CorrelationStep(Step):
    """CorrelationPipeline.correlation (vps_fft_x modes 5 and 6) against correlation_ref.correlation of the same float32 fields.
    refused=True: first the CIC window of N is set and the lag tables uploaded WITHOUT clearing it -- bin_real must be refused
    ("a k-space window is set") with no x-pass launch and untouched accumulators; the pipeline, which clears the window, then
    works."""
    kind = "correlation"
    cpu = False

    def __init__(self, tag, N, refused=False):
        super().__init__(tag, N)
        self.refused = refused
        self.keys |= {"bin", "xpart", "win"}

    def make_ref(self, dev):
        fl = [chk.separable_slab(torch.device("cpu"), f, 0, self.N).numpy() for f in factors(self.N)]
        self.ref = cref.correlation(fl, default_box(self.N))

    def expected_facts(self):
        out = [self.facts(window=None, lattice="r")]
        return ([self.facts(window="cic", lattice="r", sub="refused")] if self.refused else []) + out

    def call(self, K):
        from vpower import device, _ffi
        N = self.N
        fl = fields(K.device, N)[1]
        cp = device.CorrelationPipeline(N, default_box(N), kernels=K)
        if self.refused:
            host_pipeline(N, deconvolve="cic", K=K).prepare()
            K.set_binning(*cp._binning)
            psum, ns = K.zeros((cp.nbins,), torch.float64), K.zeros((cp.nbins,), torch.int64)
            K.timing(True)
            try:
                try:
                    K.bin_real(fl[0], N, psum, ns)
                    msg = None
                except _ffi.VpsError as e:
                    msg = str(e)
                K.sync()
                launches = len(K.timing_list("fft_x"))
            finally:
                K.timing(False)
            yield "refused", (msg, launches, bool(psum.any()) or bool(ns.any())), self.expected_facts()[0]
        tab, xi0 = cp.correlation(fl)
        yield "", (tab, xi0), self.expected_facts()[-1]

    def check(self, label, got, what):
        if label == "refused":
            msg, launches, touched = got
            assert msg is not None and "(-1)" in msg and "k-space window is set" in msg, (what, msg)
            assert launches == 0 and not touched, (what, launches, touched)
            return
        tab, xi0 = got
        xr, cnt, xi0_ref = self.ref
        assert np.array_equal(tab[:, 2], cnt.astype(np.float64)), (what, "lattice counts")
        err = max(float(np.max(np.abs(tab[:, 1] - xr))), abs(xi0 - xi0_ref)) / xi0_ref
        assert err <= XI_EXACT_BAR, (what, "xi", err)


# ------------------------------------------------------------------------------------------------- density exponent ----
_PARTICLES = {}


def particles(N, Np):
    key = (N, Np)
    if key not in _PARTICLES:
        from vpower import synth
        pos, vel, _, dens = synth.particles(41, Np, 1.0)
        _PARTICLES[key] = (pos, vel, dens, wref.ngp_vec_grid(pos, vel, dens, N, 1.0))
    return _PARTICLES[key]


class DepositStep(Step):
    """deposit_field of VPS_WEIGHTED_VELOCITY and VPS_DENSITY with exponent alpha (per cell against weighted_ref / density_ref,
    FIELD_RTOL of the field's max) and, where deposit_fft_zy_supported says so, the pencil route (z/y images against numpy's
    transform of the reference fields, IMAGE_RTOL of their rms).
    nan_after=True: afterwards vps_set_density_weight(NaN) must be refused, and a VPS_WEIGHTED_VELOCITY call through the C ABI
    that sets no exponent of its own must still form rho^alpha v."""
    kind = "deposit"
    cpu = False

    def __init__(self, tag, N, Np, alpha, nan_after=False):
        super().__init__(tag, N)
        self.Np, self.alpha, self.nan_after = Np, float(alpha), nan_after
        self.keys = {"alpha"} | fft_keys(N)

    def make_ref(self, dev):
        grid = particles(self.N, self.Np)[3]
        self.ref = (wref.fields_from_vec_grid(grid, self.alpha), [dref.density_field(grid, self.alpha)])

    def expected_facts(self):
        out = [self.facts(alpha=round(self.alpha, 6), sub=s) for s in ("weighted", "density", "weighted pencil", "density pencil")]
        return out + ([self.facts(alpha=round(self.alpha, 6), sub="after NaN")] if self.nan_after else [])

    def _device_particles(self, K):
        key = ("dev", str(K.device), self.N, self.Np)
        if key not in _PARTICLES:
            pos, vel, dens, _ = particles(self.N, self.Np)
            _PARTICLES[key] = tuple(torch.as_tensor(a).to(K.device) for a in (pos, vel, dens))
        return _PARTICLES[key]

    def call(self, K):
        from vpower import device
        N = self.N
        d = self._device_particles(K)
        ef = self.expected_facts()
        qs = (device.WeightedVelocity(self.alpha), device.Density(self.alpha))
        for i, q in enumerate(qs):
            yield ef[i]["sub"], K.deposit_field(d[0], d[1], d[2], N, 1.0, 0, N, q).cpu().numpy(), ef[i]
        for i, q in enumerate(qs):
            if K.fused_supported(N, q):
                spec, nyq = K.deposit_fft_zy(d[0], d[1], d[2], N, 1.0, 0, N, q)
                yield ef[2 + i]["sub"], (spec.cpu().numpy(), nyq.cpu().numpy()), ef[2 + i]
        if self.nan_after:
            K.deposit_field(d[0], d[1], d[2], N, 1.0, 0, N, qs[0])        # the exponent in force: this step's
            rc = K.lib.vps_set_density_weight(K.ctx, float("nan"))
            assert rc == -1, rc                                          # VPS_ERR_ARG
            out = K.empty((3, N, N, N), torch.float32)
            work = K.workspace("deposit", K.lib.vps_deposit_workspace_bytes(d[0].shape[0], 4, N, N))
            K._stream()
            K._chk(K.lib.vps_deposit_field(K.ctx, K._ptr(d[0]), 0, K._ptr(d[1]), K._ptr(d[2]), d[0].shape[0], N, 1.0, 0, N,
                                           int(device.WEIGHTED), 0, K._ptr(out), K._ptr(work)))
            yield "after NaN", out.cpu().numpy(), ef[4]

    def check(self, label, got, what):
        ref = self.ref[1] if label.startswith("density") else self.ref[0]
        if label.endswith("pencil"):
            spec, nyq = got
            h = self.N // 2
            assert spec.shape[0] == len(ref)
            for c, f in enumerate(ref):
                ex = np.fft.fft(np.fft.rfft(f, axis=2), axis=1)            # [x, ky, kz <= N/2]
                scale = np.sqrt(np.mean(np.abs(ex) ** 2))
                err = np.max(np.abs(spec[c].transpose(2, 1, 0) - ex[:, :, :h])) / scale
                errn = np.max(np.abs(nyq[c].T - ex[:, :, h])) / scale
                assert err < IMAGE_RTOL and errn < IMAGE_RTOL, (what, c, err, errn)
            return
        assert got.shape[0] == len(ref), (what, got.shape)
        scale = max(np.max(np.abs(f)) for f in ref)
        err = max(float(np.max(np.abs(got[c].astype(np.float64) - ref[c]))) for c in range(len(ref))) / scale
        assert err < FIELD_RTOL, (what, err)


# ------------------------------------------------------------------------------------------------------------ orders ----
def shares(a, b):
    return bool(a.keys & b.keys)


def covering_orders(steps):
    """Orders (lists of indices into `steps`), each for a fresh context: the first walks every ordered pair (a, b) of steps
    that share a cache key, the others put every remaining step first."""
    n = len(steps)
    need = {(a, b) for a in range(n) for b in range(n) if a != b and shares(steps[a], steps[b])}
    order, left = [0], set(need)
    while left:
        cur = order[-1]
        nxt = sorted(b for (a, b) in left if a == cur)
        if nxt:
            order.append(nxt[0])
        else:
            a, b = min(left)
            if a != cur:
                order.append(a)
                left.discard((cur, a))
            order.append(b)
        left.discard((order[-2], order[-1]))
    orders = [order]
    for s in range(1, n):
        orders.append([s, (s + 1) % n] if n > 1 else [s])
    return orders


def pairs_of(order):
    return set(zip(order[:-1], order[1:]))


def check_orders(steps, orders):
    """What the issue asks of the orders of a leg."""
    n = len(steps)
    assert {o[0] for o in orders} >= set(range(n)), "every step is the first call on a fresh context"
    got = set().union(*[pairs_of(o) for o in orders])
    need = {(a, b) for a in range(n) for b in range(n) if a != b and shares(steps[a], steps[b])}
    assert need <= got, sorted(need - got)


# -------------------------------------------------------------------------------------------------------------- legs ----
class Leg:
    def __init__(self, name, steps, prescribed=()):
        self.name, self.steps = name, steps
        by_tag = {s.tag: i for i, s in enumerate(steps)}
        assert len(by_tag) == len(steps)
        self.orders = ([[by_tag[t] for t in prescribed]] if prescribed else []) + covering_orders(steps)

    def make_refs(self, dev):
        for s in self.steps:
            if s.ref is None:
                s.make_ref(dev)


def leg_a1(N):
    return Leg("a1", [PipeStep("library", N), PipeStep("script", N, flavour="script"), PipeStep("band", N, krange="band"),
                      PipeStep("deep", N, krange="deep"), PipeStep("many", N, krange="many"), PipeStep("wide", N, krange="wide"),
                      RawStep("prefix", N, "prefix")],
               ("library", "script", "library", "band", "deep", "library", "many", "wide", "library", "prefix", "library"))


def leg_a2(N):
    return Leg("a2", [PipeStep("library", N), RawStep("asym", N, "asym")], ("library", "asym", "library"))


def leg_a3(N):
    return Leg("a3", [PipeStep("library", N), PipeStep("nofast", N, opts={"no_fast_binning": 1})], ("library", "nofast", "library"))


def leg_a4(N):
    return Leg("a4", [PipeStep("library", N), RawStep("toggle", N, "toggle")], ("library", "toggle", "library"))


def leg_b(sizes, order):
    steps = [PipeStep("spectrum %d" % N, N) for N in sizes] + [WriteStep("write %d" % N, N) for N in sizes]
    return Leg("b", steps, ["spectrum %d" % N for N in order] + ["write %d" % N for N in order])


def leg_c(N, N2):
    steps = [PipeStep("cic", N, window="cic"), PipeStep("none", N), PipeStep("tsc", N, window="tsc"),
             PipeStep("cic %d" % N2, N2, window="cic"), WindowMismatchStep("mismatch", N, N2),
             PipeStep("ones", N, window="ones"), PipeStep("ones %d" % N2, N2, window="ones")]
    return Leg("c", steps, ("cic", "none", "tsc", "cic", "cic %d" % N2, "mismatch", "none", "ones", "ones %d" % N2, "ones", "none"))


def leg_d(N, geom, geom2):
    (G, C), (G2, C2) = geom, geom2
    steps = [ExchangeStep("packed", N, G, C), ExchangeStep("unpacked", N, G, C, scope=False),
             ExchangeStep("packed band", N, G, C, krange="band"), ExchangeStep("packed other geometry", N, G2, C2),
             ScopeExceptionStep("exception", N)]
    return Leg("d", steps, ("packed", "unpacked", "packed band", "packed other geometry", "packed", "exception", "packed"))


def leg_e(N, Nsmall):
    steps = [PipeStep("most bins", N, krange="many"), PipeStep("few bins small N", Nsmall, krange="wide"),
             PipeStep("one workgroup per CU", N, opts={"x_wg_per_cu": 1})]
    return Leg("e", steps, ("most bins", "few bins small N", "one workgroup per CU"))


def leg_f(N):
    steps = [PipeStep("spectrum", N), HelmholtzStep("helmholtz", N), CorrelationStep("correlation", N),
             PipeStep("cic", N, window="cic"), CorrelationStep("correlation refused", N, refused=True)]
    return Leg("f", steps, ("spectrum", "helmholtz", "correlation", "spectrum", "cic", "correlation refused", "spectrum",
                            "helmholtz", "correlation", "helmholtz"))


def leg_g(N, Np):
    steps = [DepositStep("alpha 1/3", N, Np, 1.0 / 3.0), DepositStep("alpha 1", N, Np, 1.0),
             DepositStep("alpha 1/2 then NaN", N, Np, 0.5, nan_after=True)]
    return Leg("g", steps, ("alpha 1/3", "alpha 1", "alpha 1/2 then NaN", "alpha 1/3"))


def leg_h(N):
    return Leg("h", [PipeStep("spectrum", N), HelmholtzStep("helmholtz", N), WriteStep("write", N)])


# The transitions legs a - h name, as (what, facts of the previous call, facts of this call): a pattern matches the facts that
# hold every one of its items.  tests/test_gpu_context_state.py asserts them on what the GPU run recorded (leg i) and
# tests/test_context_state_cpu.py on what the orders promise.
REQUIRED = (
    ("a1 library -> script flavour", dict(leg="a1", tag="library"), dict(leg="a1", tag="script")),
    ("a1 script -> library flavour", dict(leg="a1", tag="script"), dict(leg="a1", tag="library")),
    ("a1 default -> band", dict(leg="a1", tag="library"), dict(leg="a1", tag="band")),
    ("a1 band -> deep", dict(leg="a1", tag="band"), dict(leg="a1", tag="deep")),
    ("a1 deep -> default", dict(leg="a1", tag="deep"), dict(leg="a1", tag="library")),
    ("a1 nbins large -> small", dict(leg="a1", tag="many"), dict(leg="a1", tag="wide")),
    ("a1 nbins small -> large", dict(leg="a1", tag="wide"), dict(leg="a1", tag="many")),
    ("a1 same axis and spacing, a prefix of the thresholds", dict(leg="a1", tag="library"), dict(leg="a1", tag="prefix")),
    ("a2 fast -> general", dict(leg="a2", mode=2), dict(leg="a2", tag="asym", mode=0)),
    ("a2 general -> fast", dict(leg="a2", tag="asym", mode=0), dict(leg="a2", mode=2)),
    ("a3 same tables, no_fast_binning on", dict(leg="a3", tag="library", mode=2), dict(leg="a3", tag="nofast", mode=0)),
    ("a3 same tables, no_fast_binning off", dict(leg="a3", tag="nofast", mode=0), dict(leg="a3", tag="library", mode=2)),
    ("a4 no_int_binning on, no upload", dict(leg="a4", sub="int on", mode=2), dict(leg="a4", sub="int off", mode=1)),
    ("a4 no_int_binning off, no upload", dict(leg="a4", sub="int off", mode=1), dict(leg="a4", sub="int on again", mode=2)),
    ("b 256 -> 16", dict(leg="b", kind="spectrum", N=256), dict(leg="b", kind="spectrum", N=16)),
    ("b 16 -> 250", dict(leg="b", kind="spectrum", N=16), dict(leg="b", kind="spectrum", N=250)),
    ("b 250 -> 128", dict(leg="b", kind="spectrum", N=250), dict(leg="b", kind="spectrum", N=128)),
    ("b 128 -> 96", dict(leg="b", kind="spectrum", N=128), dict(leg="b", kind="spectrum", N=96)),
    ("b 96 -> 256", dict(leg="b", kind="spectrum", N=96), dict(leg="b", kind="spectrum", N=256)),
    ("b 256 -> 128 (shared 128-point tables)", dict(leg="b", kind="spectrum", N=256), dict(leg="b", kind="spectrum", N=128)),
    ("b write 256 -> 16", dict(leg="b", kind="write", N=256), dict(leg="b", kind="write", N=16)),
    ("b write 16 -> 250", dict(leg="b", kind="write", N=16), dict(leg="b", kind="write", N=250)),
    ("b write 250 -> 128", dict(leg="b", kind="write", N=250), dict(leg="b", kind="write", N=128)),
    ("b write 128 -> 96", dict(leg="b", kind="write", N=128), dict(leg="b", kind="write", N=96)),
    ("b write 96 -> 256", dict(leg="b", kind="write", N=96), dict(leg="b", kind="write", N=256)),
    ("b write 256 -> 128", dict(leg="b", kind="write", N=256), dict(leg="b", kind="write", N=128)),
    ("c cic -> none", dict(leg="c", window="cic", N=128), dict(leg="c", window=None, N=128)),
    ("c none -> tsc", dict(leg="c", window=None, N=128), dict(leg="c", window="tsc", N=128)),
    ("c tsc -> cic", dict(leg="c", window="tsc", N=128), dict(leg="c", window="cic", N=128)),
    ("c cic 128 -> cic 256", dict(leg="c", window="cic", N=128), dict(leg="c", window="cic", N=256)),
    ("c cic 256 -> x pass at 128 refused", dict(leg="c", window="cic", N=256), dict(leg="c", kind="window-mismatch")),
    ("c refused -> none at 128", dict(leg="c", kind="window-mismatch"), dict(leg="c", window=None, N=128, kind="spectrum")),
    ("c ones 128 -> ones 256", dict(leg="c", window="ones", N=128), dict(leg="c", window="ones", N=256)),
    ("c ones 256 -> ones 128", dict(leg="c", window="ones", N=256), dict(leg="c", window="ones", N=128)),
    ("d packed in scope -> unpacked outside", dict(leg="d", tag="packed"), dict(leg="d", tag="unpacked")),
    ("d unpacked -> packed, another k range", dict(leg="d", tag="unpacked"), dict(leg="d", tag="packed band")),
    ("d packed -> packed band, same (N, G, nchunks)", dict(leg="d", tag="packed"), dict(leg="d", tag="packed band")),
    ("d packed band -> another (G, nchunks)", dict(leg="d", tag="packed band"), dict(leg="d", tag="packed other geometry")),
    ("d another (G, nchunks) -> the first again", dict(leg="d", tag="packed other geometry"), dict(leg="d", tag="packed")),
    ("d packed -> scope left by an exception", dict(leg="d", tag="packed"), dict(leg="d", kind="scope-exception")),
    ("d scope left by an exception -> packed", dict(leg="d", kind="scope-exception"), dict(leg="d", tag="packed")),
    ("e large partial-sum buffer -> small N, few bins", dict(leg="e", tag="most bins"), dict(leg="e", tag="few bins small N")),
    ("e small -> one workgroup per CU", dict(leg="e", tag="few bins small N"), dict(leg="e", tag="one workgroup per CU")),
    ("e most bins -> one workgroup per CU", dict(leg="e", tag="most bins"), dict(leg="e", tag="one workgroup per CU")),
    ("f spectrum -> helmholtz", dict(leg="f", tag="spectrum"), dict(leg="f", kind="helmholtz")),
    ("f helmholtz -> correlation", dict(leg="f", kind="helmholtz"), dict(leg="f", kind="correlation", sub=None)),
    ("f correlation -> spectrum (k tables back)", dict(leg="f", kind="correlation", sub=None), dict(leg="f", tag="spectrum")),
    ("f window set -> correlation refused", dict(leg="f", tag="cic"), dict(leg="f", kind="correlation", sub="refused")),
    ("f refused -> correlation works", dict(leg="f", kind="correlation", sub="refused"), dict(leg="f", kind="correlation", sub=None)),
    ("f correlation -> helmholtz", dict(leg="f", kind="correlation", sub=None), dict(leg="f", kind="helmholtz")),
    ("g 1/3 -> 1", dict(leg="g", tag="alpha 1/3"), dict(leg="g", tag="alpha 1")),
    ("g 1 -> 1/2", dict(leg="g", tag="alpha 1"), dict(leg="g", tag="alpha 1/2 then NaN")),
    ("g NaN refused, 1/2 in force", dict(leg="g", tag="alpha 1/2 then NaN"), dict(leg="g", sub="after NaN")),
    ("g 1/2 -> 1/3", dict(leg="g", sub="after NaN"), dict(leg="g", tag="alpha 1/3")),
    ("h timing on -> off", dict(leg="h", timing=True), dict(leg="h", timing=False)),
    ("h timing off -> on", dict(leg="h", timing=False), dict(leg="h", timing=True)),
)


def matches(pattern, facts):
    return all(facts.get(k) == v for k, v in pattern.items())


def missing_transitions(recorded, legs=None):
    """Names of REQUIRED not found among `recorded` = [(facts of the previous call | None, facts)], for the legs given."""
    out = []
    for what, prev, this in REQUIRED:
        if legs is not None and this["leg"] not in legs:
            continue
        if not any(p is not None and matches(prev, p) and matches(this, f) for p, f in recorded):
            out.append(what)
    return out


def run_order(K, leg, order, recorded, visits=None, extra=None, on_visit=None):
    """The steps of `order` on K, each checked against its own reference right after its call.  A failure names the leg, the
    step and the step it followed."""
    prev, prev_name = None, "a fresh context"
    for i in order:
        step = leg.steps[i]
        calls = step.call(K)
        while True:
            try:
                label, got, facts = next(calls)
            except StopIteration:
                break
            except Exception as e:
                raise AssertionError("leg %s: step '%s' after '%s' raised %s: %s" % (leg.name, step.tag, prev_name, type(e).__name__, e)) from e
            name = "%s%s" % (step.tag, " [%s]" % label if label else "")
            what = "leg %s: step '%s' after '%s'" % (leg.name, name, prev_name)
            facts = dict(facts, leg=leg.name, **(extra or {}))
            facts.setdefault("sub", None)
            recorded.append((prev, facts))
            step.check(label, got, what)
            if on_visit is not None:
                on_visit(step, label, got, what)
            prev, prev_name = facts, name


def promised(leg, extra=None):
    """[(facts of the previous call | None, facts)] of the leg's orders as the steps announce them on the host: what a run on a
    context records, without one."""
    out = []
    for order in leg.orders:
        prev = None
        for i in order:
            for f in leg.steps[i].expected_facts():
                f = dict(f, leg=leg.name, **(extra or {}))
                f.setdefault("sub", None)
                out.append((prev, f))
                prev = f
    return out


B_SIZES = (256, 16, 250, 128, 96)
B_ORDER = (256, 16, 250, 128, 96, 256, 128)
G_PARTICLES = 200_000


def gpu_legs():
    """The legs of tests/test_gpu_context_state.py at the sizes the issue names (no field above 256^3)."""
    return {"a1": leg_a1(128), "a2": leg_a2(128), "a3": leg_a3(128), "a4": leg_a4(128), "b": leg_b(B_SIZES, B_ORDER),
            "c": leg_c(128, 256), "d128": leg_d(128, (4, 2), (2, 4)), "d256": leg_d(256, (8, 2), (4, 4)), "e": leg_e(256, 16),
            "f": leg_f(128), "g": leg_g(64, G_PARTICLES), "h": leg_h(128)}


def cpu_legs():
    """The same legs at the sizes the numpy stand-ins follow in a moment (powers of two; 16 wherever one size does)."""
    return {"a1": leg_a1(16), "a2": leg_a2(16), "a3": leg_a3(16), "a4": leg_a4(16), "b": leg_b((32, 16, 64), (32, 16, 64, 32, 16)),
            "c": leg_c(16, 32), "d": leg_d(16, (2, 2), (4, 1)), "e": leg_e(32, 16), "f": leg_f(16), "g": leg_g(16, 2000),
            "h": leg_h(16)}
