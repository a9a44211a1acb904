"""The state a context carries between calls: ONE vps_ctx through sequences of different configurations.

Every other GPU test configures a context in one way, calls and moves on.  Here a step (a configuration, a call, its float64
reference computed up front: tests/context_sequences.py) runs in several orders on a context of this module's own -- a freshly
constructed HipKernels per order, never default_kernels(), so that no other module warms it -- and every call is compared with
its own reference right after it.  Every step is the first call on a fresh context in some order and follows every step it
shares a cache key with in some order (context_sequences.covering_orders; tests/test_context_state_cpu.py holds the orders to
that and runs them on a kernel set without state).  A failure names the leg, the step and the step it followed.

What the context keeps (csrc/vps_internal.h) and the leg that walks it:
  a. binning tables, their "same tables" shortcut and the derived mode (d_k2 / d_thr / h_k2 / h_thr, bin_fast, bin_int, d_nthr):
     flavours, k ranges, bin counts, a bit-equal PREFIX of the thresholds with fewer bins (what a shortcut that forgot nbins would
     skip), a table that is not mirrored, the options no_fast_binning (read at upload) and no_int_binning (read at use);
  b. fft_tables, keyed by complex length NC: the z pass of N takes NC = N / 2 and the y and x passes NC = N (fft.hip: fft_z_of,
     fft_y_of, fft_x_impl), so 16 touches {8, 16}, 96 {48, 96}, 128 {64, 128}, 250 {125, 250} and 256 {128, 256}: 128 and 256
     share the 128-point tables, no other two of these sizes share a length.  Binned and in write mode;
  c. the window (d_win / win_N / h_win) and its shortcut, the refusal of an x pass at N under a window for another N, and a
     table of ones at 128 and 256: bit-equal over the shorter length, what a shortcut that forgot N would skip;
  d. the row cut, binning_only() and the plane tables of the chunked exchange (d_kcut / h_kcut, ypack, bin_only), the slab
     decomposition emulated through the production calls; a scope left by an exception;
  e. the partial-sum buffer (d_xpart / xpart_cap), sized by the largest workgroups x bins product first;
  f. the Helmholtz accumulator and the real-space lattice (vps_fft_x modes 5 - 7) between spectra; the refusal under a window;
  g. the density exponent (weight_alpha), and a refused NaN;
  h. the timing switch and its event pool;
  i. (last) the ordered pairs of host-side facts the legs recorded cover context_sequences.REQUIRED.

Equality between visits.  Whether two identical calls give bit-identical results is measured, not assumed: leg b's probe runs
every step type as the first call on two fresh contexts.  Measured on an MI355X (gfx950) on 2026-10-21: bit-equal for every
step type -- Psum of PowerPipeline.spectrum at 16, 96, 128, 250 and 256 and every mode of the write-mode x pass at the same
sizes.  So a later visit of a whole-grid spectrum or of a write-mode pass must equal the first visit bit for bit, on top of its
own reference (PSUM_VISITS_BIT_EQUAL / WRITE_VISITS_BIT_EQUAL below; the probe fails if that stops being what the device does).
The emulated exchange, the Helmholtz sums, the correlation and the deposits (whose LDS adds come in any order) were not probed
and are held to their references alone.  Shell counts are bit-equal to the exact counts at every visit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import context_sequences as cs  # noqa: E402

# Outcome of leg b's probe on an MI355X (gfx950), 2026-10-21.  True: visits are held to bit-equality; False: every visit is held to
# its float64 reference alone (PSUM_RTOL / MODE_RTOL).  The probe fails if a True here stops being what the device does.
PSUM_VISITS_BIT_EQUAL = True
WRITE_VISITS_BIT_EQUAL = True

LEGS = cs.gpu_legs()
RECORDED = []        # (facts of the previous call on the context | None, facts of this call), every leg
RAN = set()          # legs that ran to their end


@pytest.fixture(scope="module")
def dev():
    d = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.reset_peak_memory_stats()
    yield d
    print("\ntest_gpu_context_state: peak device memory %.2f GB" % (torch.cuda.max_memory_allocated() / 1e9))
    cs.release()
    cs._PARTICLES.clear()
    torch.cuda.empty_cache()


def _fresh():
    from vpower import device
    return device.HipKernels()


def _visits():
    """on_visit of cs.run_order: the first result of every (step, label) is kept; a later visit is held to it where the probe
    found the device to repeat itself bit for bit."""
    first = {}

    def on_visit(step, label, got, what):
        if step.kind == "write":
            if WRITE_VISITS_BIT_EQUAL:
                prev = first.setdefault((step.tag, label), got)
                assert prev is got or torch.equal(prev, got), (what, "differs from the first visit")
        elif step.kind in ("spectrum", "raw") and PSUM_VISITS_BIT_EQUAL:
            prev = first.setdefault((step.tag, label), got)
            assert prev is got or np.array_equal(prev[0], got[0]), (what, "Psum differs from the first visit")
    return on_visit


def _run_leg(name, dev):
    leg = LEGS[name]
    leg.make_refs(dev)
    on_visit = _visits()
    for order in leg.orders:
        K = _fresh()
        try:
            cs.run_order(K, leg, order, RECORDED, on_visit=on_visit)
        finally:
            K.close()
    RAN.add(name)


# ----------------------------------------------------------------------------------------- b. probe, then size switches ----
def test_b_probe_two_fresh_contexts(dev):
    """Every step type of leg b as the FIRST call on two fresh contexts: are the results bit-equal?  Prints the finding per
    step; fails if the module claims bit-equality that the device does not show."""
    leg = LEGS["b"]
    leg.make_refs(dev)
    for step in leg.steps:
        got = []
        for _ in range(2):
            K = _fresh()
            try:
                for label, g, _f in step.call(K):
                    step.check(label, g, "probe of '%s' on a fresh context" % step.tag)
                    got.append(g)
            finally:
                K.close()
        if step.kind == "write":
            equal = torch.equal(got[0], got[1])
            diff = float((got[0] - got[1]).abs().max() / got[0].abs().square().mean().sqrt()) / cs.MODE_RTOL
            print("probe %-14s bit-equal: %-5s  max |difference| / rms = %.3g MODE_RTOL" % (step.tag, equal, diff))
            assert equal or not WRITE_VISITS_BIT_EQUAL, step
        else:
            assert np.array_equal(got[0][1], got[1][1]), (step, "shell counts")
            equal = np.array_equal(got[0][0], got[1][0])
            diff = float(np.max(np.abs(got[0][0] - got[1][0]) / np.abs(step.ref[0]))) / cs.PSUM_RTOL
            print("probe %-14s Psum bit-equal: %-5s  max relative difference = %.3g PSUM_RTOL" % (step.tag, equal, diff))
            assert equal or not PSUM_VISITS_BIT_EQUAL, step


def test_b_size_switches(dev):
    """256 -> 16 -> 250 -> 128 -> 96 -> 256 -> 128 through PowerPipeline.spectrum (three components), the same order through
    fft_zy + fft_x_write against every exact mode, then every other order of context_sequences.covering_orders."""
    _run_leg("b", dev)


# ------------------------------------------------------------------------------------------------- a. binning tables ----
def test_a1_flavours_k_ranges_and_bin_counts(dev):
    _run_leg("a1", dev)


def test_a2_fast_general_fast(dev):
    """Mirrored tables, then a k2 axis made asymmetric on purpose through set_binning, then mirrored again: 2 -> 0 -> 2."""
    _run_leg("a2", dev)
    modes = [f["mode"] for _, f in RECORDED if f["leg"] == "a2"][:3]
    assert modes == [2, 0, 2], modes


def test_a3_same_tables_under_no_fast_binning(dev):
    """The same tables uploaded again with no_fast_binning set: the upload must not take the shortcut (mode 0), nor the next."""
    _run_leg("a3", dev)
    modes = [f["mode"] for _, f in RECORDED if f["leg"] == "a3"][:3]
    assert modes == [2, 0, 2], modes


def test_a4_no_int_binning_is_read_at_use(dev):
    """no_int_binning toggled between calls with no upload in between: 2 -> 1 -> 2."""
    _run_leg("a4", dev)
    modes = [f["mode"] for _, f in RECORDED if f["leg"] == "a4" and f["tag"] == "toggle"][:3]
    assert modes == [2, 1, 2], modes


# ---------------------------------------------------------------------------------------------------------- c. window ----
def test_c_window_tables(dev):
    _run_leg("c", dev)


# ------------------------------------------------------------------------- d. row cut, binning_only, packed exchange ----
@pytest.mark.parametrize("N", [128, 256])
def test_d_row_cut_scope_and_packed_exchange(dev, N):
    _run_leg("d%d" % N, dev)


# ---------------------------------------------------------------------------------------------- e. partial-sum buffer ----
def test_e_partial_sum_buffer_sized_by_the_largest_call_first(dev):
    leg = LEGS["e"]
    leg.make_refs(dev)
    big, small, one = leg.steps
    assert big.nbins > 16 * small.nbins and small.N < big.N
    _run_leg("e", dev)


# ------------------------------------------------------------------------------- f. Helmholtz and real-lattice modes ----
def test_f_helmholtz_correlation_and_spectra_interleaved(dev):
    _run_leg("f", dev)


# ------------------------------------------------------------------------------------------------ g. density exponent ----
def test_g_density_exponent(dev):
    """alpha 1/3 -> 1 -> 1/2 -> (NaN refused: 1/2 stays) -> 1/3: deposit_field and the pencil route, VPS_WEIGHTED_VELOCITY and
    VPS_DENSITY, each visit against weighted_ref / density_ref; the first and the last visit to 1/3 against the SAME reference
    (the deposits add in LDS in any order: tests/test_gpu_weighted.py, so agreement is through the per-cell bar)."""
    leg = LEGS["g"]
    assert any(s.tag == "alpha 1/3" for s in leg.steps) and leg.orders[0][0] == leg.orders[0][-1]
    _run_leg("g", dev)
    assert all(f.get("sub") for _, f in RECORDED if f["leg"] == "g")
    assert any(f["sub"] == "weighted pencil" for _, f in RECORDED if f["leg"] == "g"), "the pencil route did not run at N = 64"


# ----------------------------------------------------------------------------------------------- h. timing on and off ----
def test_h_timing_switched_in_mid_sequence(dev):
    leg = LEGS["h"]
    leg.make_refs(dev)
    on_visit = _visits()
    K = _fresh()
    counts = []
    try:
        for on in (True, False, True):
            K.timing(on)                      # (enable + reset: the events of the visit before go back to the pool)
            cs.run_order(K, leg, range(len(leg.steps)), RECORDED, extra={"timing": on}, on_visit=on_visit)
            K.sync()
            counts.append({k: n for k, (n, _) in K.timing_get().items()})
        K.timing(False)
    finally:
        K.close()
    assert counts[0]["fft_x"] > 0 and counts[0]["fft_z"] > 0 and counts[0]["fft_y"] > 0, counts[0]
    assert all(n == 0 for n in counts[1].values()), counts[1]
    assert counts[2] == counts[0], (counts[0], counts[2])
    # the three visits follow each other on one context: the recorded pairs at the seams
    seams = [(p, f) for p, f in RECORDED if f["leg"] == "h" and p is None]
    assert len(seams) == 3
    RECORDED.extend([({"leg": "h", "timing": a}, {"leg": "h", "timing": b, "sub": None}) for a, b in ((True, False), (False, True))])
    RAN.add("h")


# -------------------------------------------------------------------------------------------------- i. coverage guard ----
def test_i_recorded_transitions_cover_the_required_list(dev):
    """Runs last, after the WHOLE file: the ordered pairs of host-side facts the legs recorded cover every transition that
    context_sequences.REQUIRED writes out.  A partial run (-k, --lf, one leg alone) has not recorded every leg and fails here by
    design; the message says so."""
    whole = "(this check needs every leg of the file to have run in the same session: %s ran)" % sorted(RAN)
    assert RAN == set(LEGS), whole
    missing = cs.missing_transitions(RECORDED)
    assert missing == [], (missing, whole)
