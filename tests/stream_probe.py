"""The stream contract of libvps_hip.so (include/vps_hip.h, "Streams") as tables, and the probe tests/test_gpu_streams.py runs every
entry point through.

Tables.  Every vps_* symbol of vpower/_ffi.py is in exactly one of
  NONBLOCKING  pure enqueues on the context's stream: the call returns while the stream is still busy.  (A call that has to
               regrow or rebuild a table the CONTEXT owns -- the x pass's partial sums, the chunk tables of vps_fft_y, the axes
               scratch -- drains the stream first, that once; the legs that reach those sites are marked blocking.)
  BLOCKING     return only after the stream has drained: they bring a value to the host, or (vps_pair_k, vps_memcpy_h2d) take
               host data whose copy they complete before returning.  A blocking leg asserts that the blocker HAS finished.
  HOST_ONLY    nothing is enqueued and no device memory is read or written
and each symbol of the first two names the leg (a key of LEGS) that runs it behind the blocker.

The probe (run_case).  On the null stream the call's device inputs hold a DECOY -- other, equally valid data of the same shapes
-- and the call has run once on them (workspace state "D-same" of tests/guarded.py; tables and code objects exist).  Then, on a
side stream S: a blocker (torch.cuda._sleep), an event behind it, the TRUE data copied into the input buffers device to device,
the call.  A non-blocking call must return before the blocker's event has completed ("blocker too short" otherwise: the leg is
inconclusive and FAILS); the outputs are read back on S and compared with the float64 reference of the true data at the route's
existing bar.  Whatever was enqueued off S, or read before S allowed it, saw the decoy: valid numbers, wrong answer.  Per leg
the decoy's own reference differs from the true one by more than 100 times the bar (asserted on the host).  No NaN and no
out-of-range value is ever handed to a kernel.

TEST INFRASTRUCTURE ONLY."""
import contextlib
import time

import numpy as np

PSUM_RTOL = 2e-5          # shell sums against the float64 oracle: the project's bar (tests/test_gpu_configs.py)
FFT_RTOL = 1e-5           # rfft3 / images: max error over the rms of the reference (tests/test_gpu_guarded.py: IMAGE_BAR)
FIELD_BAR = 1e-5          # fields: max error over the maximum of the reference (tests/test_gpu_guarded.py)
GUARD_FACTOR = 100.0      # the decoy's reference must miss the true one by this many bars
BLOCKER_MS = 200.0        # see tests/test_gpu_streams.py (module docstring) and DESIGN.md section 5

# symbol -> leg of tests/test_gpu_streams.py that runs it behind the blocker
NONBLOCKING = {
    "vps_set_stream": "switch_sort_workspace",
    "vps_memset": "memory_helpers",
    "vps_cell_index": "cell_index",
    "vps_deposit_ngp": "deposit_c4",
    "vps_deposit_field": "deposit_field",
    "vps_deposit_fft_zy": "fused_whole",
    "vps_density_velocity_vector": "density_velocity_vector",
    "vps_field_algebra": "field_algebra",
    "vps_field_algebra_out": "field_algebra_out",
    "vps_assign_expand": "assign_expand_cic",
    "vps_deposit_assign": "deposit_assign_cic",
    "vps_fft_zy": "raw_fft_zy_and_power_bin",
    "vps_fft_zy_weighted": "fft_zy_weighted",
    "vps_fft_z": "fft_z",
    "vps_deposit_fft_z": "deposit_fft_z",
    "vps_fft_y": "fft_y_chunk_packed",
    "vps_fft_x": "fft_x_bin",
    "vps_fft_x_bin": "fft_x_bin_multi",
    "vps_fft_x_bin_chunk": "fft_x_bin_chunk",
    "vps_fft_x_bin_helmholtz": "fft_x_bin_helmholtz",
    "vps_fft_x_bin_chunk_helmholtz": "fft_x_bin_chunk_helmholtz",
    "vps_spectrum_zimages": "library_exchange",
    "vps_allreduce_shells": "library_exchange",
    "vps_power_bin": "raw_fft_zy_and_power_bin",
    "vps_rfft3": "rfft3",
    "vps_power_grid": "power_grid",
}
# symbol -> (leg, what it brings to the host)
BLOCKING = {
    "vps_destroy": ("destroy_with_work_pending", "drains the stream before the context's tables are freed"),
    "vps_sync": ("memory_helpers", "that is its purpose"),
    "vps_memcpy_h2d": ("memory_helpers", "the copy from the caller's host buffer is complete on return"),
    "vps_memcpy_d2h": ("memory_helpers", "the bytes"),
    "vps_timing_reset": ("timing", "events in use go back to the pool"),
    "vps_timing_get": ("timing", "elapsed times"),
    "vps_timing_list": ("timing", "elapsed times"),
    "vps_preprocess": ("preprocess", "minimum and bulk velocity"),
    "vps_totals": ("totals", "five sums"),
    "vps_count_in_slab": ("deposit_fft_z_slab", "the count"),
    "vps_deposit_fft_z_slab": ("deposit_fft_z_slab", "the compaction counter of a slab-sized sort"),
    "vps_nn_resample": ("nn_resample-column", "bounding box of the particles (and the open-point count under timing)"),
    "vps_nn_resample_field": ("nn_resample_field-column", "as vps_nn_resample"),
    "vps_nn_resample_quantity": ("nn_resample_quantity-column", "as vps_nn_resample"),
    "vps_set_binning": ("tables_binning", "changed tables: earlier launches may still read the old ones"),
    "vps_set_window": ("tables_window", "changed table: earlier launches may still read the old one"),
    "vps_comm_destroy": ("library_exchange", "drains the communication stream"),
    "vps_pair_k": ("pair_k", "the copies of the caller's host axes are complete on return"),
    "vps_hist_pairs": ("hist_pairs", "the edges live in a device buffer of the call's own"),
}
HOST_ONLY = (
    "vps_create", "vps_last_error", "vps_version", "vps_set_option", "vps_get_option", "vps_device_info", "vps_binning_mode",
    "vps_malloc", "vps_free", "vps_timing_enable", "vps_deposit_workspace_bytes", "vps_deposit_fft_zy_supported",
    "vps_deposit_fft_zy_workspace_bytes", "vps_deposit_fft_zy_workspace_bytes_shared", "vps_nn_workspace_bytes", "vps_nn_plan",
    "vps_nn_last_search", "vps_fft_supported", "vps_set_bin_only", "vps_set_density_weight", "vps_deposit_assign_workspace_bytes",
    "vps_deposit_assign_plan", "vps_fft_workspace_bytes", "vps_fft_zimage_bytes", "vps_deposit_fft_z_workspace_bytes",
    "vps_deposit_fft_z_workspace_bytes_slab", "vps_deposit_plan", "vps_fft_y_chunk_elems", "vps_fft_y_packed",
    "vps_fft_y_chunk_block", "vps_comm_unique_id", "vps_comm_create", "vps_comm_info", "vps_spectrum_zimages_workspace_bytes",
    "vps_power_workspace_bytes", "vps_hist_max_bins",
)


# ------------------------------------------------------------------------------------------- comparing ----
def _host(x):
    """numpy float64 / complex128 / integer array of a tensor or array."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return x.astype(np.complex128)
    return x.astype(np.float64) if x.dtype.kind == "f" else x


def error_in_bars(got, ref, kind):
    """How many bars `got` misses `ref` by (<= 1 passes).  kind: "exact" | "field" (max error / FIELD_BAR max |ref|) | "image"
    (max error / FFT_RTOL rms ref) | "psum" (per element, PSUM_RTOL relative, no absolute term) | ("rel", r) | ("abs", a)."""
    g, r = _host(got), _host(ref)
    if g.shape != r.shape:
        return float("inf")
    if not np.all(np.isfinite(g)):
        return float("inf")
    if kind == "exact":
        return 0.0 if np.array_equal(g, r) else float("inf")
    err = np.abs(g - r)
    if kind == "field":
        return float(err.max() / (FIELD_BAR * np.abs(r).max()))
    if kind == "image":
        return float(err.max() / (FFT_RTOL * np.sqrt(np.mean(np.abs(r) ** 2))))
    if kind == "psum":
        kind = ("rel", PSUM_RTOL)
    if isinstance(kind, tuple) and kind[0] == "rel":
        if np.any((r == 0) & (g != 0)):
            return float("inf")
        nz = r != 0
        return float(np.max(err[nz] / (kind[1] * np.abs(r[nz])), initial=0.0))
    if isinstance(kind, tuple) and kind[0] == "abs":
        return float(np.max(err / kind[1]))
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------- the blocker ----
class Blocker:
    """torch.cuda._sleep of BLOCKER_MS, calibrated once with events (or, without _sleep, a chain of elementwise operations)."""

    def __init__(self, device, ms=BLOCKER_MS):
        import torch
        self.torch, self.device, self.ms = torch, device, ms
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.buf = None if self.sleep else torch.zeros(1 << 26, dtype=torch.float32, device=device)
        self.units = 1
        unit = 10_000_000 if self.sleep else 8
        t = self._time(unit)
        t = self._time(unit)                       # (the second: the first pays for loading the kernel)
        self.units = max(1, int(unit * ms / max(t, 1e-3)))
        self.measured_ms = self._time(self.units)
        self.enqueue_ms = []                       # (leg, host milliseconds of the non-blocking call behind the blocker)

    def _go(self, units):
        if self.sleep:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                self.buf.mul_(1.0000001).add_(1e-9)

    def _time(self, units):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        self._go(units)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def enqueue(self):
        self._go(self.units)


class Case:
    """One leg.  bufs: the device tensors the call reads (they hold the decoy); true: what goes into them on S; call() -> list of
    outputs (tensors or arrays); ref / decoy_ref: float64 references of the true and of the decoy data; kinds: one bar per output
    (error_in_bars); indep: indices of outputs that do not depend on the data (shell counts); blocking: the call drains the stream
    (asserted: the blocker has finished when it returns); bitwise: the same call on the null stream gives the same bits; warm: what runs on the decoy first (default: call)."""

    def __init__(self, name, bufs, true, call, ref, decoy_ref, kinds, blocking=False, bitwise=True, indep=(), warm=None, reset=None):
        self.name, self.bufs, self.true, self.call, self.ref, self.decoy_ref, self.kinds = name, bufs, true, call, ref, decoy_ref, kinds
        self.blocking, self.bitwise, self.indep, self.warm, self.reset = blocking, bitwise, tuple(indep), warm, reset


def _outputs_to_host(outs):
    return [_host(o) for o in outs]


def run_case(case, blocker):
    """The six steps of the module docstring; returns the outputs read back on S (host arrays)."""
    torch = blocker.torch
    assert len(case.ref) == len(case.decoy_ref) == len(case.kinds)
    assert len(case.bufs) == len(case.true)
    guarded = 0
    for i, (rt, rd, kind) in enumerate(zip(case.ref, case.decoy_ref, case.kinds)):
        if i in case.indep:
            continue
        miss = error_in_bars(rd, rt, kind)
        assert miss >= GUARD_FACTOR, "%s: the decoy's reference of output %d is only %.3g bars from the true one" % (case.name, i, miss)
        guarded += 1
    assert guarded >= 1, "%s: no output depends on the data" % case.name
    for b, t in zip(case.bufs, case.true):
        assert b.shape == t.shape and b.dtype == t.dtype and b.data_ptr() != t.data_ptr()
    (case.warm or case.call)()                      # on the decoy: workspaces as a real call leaves them, tables built
    if case.reset:
        case.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=blocker.device)
    with torch.cuda.stream(side):
        blocker.enqueue()
        behind = torch.cuda.Event()
        behind.record(side)
        for b, t in zip(case.bufs, case.true):
            b.copy_(t, non_blocking=True)
        t0 = time.perf_counter()
        outs = case.call()
        ms = (time.perf_counter() - t0) * 1e3
        pending = not behind.query()
        if case.blocking:
            assert not pending, "%s is listed as blocking but returned after %.2f ms with the stream still busy" % (case.name, ms)
        else:
            blocker.enqueue_ms.append((case.name, ms))
            assert pending, ("blocker too short: %s returned after %.1f ms of host time, the blocker (%.0f ms) had already finished -- "
                             "or the call waited for the stream, which the contract says it does not" % (case.name, ms, blocker.measured_ms))
        got = _outputs_to_host(outs)               # read back on S
    side.synchronize()
    print("%s: %s after %.2f ms of host time (blocker %s)" % (case.name, "returned" if not case.blocking else "returned (blocking)", ms,
                                                              "pending" if pending else "finished"))
    assert len(got) == len(case.ref), (case.name, len(got), len(case.ref))
    for i, (g, r, kind) in enumerate(zip(got, case.ref, case.kinds)):
        miss = error_in_bars(g, r, kind)
        away = error_in_bars(g, case.decoy_ref[i], kind)
        print("  output %d (%s): %.3g bars from the reference, %.3g from the decoy's" % (i, kind, miss, away))
        assert miss <= 1.0, ("%s on a side stream: output %d misses its float64 reference by %.3g bars (%s); it is %.3g bars from the "
                             "DECOY's reference" % (case.name, i, miss, kind, away))
    if case.bitwise:
        for b, t in zip(case.bufs, case.true):
            b.copy_(t)
        if case.reset:
            case.reset()
        null = _outputs_to_host(case.call())
        torch.cuda.synchronize()
        for i, (g, n) in enumerate(zip(got, null)):
            assert g.shape == n.shape and np.array_equal(g.view(np.uint8), n.view(np.uint8)), (
                "%s: output %d on the side stream differs from the same call on the null stream in %d elements"
                % (case.name, i, int(np.sum(g != n))))
    return got


@contextlib.contextmanager
def options(opts):
    from vpower import _ffi
    with contextlib.ExitStack() as stack:
        for k, v in opts.items():
            stack.enter_context(_ffi.option(k, v))
        yield
