"""Guarded, poisoned, exact-size memory for the real entry points of vpower.device.HipKernels.

Every output of the wrapper class comes from self.empty / self.zeros and every workspace from self.workspace.  GuardedAllocator
overrides those three and nothing else; guarded_kernels() puts it in front of the wrapper class, so that the library's own calls
run on memory in which a skipped store, a store next to a buffer and a workspace formula that is short all show:

  arena     [front guard | payload | rear guard], one private allocation per buffer.  The payload is exactly the bytes asked for
            and starts on a 256-byte boundary; each guard is at least GUARD_BYTES long and holds GUARD_BYTE in every byte, so
            that its 32-bit words are neither 0 nor a NaN nor all ones: a stray zeroing store, a stray poison and a stray NaN
            are all visible.
  empty     payload = 0xFF bytes: NaN as float32 / float64 / complex64, -1 as int32 / int64, the maximum of an unsigned type.
  zeros     payload = 0 (accumulators are read-modify-write), same guards.
  workspace payload = exactly the nbytes the library's *_workspace_bytes function returned, in the state the test chose:
            state "Z": a fresh arena, zero-filled;
            state "D": the arena the LAST call with this key left behind, as it left it -- the payload view cut to the new nbytes
                       and the rear guard rewritten over whatever lies behind it.  D-same is a real call of the same shape on
                       other data before the tested one, D-other a real call of a larger shape.  No synthetic pattern ever goes
                       into a workspace: a stale word is always one a real call wrote.
            Inside `with G.sequence():` the first request of a key applies the state and every later one of the same size gets
            the SAME tensor (same data_ptr), for call sequences that legitimately read what the call before left (the reuse_sort
            token, share_energy, the two-slot exchange).

check() reports on every buffer handed out since the last check(): the offset of the first changed byte of either guard (None:
intact) and, for `empty` outputs, the flat indices of the elements that still hold the poison.  It then lets go of the outputs
(their arenas live as long as the caller's tensors, no longer) and keeps only the workspaces, for state "D"; release() drops those.

TEST INFRASTRUCTURE ONLY.  Device-agnostic: tests/test_guarded_cpu.py pins all of the above on CPU tensors."""
import contextlib

import torch

GUARD_BYTES = 1 << 20
GUARD_BYTE = 0x5A           # 0x5A5A5A5A: 1.5e16 as float32, 1.5e9 as int32; 0x5A5A5A5A5A5A5A5A: 1.7e128 as float64
POISON_BYTE = 0xFF
ALIGN = 256


class Report:
    """What check() found for one buffer.  front / rear: offset (bytes, from the guard's first byte) of the first changed byte,
    None if intact.  poison: for an `empty` output the sorted flat indices (int64, on the host) of the elements still holding
    the poison, else None."""

    def __init__(self, name, kind, ptr, nbytes, shape, dtype, front, rear, poison):
        self.name, self.kind, self.ptr, self.nbytes = name, kind, ptr, nbytes        # name of a workspace: its key
        self.shape, self.dtype, self.front, self.rear, self.poison = shape, dtype, front, rear, poison

    def findings(self):
        """Names of the checks this buffer fails: "front guard", "rear guard" ("poison" is for the caller to judge: only it
        knows which elements the contract leaves unwritten)."""
        return [n for n, v in (("front guard", self.front), ("rear guard", self.rear)) if v is not None]

    def __repr__(self):
        return "Report(%s: front %r, rear %r, poison %s)" % (self.name, self.front, self.rear,
                                                             None if self.poison is None else "%d elements" % len(self.poison))


class _Arena:
    def __init__(self, device, nbytes):
        self.capacity = int(nbytes)
        self.raw = torch.empty(2 * GUARD_BYTES + ALIGN + self.capacity, dtype=torch.uint8, device=device)
        self.off = GUARD_BYTES + (-(self.raw.data_ptr() + GUARD_BYTES)) % ALIGN
        self.nbytes = self.capacity
        self.raw[: self.off] = GUARD_BYTE
        self.write_rear_guard()

    def write_rear_guard(self):
        self.raw[self.off + self.nbytes:] = GUARD_BYTE

    def payload(self):
        return self.raw[self.off: self.off + self.nbytes]

    @staticmethod
    def _first_changed(guard):
        bad = guard != GUARD_BYTE
        if not bool(bad.any()):
            return None
        return int(torch.nonzero(bad)[0, 0])

    def guards(self):
        return self._first_changed(self.raw[: self.off]), self._first_changed(self.raw[self.off + self.nbytes:])


def poison_mask(t):
    """Per element of t: does it still hold the poison?  Floating and complex types: any of its real scalars is the all-ones
    word (no arithmetic produces that NaN, and a complex store that skipped one half is still reported); integer types: the
    whole element is all ones (the upper half of a small negative int64 is all ones legitimately)."""
    if t.is_complex():
        return poison_mask(torch.view_as_real(t)).any(dim=-1)
    if t.dtype == torch.float32:
        return t.view(torch.int32) == -1
    if t.dtype == torch.float64:
        return t.view(torch.int64) == -1
    if t.dtype in (torch.int32, torch.int64, torch.int16, torch.int8):
        return t == -1
    if t.dtype == torch.uint8:
        return t == 0xFF
    raise TypeError("no poison rule for %s" % t.dtype)


class GuardedAllocator:
    """empty / zeros / workspace of the kernels wrapper on guarded arenas of `device` (see the module docstring)."""

    def __init__(self, device):
        self._init_guarded(device)

    def _init_guarded(self, device):
        self.device = torch.device(device)
        self.state = "Z"
        self._handed = []          # (kind, name, arena, shape, dtype) since the last check()
        self._kept = {}            # key -> arena of the last workspace of that key
        self._held = None          # inside sequence(): key -> (nbytes, tensor)
        self._serial = 0

    # -- the three overrides ----------------------------------------------------------
    def _output(self, kind, shape, dtype, fill):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        a = _Arena(self.device, n * item)
        a.payload().fill_(fill)
        t = a.payload().view(dtype).view(shape)
        assert t.data_ptr() % ALIGN == 0 and t.numel() == n
        self._serial += 1
        self._handed.append((kind, "%s#%d" % (kind, self._serial), a, shape, dtype))
        return t

    def empty(self, shape, dtype):
        return self._output("empty", shape, dtype, POISON_BYTE)

    def zeros(self, shape, dtype):
        return self._output("zeros", shape, dtype, 0)

    def workspace(self, key, nbytes):
        nbytes = int(nbytes)
        if self._held is not None and key in self._held:
            held_bytes, t = self._held[key]
            if held_bytes == nbytes:
                return t
        if self.state == "Z":
            a = _Arena(self.device, nbytes)
            a.payload().zero_()
        elif self.state == "D":
            a = self._kept.get(key)
            if a is None or a.capacity < nbytes:
                raise AssertionError("state D: no earlier call left a %r workspace of at least %d bytes (have %s)"
                                     % (key, nbytes, None if a is None else a.capacity))
            a.nbytes = nbytes
            a.write_rear_guard()
        else:
            raise ValueError("state must be 'Z' or 'D', not %r" % (self.state,))
        self._kept[key] = a
        t = a.payload()
        assert t.data_ptr() % ALIGN == 0 and t.numel() == nbytes
        self._handed.append(("workspace", key, a, (nbytes,), torch.uint8))
        if self._held is not None:
            self._held[key] = (nbytes, t)
        return t

    # -- what the tests drive -----------------------------------------------------------
    @contextlib.contextmanager
    def sequence(self):
        """Calls that legitimately read what the one before left in the workspace: one unit, one workspace tensor."""
        self._held = {}
        try:
            yield
        finally:
            self._held = None

    def check(self):
        """One Report per buffer handed out since the last check() (a workspace handed out several times: one); forgets the
        outputs, keeps the workspaces for state 'D'."""
        out, seen = [], set()
        for kind, name, a, shape, dtype in self._handed:
            if id(a) in seen:
                continue
            seen.add(id(a))
            front, rear = a.guards()
            poison = None
            if kind == "empty":
                mask = poison_mask(a.payload().view(dtype)).reshape(-1)
                poison = torch.nonzero(mask).reshape(-1).cpu()
            out.append(Report(name, kind, a.raw.data_ptr() + a.off, a.nbytes, shape, dtype, front, rear, poison))
        self._handed = []
        return out

    def workspace_bytes(self, key):
        """A copy of the payload the last workspace of `key` holds now (uint8, on the device)."""
        return self._kept[key].payload().clone()

    def release(self):
        """Drops every arena this allocator still holds."""
        self._handed = []
        self._kept = {}
        self._held = None


def report_of(reports, tensor):
    """The Report of the buffer `tensor` was handed out as."""
    for r in reports:
        if r.ptr == tensor.data_ptr():
            return r
    raise KeyError("no report for the tensor at %#x" % tensor.data_ptr())


def guard_findings(reports):
    """[(buffer name, check name, offset)] of every guard that changed."""
    return [(r.name, n, r.front if n == "front guard" else r.rear) for r in reports for n in r.findings()]


def guarded_kernels(device=None):
    """The kernels wrapper vpower.device.default_kernels() returns, with a context of its own, on guarded memory."""
    from vpower import device as D

    class GuardedHipKernels(GuardedAllocator, D.HipKernels):
        def __init__(self, device=None):
            D.HipKernels.__init__(self, device)
            self._init_guarded(self.device)

    return GuardedHipKernels(device)
