"""tests/guarded.py pinned without a GPU: torch CPU tensors and plain functions that stand in for kernels.  Every planted
defect must be reported by the check named for it and by no other; a correct function gives no finding in any workspace state.
Run anywhere:  python -m pytest tests/test_guarded_cpu.py -q"""
import gc
import weakref

import numpy as np
import pytest
import torch

import guarded as gd

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.float64, torch.complex64, torch.int32, torch.int64, torch.uint8]
N = 1000          # elements of the stand-ins' outputs


@pytest.fixture
def G():
    g = gd.GuardedAllocator(CPU)
    yield g
    g.release()


# ---- stand-ins for kernels: out[i] = 2 x[i] + (a running count kept in the workspace) -----------------------------------------
def _elem(t, index):
    """A one-element view at `index` elements from t's first (negative / past the end: into the arena's guards)."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + index)


def correct(G, x, skip=None, stray=None, short=0, stale=False):
    """Fills the workspace with x, then out = 2 * workspace.  skip: an output element left unwritten; stray: an element index
    (relative to out) written besides; short: the workspace is asked for with that many bytes too few, as a size formula that
    is short would; stale: word 0 of the workspace is read before anything wrote it (added to out[0])."""
    n = x.numel()
    out = G.empty((n,), torch.float32)
    work = G.workspace("standin", 4 * n - short)
    wv = work.view(torch.float32)
    w = torch.as_strided(wv, (n,), (1,), wv.storage_offset())            # the n words the kernel believes in
    before = float(w[0]) if stale else 0.0
    w.copy_(x)
    res = 2 * w
    res[0] += before
    if skip is None:
        out.copy_(res)
    else:
        out[:skip] = res[:skip]
        out[skip + 1:] = res[skip + 1:]
    if stray is not None:
        _elem(out, stray).fill_(7.0)
    return out


def _x(seed, n=N):
    return torch.as_tensor(np.random.default_rng(seed).integers(1, 100, n).astype(np.float32))


def _all_findings(reports, written_everywhere=True):
    """{(buffer kind, check)}: guards that changed, and "poison" for an output with elements left."""
    out = {(r.kind, n) for r in reports for n in r.findings()}
    out |= {(r.kind, "poison") for r in reports if r.poison is not None and len(r.poison)}
    return out


# ---- layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_poison_reads_as_nan_minus_one_or_maximum(G, dtype):
    t = G.empty((3, 5), dtype)
    assert t.shape == (3, 5) and t.dtype == dtype and t.is_contiguous()
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
    elif dtype.is_complex:
        assert bool(torch.isnan(t.real).all()) and bool(torch.isnan(t.imag).all())
    elif dtype == torch.uint8:
        assert bool((t == 255).all())
    else:
        assert bool((t == -1).all())
    assert bool(gd.poison_mask(t).all())
    z = G.zeros((3, 5), dtype)
    assert bool((z == 0).all()) and not bool(gd.poison_mask(z).any())
    (r, rz) = G.check()
    assert r.kind == "empty" and np.array_equal(r.poison.numpy(), np.arange(15)) and r.findings() == []
    assert rz.kind == "zeros" and rz.poison is None and rz.findings() == []


def test_guard_words_are_not_zero_nan_or_all_ones():
    a = gd._Arena(CPU, 12)
    assert a.off >= gd.GUARD_BYTES and a.raw.numel() - a.off - a.nbytes >= gd.GUARD_BYTES
    front = a.raw[: a.off]
    assert bool((front == gd.GUARD_BYTE).all()) and bool((a.raw[a.off + 12:] == gd.GUARD_BYTE).all())
    w32 = front[: 1024].view(torch.int32)
    assert bool((w32 != 0).all()) and bool((w32 != -1).all())
    assert not bool(torch.isnan(front[: 1024].view(torch.float32)).any())
    assert not bool(torch.isnan(front[: 1024].view(torch.float64)).any())
    assert not bool(torch.isinf(front[: 1024].view(torch.float32)).any())
    assert gd.GUARD_BYTE != gd.POISON_BYTE and gd.GUARD_BYTE != 0


@pytest.mark.parametrize("nbytes", [0, 1, 4, 255, 256, 257, 4097])
def test_payload_is_exact_and_aligned(G, nbytes):
    w = G.workspace("k", nbytes)
    assert w.numel() == nbytes and w.dtype == torch.uint8 and w.data_ptr() % 256 == 0
    assert bool((w == 0).all())                                           # state Z
    t = G.empty((nbytes,), torch.uint8)
    assert t.data_ptr() % 256 == 0
    for shape, dtype in (((7,), torch.complex64), ((3, 3), torch.float64)):
        assert G.empty(shape, dtype).data_ptr() % 256 == 0
    assert all(r.findings() == [] for r in G.check())


def test_arena_is_released_with_the_buffer(G):
    t = G.empty((10,), torch.float32)
    raw = weakref.ref(t._base if t._base is not None else t)
    G.workspace("k", 64)
    G.check()
    assert raw() is not None                                             # the caller's tensor keeps its arena
    del t
    gc.collect()
    assert raw() is None, "an output's arena must go with the output"
    kept = weakref.ref(G._kept["k"].raw)
    assert kept() is not None                                            # the workspace stays for state D ...
    G.release()
    gc.collect()
    assert kept() is None                                                # ... until release()


# ---- planted defects ---------------------------------------------------------------------------------------------------------
def test_correct_function_has_no_finding_in_any_state(G):
    x, ref = _x(1), 2 * _x(1)
    outs = {}
    G.state = "Z"
    outs["Z"] = correct(G, x)
    assert _all_findings(G.check()) == set()
    correct(G, _x(2))                                                     # a real call of the same shape on other data
    G.check()
    G.state = "D"
    outs["D-same"] = correct(G, x)
    assert _all_findings(G.check()) == set()
    G.state = "Z"
    correct(G, _x(3, 3 * N))                                              # a real call of a larger shape
    G.check()
    G.state = "D"
    outs["D-other"] = correct(G, x)
    rep = G.check()
    assert _all_findings(rep) == set()
    assert [r.nbytes for r in rep if r.kind == "workspace"] == [4 * N]    # cut to the new size
    for name, o in outs.items():
        assert torch.equal(o, ref), name


@pytest.mark.parametrize("skip", [0, N // 2, N - 1], ids=["first", "middle", "last"])
def test_unwritten_element_is_reported_by_the_poison_check_only(G, skip):
    out = correct(G, _x(1), skip=skip)
    rep = G.check()
    assert _all_findings(rep) == {("empty", "poison")}
    assert gd.report_of(rep, out).poison.tolist() == [skip]


def test_store_before_the_start_is_reported_by_the_front_guard_only(G):
    out = correct(G, _x(1), stray=-1)
    rep = G.check()
    assert _all_findings(rep) == {("empty", "front guard")}
    r = gd.report_of(rep, out)
    assert r.front == G_front_len(r, out) - 4 and r.rear is None
    assert gd.guard_findings(rep) == [(r.name, "front guard", r.front)]


def G_front_len(r, out):
    """Bytes of the front guard of the arena behind `out`."""
    return out.storage_offset() * out.element_size()


def test_store_past_the_end_is_reported_by_the_rear_guard_only(G):
    out = correct(G, _x(1), stray=N)
    rep = G.check()
    assert _all_findings(rep) == {("empty", "rear guard")}
    assert gd.report_of(rep, out).rear == 0 and gd.report_of(rep, out).front is None


def test_stray_store_into_a_zeros_buffer_guard(G):
    acc = G.zeros((16,), torch.int64)
    _elem(acc, 16).fill_(0)                                               # a stray ZEROING store
    _elem(acc, -1).fill_(-1)                                              # a stray poison
    (r,) = G.check()
    assert r.findings() == ["front guard", "rear guard"] and r.rear == 0 and r.poison is None


@pytest.mark.parametrize("state", ["Z", "D"])
def test_workspace_256_bytes_short_trips_the_rear_guard_only(G, state):
    x = _x(1)
    if state == "D":
        correct(G, _x(3, 3 * N))
        G.check()
    G.state = state
    correct(G, x, short=256)
    rep = G.check()
    assert _all_findings(rep) == {("workspace", "rear guard")}
    (w,) = [r for r in rep if r.kind == "workspace"]
    assert w.nbytes == 4 * N - 256 and w.rear == 0 and w.name == "standin"


def test_stale_workspace_read_shows_between_the_states(G):
    x, ref = _x(1), 2 * _x(1)
    G.state = "Z"
    z = correct(G, x, stale=True)
    assert _all_findings(G.check()) == set()
    correct(G, _x(2), stale=True)
    G.check()
    G.state = "D"
    d = correct(G, x, stale=True)
    assert _all_findings(G.check()) == set()                              # no guard, no poison: only the comparison sees it
    assert torch.equal(z, ref) and not torch.equal(d, ref) and not torch.equal(z, d)
    assert torch.nonzero(z != d).reshape(-1).tolist() == [0]


def test_state_d_needs_an_earlier_call_of_at_least_that_size(G):
    G.state = "D"
    with pytest.raises(AssertionError, match="no earlier call"):
        G.workspace("k", 64)
    G.state = "Z"
    G.workspace("k", 64)
    G.state = "D"
    with pytest.raises(AssertionError, match="no earlier call"):
        G.workspace("k", 65)
    assert G.workspace("k", 64).numel() == 64


def test_state_d_keeps_the_bytes_and_rewrites_the_rear_guard(G):
    G.state = "Z"
    w = G.workspace("k", 1024)
    w.copy_(torch.arange(1024) % 251)
    ptr = w.data_ptr()
    G.check()
    G.state = "D"
    v = G.workspace("k", 512)
    assert v.data_ptr() == ptr and v.numel() == 512
    assert torch.equal(v, (torch.arange(512) % 251).to(torch.uint8))      # a real call's leftovers, not a pattern
    (r,) = G.check()
    assert r.findings() == [] and r.nbytes == 512                         # the dirt behind the cut is guard again
    assert torch.equal(G.workspace_bytes("k"), v)


@pytest.mark.parametrize("state", ["Z", "D"])
def test_sequence_hands_out_one_workspace(G, state):
    G.workspace("k", 4096).fill_(3)
    G.check()
    G.state = state
    with G.sequence():
        a = G.workspace("k", 2048)
        a[:8] = 9
        b = G.workspace("k", 2048)
        assert a.data_ptr() == b.data_ptr() and bool((b[:8] == 9).all())
        assert bool((b[8:] == (0 if state == "Z" else 3)).all())
        other = G.workspace("j", 16) if state == "Z" else None
        assert other is None or other.data_ptr() != a.data_ptr()
    rep = G.check()
    assert [r.name for r in rep if r.name == "k"] == ["k"]                # one buffer, one report
    c = G.workspace("k", 2048)
    assert (c.data_ptr() == a.data_ptr()) == (state == "D")               # outside a sequence the state applies again
