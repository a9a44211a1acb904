"""The torch mirrors of tests/device_ref.py on the CPU against the numpy mirrors they restate (gradient_ref.fields32_all,
filter_ref.fields32_all), value for value, at slab heights that divide N and that do not; the generators, which give the same
tensor whatever the slab height; and the checker, which has to see a wrong output: this is the sensitivity check of the large-grid
tests (tests/test_gpu_large_grids.py) -- no kernel is ever built with a narrowed offset to see them fail."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import device_ref as dr  # noqa: E402
import filter_ref as fr  # noqa: E402
import gradient_ref as gr  # noqa: E402

CPU = torch.device("cpu")
GRADIENT_N, FILTER_NM, slab_heights, whole = dr.GRADIENT_N, dr.FILTER_NM, dr.slab_heights, dr.whole


@pytest.mark.parametrize("N", GRADIENT_N)
def test_gradient_mirror_equals_the_numpy_mirror(N):
    lc = 0.25
    ch = dr.integer_velocity(N, seed=N, device=CPU)
    u = ch[:3].numpy()
    assert np.abs(u).max() == 1024 and np.array_equal(u, np.round(u)) and bool(torch.isnan(ch[3]).all())
    ref = gr.fields32_all(u, lc)
    for what in gr.CODES:
        for slab in slab_heights(N):
            got = whole(N, slab, lambda x0, x1: dr.gradient_slab(ch, lc, what, x0, x1))
            assert got.dtype == np.float32 and got.shape == ref[what].shape
            assert np.array_equal(got, ref[what]), (what, N, slab, int(np.sum(got != ref[what])))
        assert np.abs(ref[what]).max() > 0


@pytest.mark.parametrize("N,m", FILTER_NM)
def test_filter_mirror_equals_the_numpy_mirror(N, m):
    ch = dr.integer_chans(N, seed=100 * N + m, device=CPU)
    refs = fr.fields32_all(ch.numpy(), m)
    for what in fr.CODES:
        for slab in slab_heights(N):
            got = whole(N, slab, lambda x0, x1: dr.filter_slab(ch, m, what, x0, x1))
            assert got.dtype == np.float32 and got.shape == refs[what].shape
            assert np.array_equal(got, refs[what]), (what, N, m, slab, int(np.sum(got != refs[what])))
        assert np.abs(refs[what]).max() > 0
    assert (refs["vm"][3] == 0).any() and (refs["vm"][3] > 0).any()          # the M = 0 path ran, and the other one


def test_filter_sums_are_shared_between_the_codes():
    """filter_form of ONE set of sums gives both codes: what a test does that wants the eleven sums once."""
    N, m = 18, 8
    ch = dr.integer_chans(N, seed=3, device=CPU)
    refs = fr.fields32_all(ch.numpy(), m)
    s, has = dr.filter_sums(ch, m, 0, N)
    for what in fr.CODES:
        assert np.array_equal(dr.filter_form(s, has, m, what).numpy(), refs[what]), what


@pytest.mark.parametrize("N", [6, 18, 70])
def test_generators_do_not_depend_on_the_slab_height(N):
    for make in (dr.integer_velocity, dr.integer_chans):
        first = make(N, 7, CPU, slab=N)
        for slab in (1, 5, 64):
            again = make(N, 7, CPU, slab=slab)
            assert np.array_equal(first.numpy(), again.numpy(), equal_nan=True), (make.__name__, N, slab)
        assert not np.array_equal(first[:3].numpy(), make(N, 8, CPU)[:3].numpy())           # the seed counts
        assert not torch.equal(first[0, 0], first[0, 1]) and not torch.equal(first[0], first[1])    # planes and channels differ
    ch = dr.integer_chans(N, 7, CPU).numpy()
    hole = min(N - 1, 19)
    assert set(np.unique(ch[3])) == {0.0, 1.0, 2.0} and np.abs(ch[:3]).max() == 3 and not ch[3, :hole, :hole, :hole].any()
    assert (ch[3, hole:] > 0).mean() > 0.6


def test_planes_wrap_on_both_sides():
    N = 6
    f = torch.arange(N ** 3, dtype=torch.float32).reshape(N, N, N)
    got = dr.planes(f, -2, N + 2)
    assert torch.equal(got, f[[4, 5, 0, 1, 2, 3, 4, 5, 0, 1]])
    got[0] = -1
    assert f[4, 0, 0] == 4 * N * N                                  # a copy, never a view
    one = dr.planes(f, 2, 3)
    one[0] = -1
    assert f[2, 0, 0] == 2 * N * N


def _counts(got, ref, slab):
    N = ref.shape[1]
    return [dr.compare(got, torch.from_numpy(ref[:, x0:x1]), x0) for x0, x1 in dr.slabs(N, slab)]


def test_checker_sees_a_wrong_output_at_the_right_slab():
    N, lc, slab = 18, 0.5, 5                                        # slabs 0..4, 5..9, 10..14, 15..17
    ch = dr.integer_velocity(N, seed=1, device=CPU)
    ref = gr.fields32(ch[:3].numpy(), lc, "strain_rate")
    good = torch.from_numpy(ref).clone()
    assert _counts(good, ref, slab) == [0, 0, 0, 0]
    assert dr.first_difference(good, torch.from_numpy(ref[:, 5:10]), 5) is None and dr.count_nan(good) == 0
    # two planes swapped in every channel
    bad = good.clone()
    bad[:, 7], bad[:, 12] = good[:, 12], good[:, 7]
    n = _counts(bad, ref, slab)
    assert n[0] == 0 and n[3] == 0 and n[1] > 0.9 * 6 * N * N and n[2] > 0.9 * 6 * N * N, n
    k, x, y, z, off = dr.first_difference(bad, torch.from_numpy(ref[:, 5:10]), 5)
    assert (k, x) == (0, 7) and off == (7 * N + y) * N + z
    # one channel shifted by one row, in the planes of one slab
    bad = good.clone()
    bad[4, 10:15] = torch.roll(good[4, 10:15], 1, dims=1)
    n = _counts(bad, ref, slab)
    assert n[:2] == [0, 0] and n[3] == 0 and n[2] > 0.9 * 5 * N * N, n
    assert dr.first_difference(bad, torch.from_numpy(ref[:, 10:15]), 10)[:2] == (4, 10)
    # one element left at the poison
    bad = good.clone()
    bad[2, 16, 3, 5] = float("nan")
    assert _counts(bad, ref, slab) == [0, 0, 0, 1] and dr.count_nan(bad) == 1
    where = dr.first_difference(bad, torch.from_numpy(ref[:, 15:18]), 15)
    assert where == (2, 16, 3, 5, ((2 * N + 16) * N + 3) * N + 5)
    assert "channel 2 at (16, 3, 5)" in dr.describe(bad, torch.from_numpy(ref[:, 15:18]), 15)
    # the same for the filter's reference: a slab of it against a correct output and one that is off by one cell in z
    chf = dr.integer_chans(N, seed=2, device=CPU)
    reff = fr.fields32(chf.numpy(), 2, "stress")
    assert dr.compare(torch.from_numpy(reff), dr.filter_slab(chf, 2, "stress", 5, 10), 5) == 0
    # (the boxes of 13 x 13 of the 18 x 18 cells of these planes lie inside the empty cube: 155 cells per plane hold a stress)
    assert dr.compare(torch.from_numpy(np.roll(reff, 1, axis=3)), dr.filter_slab(chf, 2, "stress", 5, 10), 5) > 0.5 * 6 * 5 * 155


def test_whole_tensor_walks_cover_every_piece(monkeypatch):
    """fill, count_nan and checksum with pieces far smaller than the tensor, and a remainder piece."""
    monkeypatch.setattr(dr, "PIECE", 1000)
    t = torch.zeros((3, 7, 11, 13), dtype=torch.float32)
    dr.fill(t, float("nan"))
    assert dr.count_nan(t) == t.numel()
    dr.fill(t, 2.0)
    assert dr.count_nan(t) == 0 and bool((t == 2.0).all())
    before = dr.checksum(t)
    assert len(before) == -(-t.numel() // 1000)
    for where in ((0, 0, 0, 0), (2, 6, 10, 12), (1, 3, 5, 7)):
        t[where] = 2.5
        assert dr.checksum(t) != before
        t[where] = 2.0
        assert dr.checksum(t) == before


def test_gradient_layout_is_the_launch_formula():
    """gradient_ref.layout at the sizes whose chunking the GPU tests name, for the 256 CUs of an MI355X."""
    assert gr.layout(128) == (64, 4) and gr.layout(250) == (84, 2) and gr.layout(16) == (16, 4) and gr.layout(96) == (96, 4)
    assert gr.layout(896) == (150, 4) and gr.layout(898) == (300, 2) and gr.layout(1028) == (257, 4) and gr.layout(1026) == (513, 2)
    assert fr.layout(896) == (64, 4) and fr.layout(898) == (60, 2) and fr.layout(1028) == (61, 4) and fr.layout(1026) == (61, 2)
