"""Host side of the direct CIC / TSC deposit (vps_deposit_assign, ABI 13): the ABI surface, the record's weight words restated in
numpy against tests/small_ref.py, the exactness of the half-cell lattice the GPU test relies on, and the `method=` keyword.
No GPU needed."""
import os
import re

import numpy as np
import pytest

import assign_direct_ref as adr
import small_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vps_deposit_assign_workspace_bytes", "vps_deposit_assign", "vps_deposit_assign_plan")
EPS = 2.0 ** -24


def test_abi_13_exports_the_direct_deposit():
    from vpower import _ffi
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION == 13
    lib = _ffi.lib()
    assert lib.vps_version() == 13
    bound = {name for name, _, _ in _ffi.SYMBOLS}
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in bound and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, code), name
    assert int(re.search(r"#define VPS_DEPOSIT_ASSIGN_PLAN_FIELDS (\d+)", hdr).group(1)) == len(_ffi.DEPOSIT_ASSIGN_PLAN_FIELDS)


def test_workspace_query_is_a_pure_function_and_refuses_bad_arguments():
    from vpower import _ffi
    lib = _ffi.lib()
    q = lib.vps_deposit_assign_workspace_bytes
    for order in (2, 3):
        for C in (1, 3, 4):
            small, large = q(10 ** 5, C, 128, order), q(10 ** 6, C, 128, order)
            # two record arrays of C + 7 words and 12 bytes of keys and ranks per particle, plus tables
            assert small > 10 ** 5 * (8 * (C + 7) + 12) and large > small
            assert large < 10 ** 6 * (8 * (C + 7) + 12) * 1.2
            # ... which is far below what the expansion route needs: its arrays and the NGP workspace of order^3 sub-particles
            S = order ** 3
            assert large * 4 < S * 10 ** 6 * (12 + 4 * C) + lib.vps_deposit_workspace_bytes(S * 10 ** 6, C, 128, 128)
    assert q(0, 4, 128, 2) > 0
    for bad in ((-1, 4, 128, 2), (10, 2, 128, 2), (10, 5, 128, 2), (10, 4, 0, 2), (10, 4, 128, 1), (10, 4, 128, 4)):
        assert q(*bad) == 0, bad


def _hard_positions(N, L, dtype):
    """Faces, centres, their float neighbours, within 1e-9 of a cell of both, outside the box and far outside it."""
    rng = np.random.default_rng(N)
    lc = L / N
    i = np.array([0, 1, 2, N // 2, N - 2, N - 1, N], dtype=np.float64)
    faces, centres = i * lc, (i + 0.5) * lc
    col = np.concatenate([
        faces, centres,
        np.nextafter(faces.astype(dtype), dtype(-np.inf)), np.nextafter(faces.astype(dtype), dtype(np.inf)),
        np.nextafter(centres.astype(dtype), dtype(-np.inf)), np.nextafter(centres.astype(dtype), dtype(np.inf)),
        centres[1:] + 1e-9 * lc, centres[1:] - 1e-9 * lc, faces[1:] + 1e-9 * lc, faces[1:] - 1e-9 * lc,
        [-0.3 * L, 1.7 * L, -L, 2 * L, 0.0, -0.0, L, 1e10, -1e10, 3e7 * L, -2.9e8 * lc],
        rng.random(4000) * L,
    ])
    return np.stack((col, col[::-1], np.roll(col, 7)), axis=1).astype(dtype)


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N,L", [(250, 2.5), (96, 1.0), (16, 1.0), (2048, 1.0)])
def test_record_weight_words_against_small_ref(N, L, dtype, assignment):
    """The weights the kernel forms from the six words of a record -- CIC the words themselves, TSC a a / 2, 1/2 + a b, b b / 2 --
    are the float64 weights of small_ref.assign_weights to 3 * 2^-24 of THEMSELVES, however small; they are not negative and
    add up to one."""
    pos = _hard_positions(N, L, dtype)
    _, w64 = sr.assign_weights(pos, N, L, assignment)
    words = adr.record_words(pos, N, L, assignment)
    w = adr.weights_from_words(words, assignment)
    assert w.dtype == np.float32 and w.shape == w64.shape
    assert np.all(w >= 0) and np.all(words >= 0)
    wd = w.astype(np.float64)
    tiny = float(np.finfo(np.float32).tiny)
    assert np.all(np.abs(wd - w64) <= 3 * EPS * w64 + tiny), np.max(np.abs(wd - w64) / np.maximum(w64, tiny))
    assert np.all(np.abs(wd.sum(axis=-1) - 1) <= 3 * 3 * EPS)
    if assignment == "tsc":
        s = pos.astype(np.float64) / (L / float(N))
        d = s - (np.floor(s) + 0.5)
        assert np.all(np.abs(wd[..., 1] - (0.75 - d * d)) <= 3 * EPS)
    else:
        # a weight of 1e-9 next to a cell centre keeps its relative precision: the word is the rounded float64 weight
        small = (w64 > 0) & (w64 < 1e-6)
        assert small.any() and np.all(np.abs(wd[small] - w64[small]) <= EPS * w64[small])


@pytest.mark.parametrize("assignment", ["cic", "tsc"])
@pytest.mark.parametrize("N,bricks", [(16, (16, 8, 16)), (96, (4, 8, 64)), (65, (4, 8, 64)), (250, (4, 8, 64))])
def test_half_cell_lattice_is_dyadic_and_covers_every_cell(N, bricks, assignment):
    """What the bit-exact GPU test assumes, checked in float64: positions are the same numbers in float32, every weight is a
    multiple of 1/8 (so every product a multiple of 2^-9), payloads are small integers, no cell sees more than a few hundred
    contributions, every cell of the grid sees one, and the first and last cell of every brick are aimed at from every offset."""
    pos, f, L = adr.lattice_particles(N, assignment, bricks, 4, seed=N)
    order = sr.ORDER[assignment]
    assert L / N == adr.LCELL and np.array_equal(pos.astype(np.float32).astype(np.float64), pos)
    assert np.array_equal(f, np.round(f)) and np.abs(f).max() <= 8
    c0, w = sr.assign_weights(pos, N, L, assignment)
    assert np.array_equal(w * 8, np.round(w * 8)) and np.all(w >= 0) and np.all(w.sum(axis=-1) == 1)
    words = adr.record_words(pos, N, L, assignment)
    assert np.array_equal(adr.weights_from_words(words, assignment).astype(np.float64), w)     # the kernel's weights: exact too
    cells, n = adr.contribution_counts(pos, N, L, assignment)
    assert len(cells) == N ** 3, "every cell of the grid receives something"
    assert n.max() * 8 * 2 ** 9 < 2 ** 24, "partial sums stay exact in float32"
    assert n.max() <= 600
    for a, bw in enumerate(bricks):
        firsts = np.arange(0, N, bw)
        for e in np.unique(np.concatenate((firsts, np.minimum(firsts + bw, N) - 1))):
            for j in range(order):
                hit = (c0[:, a] + j) % N == e
                assert np.any(hit & (w[:, a, j] > 0)), (a, e, j)


def test_method_keyword_is_checked_before_the_device():
    from vpower import interp
    pos, f = np.zeros((4, 3)), np.ones(4)
    with pytest.raises(ValueError, match="method"):
        interp.deposit_to_grid(f, pos, 16, 1.0, assignment="cic", method="scatter")
    with pytest.raises(ValueError, match="method"):
        interp.deposit_to_grid(f, pos, 16, 1.0, method=None)
    gp = interp.GasParticles(pos, np.ones(4), np.ones(4), np.zeros((4, 3)), 1.0)
    with pytest.raises(ValueError, match="method"):
        gp.deposit_to_field(16, "tsc", method="Direct")
    assert interp.METHODS == ("expand", "direct")
