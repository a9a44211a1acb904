"""The two nearest-neighbour references of tests/test_gpu_nn_matrix.py (oracle/gpu_checks.py: nn_brute_force, nn_slab_reference)
pinned to orc.exact_nn_lattice on the CPU, the proof behind `certified` put to the test (an empty box, a k one too small), the
set-up of every GPU leg run at a scaled-down particle count, and the cell-list geometries of the GPU legs through vps_nn_plan
(host only)."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import vps_oracle as orc  # noqa: E402
from oracle import gpu_checks as chk  # noqa: E402

CPU = torch.device("cpu")
N = 24
NP = 20_000

# uniform and reaching beyond the particles on both sides; one axis descending; no axis uniform
LATTICES = {
    "uniform": lambda: [np.linspace(-0.08, 1.07, N)] * 3,
    "descending": lambda: [chk.nn_uniform_axis(N), chk.nn_uniform_axis(N)[::-1].copy(), chk.nn_uniform_axis(N)],
    "jittered": lambda: [chk.nn_jittered_axis(N, 5 + a) for a in range(3)],
}
_CASES = {}


def _case(name, dtype):
    """(numpy axes, torch axes, pos, k, oracle indices [N^3]) of a lattice: computed once, shared, never modified."""
    key = (name, dtype)
    if key not in _CASES:
        axes = LATTICES[name]()
        pos, nbar = chk.nn_matrix_particles(CPU, NP, dtype, axes, 0, N, seed=3, ndup=300)
        taxes = [chk._axis(a, CPU) for a in axes]
        k = chk.nn_search_k(nbar, chk.nn_gap_min(taxes))
        want = torch.as_tensor(orc.exact_nn_lattice(pos.numpy(), *axes))
        _CASES[key] = (axes, taxes, pos, k, want)
    return _CASES[key]


def test_the_particles_have_the_features_the_matrix_needs():
    axes, taxes, pos, k, want = _case("uniform", torch.float64)
    p = pos.numpy()
    assert p.min() >= 0 and p.max() < 1 and axes[0][0] < 0 and axes[0][-1] > 1                            # queries outside the box
    c = np.array([0.5 * (axes[0][0] + axes[0][-1]), axes[1][N // 2], axes[2][N // 2]])
    assert (np.abs(p[: NP // 10] - c).max(axis=1) < 0.06).all()                                         # the clump
    first = {tuple(q) for q in p[:-300]}
    assert all(tuple(q) in first for q in p[-300:])                                                       # duplicates: exact ties
    h = axes[0][1] - axes[0][0]
    lo = np.array([axes[0][0], axes[1][N // 5], axes[2][N // 5]]) - 0.25 * h
    assert not ((p >= lo) & (p < lo + 10 * h)).all(axis=1).any()                                          # the empty box
    lattice = {(x, y, z) for x in axes[0] for y in axes[1] for z in axes[2]}
    assert sum(tuple(q) in lattice for q in p) >= 8                                                       # particles ON lattice points
    # ties exist and the oracle gives them to the lower index
    assert (want < NP - 300).all() and np.isin(p[-300:, 0], p[want.numpy(), 0]).any()
    assert chk.nn_search_k(nbar=0.9 * NP, gap_min=chk.nn_gap_min(taxes)) == k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_brute_force_equals_the_oracle(dtype):
    axes, taxes, pos, k, want = _case("uniform", dtype)
    for x0, nx in ((0, 4), (10, 4)):                 # (the first rows lie outside the particles' box, the others cross the clump)
        flat = torch.arange(nx * N * N)
        idx, best = chk.nn_brute_force(pos, chk.lattice_points(taxes, x0, nx, flat), batch=256, chunk=7000)
        assert torch.equal(idx, want[x0 * N * N:(x0 + nx) * N * N])
        q = chk.lattice_points(taxes, x0, nx, flat).numpy()
        d = q - pos.numpy().astype(np.float64)[idx.numpy()]
        assert np.array_equal(best.numpy(), (d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2)


@pytest.mark.parametrize("name", sorted(LATTICES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_slab_reference_equals_the_oracle(name, dtype):
    """Whole lattice and two slabs: every certified point is the oracle's; the empty box leaves uncertified ones, none of them is
    skipped, and brute force settles each to the oracle's answer."""
    axes, taxes, pos, k, want = _case(name, dtype)
    assert k >= 2
    for x0, nx in ((0, N), (0, 5), (N - 7, 7)):
        idx, best, cert = chk.nn_slab_reference(pos, taxes, x0, nx, k, budget=1 << 20)
        w = want[x0 * N * N:(x0 + nx) * N * N]
        assert torch.equal(idx[cert], w[cert])
        nopen = int((~cert).sum())
        if x0 == 0:
            assert 0 < nopen <= chk.NN_UNCERTIFIED_CAP       # (the empty box starts at the slab's first row)
        if nx == N:
            assert not torch.equal(idx, w) or name != "uniform", "the empty box was meant to defeat the local search somewhere"
        assert chk.nn_settle(pos, taxes, x0, nx, idx, best, cert) == nopen
        assert torch.equal(idx, w)
        q = chk.lattice_points(taxes, x0, nx, torch.arange(nx * N * N)).numpy()
        d = q - pos.numpy().astype(np.float64)[idx.numpy()]
        assert np.array_equal(best.numpy(), (d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2)


@pytest.mark.parametrize("name", sorted(LATTICES))
def test_a_k_one_too_small_certifies_less_and_nothing_wrong(name):
    axes, taxes, pos, k, want = _case(name, torch.float32)
    counts = []
    for kk in (k, k - 1, k - 2):
        idx, best, cert = chk.nn_slab_reference(pos, taxes, 0, N, kk)
        assert torch.equal(idx[cert], want[cert]), kk
        counts.append(int((~cert).sum()))
    assert counts[0] < counts[1] < counts[2], counts
    with pytest.raises(AssertionError, match="uncertified"):
        chk.nn_settle(pos, taxes, 0, N, idx, best, cert, cap=counts[2] - 1)


def test_the_cap_refuses_before_anything_is_compared():
    axes, taxes, pos, k, want = _case("uniform", torch.float32)
    idx, best, cert = chk.nn_slab_reference(pos, taxes, 0, N, k)
    before = idx.clone()
    with pytest.raises(AssertionError):
        chk.nn_settle(pos, taxes, 0, N, idx, best, cert, cap=0)
    assert torch.equal(idx, before)


@pytest.mark.parametrize("leg", chk.NN_MATRIX, ids=lambda l: l["name"])
def test_every_gpu_leg_stays_under_the_cap_at_a_scaled_down_count(leg):
    """The uncertified count depends on nbar h^3 (through k) and on the slab's rows, not on the particle count: the leg's set-up
    on a 48^3 lattice of the same kind with the same nbar h^3, its first slab's rows (at most 48).  The count is asserted as
    the GPU leg asserts it, and what is left open equals brute force."""
    kind, NL = leg["lattice"]
    n_small = 48
    n = int(round(leg["n"] * ((n_small - 1) / (NL - 1)) ** 3))
    axes = chk.nn_matrix_axes((kind, n_small), seed=11)
    nx = min(leg["slabs"][0][1], n_small)
    x0 = 0 if leg["slabs"][0][0] == 0 else (n_small - nx) // 2
    pos, nbar = chk.nn_matrix_particles(CPU, n, getattr(torch, leg["dtype"]), axes, x0, nx, seed=2, ndup=min(1000, n // 50))
    taxes = [chk._axis(a, CPU) for a in axes]
    big = chk.nn_matrix_axes(leg["lattice"], seed=11)
    k = chk.nn_search_k(nbar, chk.nn_gap_min(taxes))
    k_big = chk.nn_search_k(0.9 * leg["n"], min(float(np.abs(np.diff(a)).min()) for a in big))
    assert abs(k - k_big) <= (1 if kind == "jittered" else 0), (k, k_big)     # (a jittered axis of 48 points has a larger smallest gap)
    idx, best, cert = chk.nn_slab_reference(pos, taxes, x0, nx, k, budget=1 << 21)
    nopen = int((~cert).sum())
    print("%s: k = %d, %d of %d points uncertified at n = %d" % (leg["name"], k, nopen, cert.numel(), n))
    assert nopen <= chk.NN_UNCERTIFIED_CAP
    pick = torch.nonzero(~cert).squeeze(1)[:64]
    pick = torch.cat([pick, torch.arange(0, cert.numel(), max(1, cert.numel() // 64))])
    chk.nn_settle(pos, taxes, x0, nx, idx, best, cert)
    bi, bb = chk.nn_brute_force(pos, chk.lattice_points(taxes, x0, nx, pick), batch=64, chunk=1 << 14)
    assert torch.equal(idx[pick], bi) and torch.equal(best[pick], bb)


# np -> (M, gshift, ngroups, lds_fine, sorted) of nn_layout; gshift None: the counting sort has no groups to speak of
GEOMETRY = {400_000: (64, 9, 512, 2112, 1), 3_000_000: (125, 12, 477, 16448, 1), 7_000_000: (167, 14, 285, 65600, 1),
            14_000_000: (210, 15, 283, 131136, 1), 27_000_000: (262, 15, 549, 131136, 1), 50_000_000: (321, 15, 1010, 131136, 1),
            100_000_000: (405, 15, 2028, 131136, 1), 105_000_000: (412, None, 2135, 0, 0)}


def test_nn_plan_reproduces_the_geometry_table():
    from vpower import _ffi, device
    for n, (M, gshift, ngroups, lds_fine, sorted_) in GEOMETRY.items():
        for f64 in (False, True):
            p = device.nn_plan(n, f64, 8 * 1024 * 1024)
            assert (p["M"], p["ngroups"], p["lds_fine"], p["sorted"]) == (M, ngroups, lds_fine, sorted_), (n, p)
            assert p["ncell"] == M ** 3 and p["nchunks"] == -(-n // 4096)
            assert gshift is None or p["gshift"] == gshift, (n, p)
            assert p["lds_scatter"] == (4 * (6 * 4096 + 2 * ngroups + 16) if sorted_ else 0), (n, p)
    assert GEOMETRY[7_000_000][3] > 64 * 1024 >= device.nn_plan(6_000_000)["lds_fine"]      # gshift 14: the first over 64 KiB
    assert device.nn_plan(100_000_000)["ngroups"] <= 2048 < device.nn_plan(105_000_000)["ngroups"]
    for leg in chk.NN_MATRIX:                                                               # the GPU legs name these geometries
        p = device.nn_plan(leg["n"], leg["dtype"] == "float64")
        assert {f: p[f] for f in leg["plan"]} == leg["plan"], (leg["name"], p)
    # the switch into the bucket sort: four chunks of 4096 particles
    assert [device.nn_plan(n)["sorted"] for n in (16383, 16384, 16385)] == [0, 1, 1]
    # the option nn_build_atomic is read as nn_layout reads it
    with _ffi.option("nn_build_atomic", 1):
        p = device.nn_plan(50_000_000)
        assert (p["sorted"], p["lds_fine"], p["M"]) == (0, 0, 321)
    assert device.nn_plan(50_000_000)["sorted"] == 1
    with pytest.raises(_ffi.VpsError):
        device.nn_plan(0)


def test_abi_10_declares_the_nn_queries():
    from vpower import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vps_hip.h")).read()
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION >= 10
    assert int(re.search(r"#define VPS_NN_PLAN_FIELDS (\d+)", hdr).group(1)) == len(_ffi.NN_PLAN_FIELDS)
    lib = _ffi.lib()
    assert lib.vps_version() == _ffi.ABI_VERSION and hasattr(lib, "vps_nn_plan") and hasattr(lib, "vps_nn_last_search")
    assert lib.vps_nn_plan(1000, 0, 0, None) < 0 and lib.vps_nn_last_search(None, None) < 0      # a status code, never a crash
