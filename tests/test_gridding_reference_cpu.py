"""The reference helpers of tests/test_gpu_gridding_matrix.py (oracle/gpu_checks.py) pinned to the oracle, on the CPU: the exact
slab histogram against orc.deposit_to_grid, the constructed particles' cells against orc.cell_index -- every particle, at
every (N, L, dtype) of the GPU matrix -- and the refactored ngp_moments_float64 against a direct restatement."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import vps_oracle as orc  # noqa: E402
from oracle import gpu_checks as chk  # noqa: E402

CPU = torch.device("cpu")


@pytest.mark.parametrize("N,L", [(16, 1.0), (24, 2.5), (50, 1.0)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_exact_slab_reference_equals_oracle_deposit(N, L, dtype):
    cells, pos, rho, vel = chk.constructed_particles(CPU, 60_000, N, L, dtype, "uniform", seed=N, chunk=25_000)
    want = orc.deposit_to_grid(np.concatenate([rho.numpy()[:, None], rho.numpy()[:, None] * vel.numpy()], axis=1).astype(np.float64),
                               pos.numpy(), N, L)                                   # [N, N, N, 4]
    rows = N // 2
    for x0 in range(0, N, rows):
        got = chk.exact_slab_reference(cells, rho, vel, N, x0, rows)
        for c in range(4):
            assert got[c].dtype == torch.int64
            assert np.array_equal(got[c].numpy().reshape(rows, N, N), want[x0:x0 + rows, :, :, c])
    pay = torch.randint(-3, 4, (cells.shape[0], 3))
    got = chk.exact_slab_reference(cells, None, None, N, 0, N, payload=pay)
    want = orc.deposit_to_grid(pay.numpy().astype(np.float64), pos.numpy(), N, L)
    assert all(np.array_equal(got[c].numpy().reshape(N, N, N), want[..., c]) for c in range(3))
    # the float64 fields of the same totals are the oracle's
    f = chk.float64_slab_fields(cells, rho, vel, N, L, 0, N, ("velocity", "mass", "momentum", "energy"))
    vec = orc.density_velocity_vector(vel.numpy().astype(np.float64), rho.numpy().astype(np.float64))
    v, m = orc.vm_from_vec_grid(orc.deposit_to_grid(vec, pos.numpy(), N, L), L / N, zero_empty=True)
    assert np.allclose(f["mass"][0].numpy().reshape(N, N, N), m, rtol=1e-14, atol=0)
    for c in range(3):
        assert np.allclose(f["velocity"][c].numpy().reshape(N, N, N), v[..., c], rtol=1e-13, atol=1e-15)
        assert np.allclose(f["momentum"][c].numpy().reshape(N, N, N), v[..., c] * m, rtol=1e-13, atol=1e-18)
    assert np.allclose(f["energy"][0].numpy().reshape(N, N, N), orc.kinetic_energy_field(v[..., 0], v[..., 1], v[..., 2], m),
                       rtol=1e-13, atol=0)


@pytest.mark.parametrize("N,L,dtype", chk.GRIDDING_MATRIX)
@pytest.mark.parametrize("dist", chk.DISTRIBUTIONS)
def test_every_constructed_cell_is_the_oracles(N, L, dtype, dist):
    """100 % of 10^6 particles per distribution, wrapped / outside-box positions included."""
    n = 1_000_000
    cells, pos, rho, vel = chk.constructed_particles(CPU, n, N, L, getattr(torch, dtype), dist, seed=7, wrap=0.25, chunk=300_000,
                                                     per_cell=1 << 20)
    assert cells.shape == (n, 3) and pos.dtype == getattr(torch, dtype)
    p = pos.numpy()
    assert ((p < 0) | (p >= L)).any(axis=1).mean() > 0.2                        # the wrap is exercised
    ref = orc.cell_index(p, N, L)
    bad = np.nonzero((ref != cells.numpy()).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], p[bad[:5]], ref[bad[:5]], cells.numpy()[bad[:5]])
    r, v = rho.numpy(), vel.numpy()
    assert set(np.unique(r)) <= {1.0, 2.0, 3.0} and set(np.unique(v)) <= set(float(i) for i in range(-3, 4))
    c = cells.numpy()
    if dist == "half_empty":
        assert c[:, 0].max() < N // 2
    if dist == "ends":
        first = (c[:, 0] == 0) & (c[:, 1] < 2) & (c[:, 2] < 16)
        last = (c[:, 0] == N - 1) & (c[:, 1] >= N - 2) & (c[:, 2] >= N - 16)
        assert (first | last).all() and first.any() and last.any()


@pytest.mark.parametrize("N", [48, 512])
def test_clump_and_ends_respect_the_cell_cap(N):
    """Under the default per-cell count no cell total passes CELL_SUM_CAP (N = 48: a background of 9 particles per cell)."""
    for dist, n in (("clump", 1_000_000), ("ends", chk.ends_count(10 ** 6))):
        cells, pos, rho, vel = chk.constructed_particles(CPU, n, N, 1.0, torch.float32, dist, seed=3)
        sums = chk.exact_slab_reference(cells, rho, vel, N, 0, N)
        assert max(int(s.abs().max()) for s in sums) <= chk.CELL_SUM_CAP
        if dist == "clump":
            cx0, cy0 = N // 3, (N // 48) * 16
            inside = (cells[:, 0] >= cx0) & (cells[:, 0] < cx0 + 2) & (cells[:, 1] >= cy0) & (cells[:, 1] < cy0 + 16)
            assert int(inside.sum()) >= min(int(0.3 * n), chk.CLUMP_PER_CELL * 32 * N)


def _moments_before_refactoring(dpos, dvel, drho, N, L, quantities, rows):
    """ngp_moments_float64 as it stood before ngp_fields_float64 was factored out of it (same operations, same order)."""
    Lcell = L / N
    vol = Lcell ** 3
    lc = torch.tensor(Lcell, dtype=dpos.dtype)
    cx = (torch.floor_divide(dpos[:, 0], lc) % N).to(torch.int64)
    out = {q: [[0.0, 0.0] for _ in range(1 if q == "energy" else 3)] for q in quantities}
    for x0 in range(0, N, rows):
        sel = torch.nonzero((cx >= x0) & (cx < x0 + rows)).squeeze(1)
        p = dpos[sel]
        flat = ((cx[sel] - x0) * N + (torch.floor_divide(p[:, 1], lc) % N).to(torch.int64)) * N \
            + (torch.floor_divide(p[:, 2], lc) % N).to(torch.int64)
        d = drho[sel].double()
        n3 = rows * N * N
        rho = torch.zeros(n3, dtype=torch.float64).index_add_(0, flat, d)
        inv = torch.where(rho > 0, 1.0 / rho, torch.zeros_like(rho))
        v = [torch.zeros(n3, dtype=torch.float64).index_add_(0, flat, d * dvel[sel, c].double()) * inv for c in range(3)]
        m = rho * vol
        for q in quantities:
            fs = v if q == "velocity" else [v[c] * m for c in range(3)] if q == "momentum" else \
                [m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])]
            for c, f in enumerate(fs):
                out[q][c][0] += float(f.sum().item())
                out[q][c][1] += float((f * f).sum().item())
    return out


def test_refactored_moments_are_unchanged():
    g = torch.Generator().manual_seed(5)
    N, L, n = 32, 2.5, 50_000
    pos = torch.rand((n, 3), generator=g, dtype=torch.float64) * 3 * L - L
    vel = torch.randn((n, 3), generator=g)
    rho = torch.exp(0.5 * torch.randn((n,), generator=g))
    qs = ("velocity", "momentum", "energy")
    for p in (pos, pos.float()):
        assert chk.ngp_moments_float64(p, vel, rho, N, L, qs, rows=8) == _moments_before_refactoring(p, vel, rho, N, L, qs, 8)


def test_abi_9_declares_the_deposit_plan():
    import os
    import re
    from vpower import _ffi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "vps_hip.h")).read()
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION >= 9
    assert int(re.search(r"#define VPS_DEPOSIT_PLAN_FIELDS (\d+)", hdr).group(1)) == len(_ffi.DEPOSIT_PLAN_FIELDS)
    lib = _ffi.lib()
    assert lib.vps_version() == _ffi.ABI_VERSION >= 9 and hasattr(lib, "vps_deposit_plan")     # the query exists from ABI 9 on
    assert lib.vps_deposit_plan(None, 1000, 4, 64, 0, 64, 0, -1, None) < 0      # no context: a status code, never a crash
