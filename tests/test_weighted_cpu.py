"""CPU tests of the density-weighted velocity w = rho^alpha v: the float64 reference (tests/weighted_ref.py) is pinned to the
oracle and to Parseval, so that the GPU tests compare against something proven; and the host-side logic of the new quantity
names (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from oracle import vps_oracle as orc

import weighted_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _field_with_empty_cells(N=16, L=2.5, Np=6000, seed=5):
    pos, vel, dens = wref.particles(seed, Np, N, L)
    grid = wref.ngp_vec_grid(pos, vel, dens, N, L)
    assert 0.15 < np.mean(grid[..., 3] == 0) < 0.6, "the field must have empty cells"
    return grid


def test_alpha_zero_and_one_reproduce_the_oracle_velocity_and_momentum():
    N, L = 16, 2.5
    Lcell = L / N
    grid = _field_with_empty_cells(N, L)
    v, m = orc.vm_from_vec_grid(grid, Lcell, zero_empty=True)
    ref_v = orc.box_spctrm(v[..., 0], v[..., 1], v[..., 2], m, Lcell, "velocity")
    ref_p = orc.box_spctrm(v[..., 0], v[..., 1], v[..., 2], m, Lcell, "momentum")
    t0 = wref.table(wref.fields_from_vec_grid(grid, 0.0), L, N)
    t1 = wref.table(wref.fields_from_vec_grid(grid, 1.0), L, N)
    assert np.array_equal(t0[:, 3], ref_v[:, 3]) and np.array_equal(t1[:, 3], ref_p[:, 3])
    assert np.allclose(t0[:, 2], ref_v[:, 2], rtol=1e-12, atol=0)
    assert np.allclose(t1[:, 2], ref_p[:, 2] / Lcell ** 6, rtol=1e-12, atol=0)
    # ... and the gridded-field form (rho = mass / Lcell^3) is the same field
    for alpha in (0.0, 1.0, 1.0 / 3.0):
        a = wref.fields_from_vec_grid(grid, alpha)
        b = wref.fields_from_vm(v[..., 0], v[..., 1], v[..., 2], m, Lcell, alpha)
        for fa, fb in zip(a, b):
            assert np.allclose(fa, fb, rtol=1e-12, atol=0)


def test_parseval_for_alpha_one_half():
    """sum over ALL modes but k = 0 of P (2 pi / L)^3 = 1/2 (<rho |v|^2> - sum_c <w_c>^2): the alpha = 1/2 spectrum
    integrates to the kinetic energy density."""
    from oracle import gpu_checks as chk
    N, L = 16, 2.5
    grid = _field_with_empty_cells(N, L)
    w = wref.fields_from_vec_grid(grid, 0.5)
    kmin, kmax, kres = chk.all_mode_k_range(N, L)
    tab = wref.table(w, L, N, flavour="script", kmin=kmin, kmax=kmax, kres=kres)
    assert int(np.nansum(tab[:, 3])) == N ** 3 - 1
    v, _ = orc.vm_from_vec_grid(grid, 1.0, zero_empty=True)
    ekin = np.mean(grid[..., 3] * (v ** 2).sum(axis=-1))
    rhs = 0.5 * (ekin - sum(np.mean(c) ** 2 for c in w))
    assert np.isclose(np.sum(tab[:, 2]) * (2 * np.pi / L) ** 3, rhs, rtol=1e-12, atol=0)


@pytest.mark.parametrize("N,L,xrows,kzs", [(16, 2.5, 4, 3), (32, 1.0, 16, 8)])
def test_blockwise_reference_for_large_grids_equals_the_dense_one(N, L, xrows, kzs):
    """weighted_ref.sparse_grid_shell_sums (what the 2048^3 leg of the GPU tests compares against: occupied cells, float64
    transform and shell sums block by block) against the dense numpy reference of the same particles."""
    import torch
    from vpower import device
    from oracle_kernels import OracleKernels
    pos, vel, dens = wref.particles(N, 40 * N * N, N, L)
    pipe = device.PowerPipeline(N, L, kernels=OracleKernels(), comm=device.SlabComm(enabled=False))
    for alpha in (1.0 / 3.0, -0.5):
        ref = wref.table(wref.ngp_fields(pos, vel, dens, N, L, alpha), L, N)
        cells, vals = wref.sparse_cell_fields(pos, vel, dens, N, L, alpha)
        assert len(cells) < N ** 3
        ps, ns = wref.sparse_grid_shell_sums(torch.device("cpu"), cells, vals, N, L, pipe.k2, pipe.thr, xrows=xrows, kzs=kzs)
        assert np.array_equal(ns, ref[:, 3].astype(np.int64))
        assert np.allclose(ps, ref[:, 2], rtol=1e-11, atol=0)


def test_empty_cells_are_zero_for_every_alpha():
    vx = np.full((4, 4, 4), 3.0)
    mass = np.ones((4, 4, 4))
    mass[0, 0, 0] = 0.0
    for alpha in (0.0, 0.5, -0.5, 2.0):
        w = wref.fields_from_vm(vx, vx, vx, mass, 0.5, alpha)
        assert w[0][0, 0, 0] == 0.0 and np.isclose(w[0][1, 1, 1], 3.0 * 8.0 ** alpha)


def test_quantity_names_and_density_weight_rules():
    from vpower import device
    assert device.WEIGHTED == 4 and device.QUANTITY["weighted_velocity"] == 4 and device.NCOMP[device.WEIGHTED] == 3
    name, q = device.resolve_quantity("weighted_velocity", 0.25)
    assert name == "weighted_velocity" and int(q) == 4 == device.WEIGHTED and q.alpha == 0.25
    # as a key the exponent counts: a table or cache keyed by quantity keeps two exponents (and the bare code) apart
    W = device.WeightedVelocity
    assert W(0.5) == W(0.5) and W(0.5) != W(1.0 / 3.0) and W(0.5) != device.WEIGHTED and not (W(0.5) == 4)
    assert len({W(0.5), W(0.5), W(1.0 / 3.0), device.WEIGHTED}) == 3 and {W(0.5): "a"}.get(W(1.0 / 3.0)) is None
    assert device.NCOMP[int(W(0.5))] == 3
    assert device.resolve_quantity("rho13_velocity")[1].alpha == 1.0 / 3.0
    assert device.resolve_quantity("rho12_velocity")[1].alpha == 0.5
    assert device.resolve_quantity("momentum") == ("momentum", device.MOMENTUM)
    with pytest.raises(ValueError, match="needs density_weight"):
        device.resolve_quantity("weighted_velocity")
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            device.resolve_quantity("weighted_velocity", bad)
    for other in ("velocity", "momentum", "energy", "rho13_velocity"):
        with pytest.raises(ValueError, match="density_weight"):
            device.resolve_quantity(other, 0.5)
    with pytest.raises(Exception, match="Unrecognized physical quantity name") as e:
        device.resolve_quantity("vorticity")
    for n in ("weighted_velocity", "rho13_velocity", "rho12_velocity", "velocity", "momentum", "energy"):
        assert n in str(e.value)
    with pytest.raises(Exception, match="Unrecognized physical quantity name"):
        device.resolve_quantity("energy", supported=device.VECTOR_QUANTITIES)
    # dealt out by component like any vector quantity
    assert device.FieldComm.units(("rho13_velocity", "energy")) == [("rho13_velocity", 0), ("rho13_velocity", 1),
                                                                    ("rho13_velocity", 2), ("energy", None)]
    u = device.FieldComm.units((device.WeightedVelocity(0.5), device.WeightedVelocity(2.0)))
    assert [c for _, c in u] == [0, 1, 2, 0, 1, 2] and [q.alpha for q, _ in u] == [0.5] * 3 + [2.0] * 3
    assert u[0] != u[3] and u[0] == (device.WeightedVelocity(0.5), 0)


def test_boxfield_argument_errors_come_before_any_device_work():
    """The name / density_weight rules of BoxField.spctrm and helmholtz_spctrm need no GPU; a valid call without one raises
    VpsError (no CPU fallback)."""
    import torch
    from vpower import _ffi, interp
    N = 8
    box = interp.BoxField(np.ones((N, N, N, 3)), np.ones((N, N, N)), 0.125)
    for call in (box.spctrm, box.helmholtz_spctrm):
        with pytest.raises(ValueError, match="needs density_weight"):
            call("weighted_velocity")
        with pytest.raises(ValueError, match="density_weight"):
            call("velocity", density_weight=0.5)
        with pytest.raises(ValueError, match="finite"):
            call("weighted_velocity", density_weight=float("nan"))
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            call("rho14_velocity")
    if not torch.cuda.is_available():
        for call, kw in ((box.spctrm, dict(quantity="rho13_velocity")), (box.helmholtz_spctrm, dict(quantity="rho12_velocity")),
                         (box.spctrm, dict(quantity="weighted_velocity", density_weight=-0.5)),
                         (box.weighted_velocity_power, dict(alpha=0.5))):
            with pytest.raises(_ffi.VpsError):
                call(**kw)


def test_abi_8_declares_the_density_weight():
    from vpower import _ffi
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION >= 8
    assert re.search(r"int\s+vps_set_density_weight\s*\(\s*vps_ctx\s*\*\s*ctx\s*,\s*double\s+alpha\s*\)", hdr)
    assert re.search(r"VPS_WEIGHTED_VELOCITY\s*=\s*4", hdr)
    lib = _ffi.lib()
    assert lib.vps_version() == _ffi.ABI_VERSION >= 8 and hasattr(lib, "vps_set_density_weight")
    assert lib.vps_set_density_weight(None, 0.5) < 0          # no context: a status code, never a crash
