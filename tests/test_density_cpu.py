"""CPU tests of the scalar density quantities 'density' (s = rho^alpha) and 'log_density' (s = ln rho): the float64 reference
(tests/density_ref.py) is pinned to the definition and to known answers, so that the GPU tests compare against something
proven; the host-side logic of the new names; and the sanity of the GPU legs' inputs (no GPU needed)."""
import os
import re
import sys

import numpy as np
import pytest

from oracle import vps_oracle as orc

import density_ref as dref
import weighted_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSUM_RTOL = 2e-5      # the bar of tests/test_gpu_density.py


def _grid(N=16, L=2.5, Np=6000, seed=5, **kw):
    pos, vel, dens = wref.particles(seed, Np, N, L, **kw)
    return wref.ngp_vec_grid(pos, vel, dens, N, L)


def test_reference_fields_follow_the_definition():
    grid = _grid()
    rho = grid[..., 3]
    assert 0.15 < np.mean(rho == 0) < 0.6, "the field must have empty cells"
    assert np.array_equal(dref.density_field(grid, 1.0), rho) and np.array_equal(dref.density_field(rho), rho)
    occ = rho != 0
    s = dref.log_density_field(grid)
    assert np.array_equal(s[occ], np.log(rho[occ])) and not s[~occ].any()
    for alpha in (0.5, -0.5, 0.0, 2.0):
        f = dref.density_field(grid, alpha)
        assert np.allclose(f[occ], rho[occ] ** alpha, rtol=1e-14, atol=0) and not f[~occ].any()     # 0 in empty cells, alpha = 0 too
    assert np.array_equal(dref.field(grid, "log"), s) and np.array_equal(dref.field(grid, 0.5), dref.density_field(grid, 0.5))


def test_table_of_a_constant_plus_one_mode():
    """s = c + A cos(2 pi m.x / L): the two modes +-m hold 0.5 (a A N^3 / 2)^2 each, a = (L / 2 pi)^1.5 / N^3; the constant
    sits in k = 0, which no shell holds."""
    N, L, A, c, m = 16, 2.5, 0.75, 3.0, (2, 1, 0)
    x = np.arange(N) / N
    ph = 2 * np.pi * (m[0] * x[:, None, None] + m[1] * x[None, :, None] + m[2] * x[None, None, :])
    tab = dref.table(c + A * np.cos(ph), L, N)
    kmode = 2 * np.pi / L * np.sqrt(sum(i * i for i in m))
    width = tab[1, 0] - tab[0, 0]
    hit = int(np.argmin(np.abs(tab[:, 0] - kmode)))
    assert abs(tab[hit, 0] - kmode) <= 0.5 * width * (1 + 1e-9)
    expect = (L / (2 * np.pi)) ** 3 * A * A / 4
    assert np.isclose(tab[hit, 2], expect, rtol=1e-12, atol=0)
    others = np.delete(tab[:, 2], hit)
    assert np.all(np.abs(others) < 1e-20 * expect + 1e-25)
    assert tab[:, 3].sum() < N ** 3          # k = 0 (at least) is in no shell


def test_log_density_table_ignores_the_density_unit_when_no_cell_is_empty():
    """ln(10 rho) = ln rho + ln 10 moves the k = 0 mode only: every shell sum is unchanged to 1e-12."""
    N, L = 16, 2.5
    grid = _grid(N, L, Np=40 * N ** 3 // 4, empty_fraction=0.0)
    rho = grid[..., 3]
    assert np.all(rho > 0)
    # (densities in units of their geometric mean: the rounding of the float64 transform itself grows with the mean of ln rho
    #  against its scatter, and at a mean of 8 it is 1.6e-12 of the shell sums -- the test is of the reference, not of numpy)
    rho = rho / np.exp(np.mean(np.log(rho)))
    t1 = dref.table(dref.log_density_field(rho), L, N)
    t10 = dref.table(dref.log_density_field(10.0 * rho), L, N)
    assert np.array_equal(t1[:, 3], t10[:, 3]) and np.allclose(t1[:, 2], t10[:, 2], rtol=1e-12, atol=0)
    # ... and does NOT when cells are empty (they count as rho = 1): the documented caveat
    g2 = _grid(N, L)
    a, b = dref.table(dref.log_density_field(g2), L, N), dref.table(dref.log_density_field(10.0 * g2[..., 3]), L, N)
    assert not np.allclose(a[:, 2], b[:, 2], rtol=1e-3, atol=0)


def test_quantity_names_density_class_and_units():
    from vpower import device
    D = device.Density
    assert (device.DENSITY, device.LOG_DENSITY) == (5, 6) and device.QUANTITY["density"] == 5 and device.QUANTITY["log_density"] == 6
    assert device.NCOMP[device.DENSITY] == 1 and device.NCOMP[device.LOG_DENSITY] == 1 and device.NCOMP[int(D(0.5))] == 1
    name, q = device.resolve_quantity("density")
    assert name == "density" and isinstance(q, D) and int(q) == 5 and q.alpha == 1.0
    name, q = device.resolve_quantity("density", -0.5)
    assert name == "density" and q == D(-0.5) and q.alpha == -0.5
    assert device.resolve_quantity("log_density") == ("log_density", device.LOG_DENSITY)
    # equality and hash by exponent; never equal to the bare code or to a weighted velocity of the same exponent
    assert D(0.5) == D(0.5) and D(0.5) != D(1.0) and D(1.0) == D() and D(0.5) != device.DENSITY and not (D(0.5) == 5)
    assert D(0.5) != device.WeightedVelocity(0.5) and device.WeightedVelocity(0.5) != D(0.5)
    assert len({D(0.5), D(0.5), D(1.0), device.DENSITY, device.WeightedVelocity(0.5)}) == 4 and {D(0.5): 1}.get(D(1.0)) is None
    assert "0.5" in repr(D(0.5))
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            device.resolve_quantity("density", bad)
    with pytest.raises(ValueError, match="density_weight"):
        device.resolve_quantity("log_density", 0.5)
    for other in ("velocity", "momentum", "energy", "rho13_velocity"):
        with pytest.raises(ValueError, match="density_weight"):
            device.resolve_quantity(other, 0.5)
    with pytest.raises(Exception, match="Unrecognized physical quantity name") as e:
        device.resolve_quantity("vorticity")
    assert "'density'" in str(e.value) and "'log_density'" in str(e.value) and "'energy'" in str(e.value)
    for scalar in ("density", "log_density", "energy"):
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            device.resolve_quantity(scalar, supported=device.VECTOR_QUANTITIES)
    # a scalar quantity is dealt out as ONE unit, by name or by code
    assert device.FieldComm.units(("density", "velocity", "log_density")) == \
        [("density", None), ("velocity", 0), ("velocity", 1), ("velocity", 2), ("log_density", None)]
    u = device.FieldComm.units((D(0.5), device.LOG_DENSITY, device.ENERGY, device.WeightedVelocity(0.5)))
    assert [c for _, c in u] == [None, None, None, 0, 1, 2] and u[0] == (D(0.5), None) and u[0] != (D(1.0), None)
    with pytest.raises(Exception, match="component"):
        device.HipKernels._component_mask(device.DENSITY, 0)


def test_boxfield_argument_errors_come_before_any_device_work():
    import torch
    from vpower import _ffi, interp
    N = 8
    box = interp.BoxField(np.ones((N, N, N, 3)), np.ones((N, N, N)), 0.125)
    with pytest.raises(ValueError, match="density_weight"):
        box.spctrm("log_density", density_weight=0.5)
    with pytest.raises(ValueError, match="finite"):
        box.spctrm("density", density_weight=float("nan"))
    for name in ("density", "log_density"):
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            box.helmholtz_spctrm(name)
    if not torch.cuda.is_available():        # a valid call without a GPU raises VpsError: no CPU fallback
        for call, kw in ((box.spctrm, dict(quantity="density")), (box.spctrm, dict(quantity="log_density")),
                         (box.spctrm, dict(quantity="density", density_weight=0.5)), (box.density_power, dict(alpha=0.5)),
                         (box.log_density_power, {})):
            with pytest.raises(_ffi.VpsError):
                call(**kw)


def test_cli_parser_and_quantity_resolution():
    sys.path.insert(0, os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts"))
    try:
        import parallel_optimized as po
    finally:
        sys.path.pop(0)
    from vpower import device
    p = po.build_parser()
    a = p.parse_args([])
    assert a.quantity == "velocity" and a.density_weight is None and po.resolve_cli_quantity(a) == ("velocity", device.VELOCITY)
    a = p.parse_args(["--quantity", "density", "--density-weight", "0.5"])
    assert po.resolve_cli_quantity(a) == ("density", device.Density(0.5))
    assert po.resolve_cli_quantity(p.parse_args(["--quantity", "log_density"])) == ("log_density", device.LOG_DENSITY)
    assert po.resolve_cli_quantity(p.parse_args(["--quantity", "rho13_velocity", "--helmholtz"]))[0] == "weighted_velocity"
    with pytest.raises(ValueError, match="density_weight"):
        po.resolve_cli_quantity(p.parse_args(["--quantity", "log_density", "--density-weight", "2"]))
    for scalar in ("density", "log_density", "energy"):
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            po.resolve_cli_quantity(p.parse_args(["--quantity", scalar, "--helmholtz"]))


def test_abi_11_declares_the_density_codes():
    from vpower import _ffi
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION >= 11
    assert re.search(r"VPS_DENSITY\s*=\s*5", hdr) and re.search(r"VPS_LOG_DENSITY\s*=\s*6", hdr)
    assert _ffi.lib().vps_version() == _ffi.ABI_VERSION >= 11


@pytest.mark.parametrize("which", [1.0, 0.5, -0.5, "log"])
def test_gpu_leg_inputs_survive_float32_rounding_of_the_field(which):
    """The inputs of the fused N = 64 leg of tests/test_gpu_density.py (eight-decade densities, empty cells, one over-full
    pencil): the float64 table of the reference field ROUNDED to float32 stays within a quarter of the bar (PSUM_RTOL / 4) of
    the unrounded one per live shell -- the bar measures the kernels, not what a float32 field can hold.  (It does, with the
    full eight decades: no leg had to narrow its density range.)"""
    N, L = 64, 1.0
    pos, vel, dens = dref.fused_inputs(N, 300_000, L)
    f = dref.field(wref.ngp_vec_grid(pos, vel, dens, N, L), which)
    ref = dref.table(f, L, N)
    got = dref.table(f.astype(np.float32).astype(np.float64), L, N)
    live = ref[:, 3] > 0
    dev = float(np.max(np.abs(got[live, 2] - ref[live, 2]) / ref[live, 2]))
    print("float32-rounded reference field %r: worst per-shell deviation %.3e (bar / 4 = %.1e)" % (which, dev, PSUM_RTOL / 4))
    assert np.array_equal(got[:, 3], ref[:, 3]) and dev < PSUM_RTOL / 4
