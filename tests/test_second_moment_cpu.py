"""The second-moment quantities without a GPU: the float64 reference's own identities, the codes in the header, the wrapper and
the library, the ABI that stays 13, the driver's parser, and the BoxFields that cannot form them."""
import os
import re
import sys

import numpy as np
import pytest

import second_moment_ref as smr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _particles(n=30000, N=16, L=2.0, seed=0):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) * L).astype(np.float32)
    pos[: n // 3] = (pos[: n // 3] * 0.05 + 0.3).astype(np.float32)          # a clump: many particles per cell
    vel = (rng.standard_normal((n, 3)) + np.array([5.0, -3.0, 1.0])).astype(np.float32)
    rho = np.exp(0.5 * rng.standard_normal(n)).astype(np.float32)
    return pos, vel, rho, N, L


@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
def test_reference_identities(assignment):
    """energy + subgrid = total cell by cell, sigma^2 >= 0, everything 0 in empty cells, the total conserved: the sum of
    total_energy over the cells is vol sum_p rho |v|^2 (the weights of a particle sum to 1), and a slab is the rows of the grid."""
    pos, vel, rho, N, L = _particles()
    m = smr.moments(pos, vel, rho, N, L, assignment)
    lc = L / N
    tot, sub, disp, en = (smr.quantity(m, lc, "total_energy"), smr.quantity(m, lc, "subgrid_energy"), smr.quantity(m, lc, "dispersion"),
                          smr.resolved_energy(m, lc))
    assert np.allclose(en + sub, tot, rtol=1e-12, atol=0)
    assert sub.min() >= 0 and disp.min() >= 0 and sub.max() > 0
    empty = m["n"] == 0
    assert not tot[empty].any() and not sub[empty].any() and not disp[empty].any()
    want = lc ** 3 * np.sum(rho.astype(np.float64) * (vel.astype(np.float64) ** 2).sum(axis=1))
    assert abs(tot.sum() - want) <= 1e-6 * want          # (float32 weight words: a particle's weights sum to 1 to 2^-24 each)
    if assignment == "ngp":
        assert abs(tot.sum() - want) <= 1e-13 * want
        one = m["n"] == 1
        assert one.any() and np.all(sub[one] <= 1e-12 * tot[one])
    ms = smr.moments(pos, vel, rho, N, L, assignment, 3, 6)
    for k in ("S2", "R", "n"):
        assert np.array_equal(ms[k], m[k][3:9])
    assert np.array_equal(ms["P"], m["P"][:, 3:9])


def test_reference_agrees_with_the_oracle_grid():
    """P and R of the reference are the oracle's NGP grid of [rho v, rho]; for CIC they agree with it to the float32 weights."""
    from oracle import vps_oracle as orc
    pos, vel, rho, N, L = _particles(8000)
    vec = orc.density_velocity_vector(vel.astype(np.float64), rho.astype(np.float64))
    m = smr.moments(pos, vel, rho, N, L)
    g = orc.deposit_to_grid(vec, pos, N, L)
    assert np.allclose(np.moveaxis(g[..., :3], -1, 0), m["P"], rtol=1e-12, atol=1e-12) and np.allclose(g[..., 3], m["R"], rtol=1e-12)
    mc = smr.moments(pos, vel, rho, N, L, "cic")
    gc = orc.deposit_assign(vec, pos, N, L, "cic")
    assert np.allclose(gc[..., 3], mc["R"], rtol=1e-5, atol=1e-6 * gc[..., 3].max())
    t = smr.table(smr.quantity(m, L / N, "subgrid_energy"), L, N)
    assert t.shape[1] == 4 and t[:, 3].sum() > 0 and np.all(t[:, 2] >= 0)


def test_codes_in_header_wrapper_and_library():
    from vpower import _ffi, device
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    for name, code in (("TOTAL_ENERGY", 7), ("SUBGRID_ENERGY", 8), ("DISPERSION", 9)):
        assert int(re.search(r"VPS_%s\s*=\s*(\d+)" % name, hdr).group(1)) == code == getattr(device, name)
        assert device.QUANTITY[name.lower()] == code and device.resolve_quantity(name.lower()) == (name.lower(), code)
        # vps_quantity_channels through the wrapper's output shape rule: one field
        assert device.NCOMP[code] == 1 and name.lower() in device.SCALAR_QUANTITIES
        assert device.needs_second_moment(code) and device.needs_second_moment(name.lower())
        with pytest.raises(ValueError, match="density_weight"):
            device.resolve_quantity(name.lower(), 0.5)
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            device.resolve_quantity(name.lower(), supported=device.VECTOR_QUANTITIES)
        with pytest.raises(Exception, match="component"):
            device.HipKernels._component_mask(code, 0)
    assert not device.needs_second_moment(device.ENERGY) and not device.needs_second_moment("energy")
    assert device.FieldComm.units(("subgrid_energy", device.DISPERSION)) == [("subgrid_energy", None), (device.DISPERSION, None)]
    q = open(os.path.join(ROOT, "large-velocity-power-spectrum_amd", "csrc", "quantity.h")).read()
    assert "vps_quantity_second_moment" in q
    # an addition within ABI 13: no new symbol, no bump
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == 13 == _ffi.ABI_VERSION
    assert _ffi.lib().vps_version() == 13


def test_driver_parser_accepts_and_refuses():
    sys.path.insert(0, os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts"))
    try:
        import parallel_optimized as po
    finally:
        sys.path.pop(0)
    from vpower import device
    p = po.build_parser()
    for name in ("total_energy", "subgrid_energy", "dispersion"):
        for g in ("ngp", "cic", "tsc"):
            a = po.check_gridding(p, p.parse_args(["--quantity", name, "--gridding", g]))
            assert po.resolve_cli_quantity(a) == (name, device.QUANTITY[name])
        a = po.check_gridding(p, p.parse_args(["--quantity", name, "--gridding", "cic", "--deconvolve"]))
        assert a.deconvolve
        for argv in (["--quantity", name], ["--quantity", name, "--gridding", "nn"]):
            with pytest.raises(SystemExit):
                po.check_gridding(p, p.parse_args(argv))
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            po.resolve_cli_quantity(p.parse_args(["--quantity", name, "--gridding", "ngp", "--helmholtz"]))
        with pytest.raises(ValueError, match="density_weight"):
            po.resolve_cli_quantity(p.parse_args(["--quantity", name, "--gridding", "ngp", "--density-weight", "2"]))
    assert tuple(po.SECOND_MOMENT) == tuple(device.SECOND_MOMENT_QUANTITIES)
    # the other quantities keep their nearest-neighbour default
    assert po.check_gridding(p, p.parse_args(["--quantity", "energy"])).gridding == "nn"


def test_fields_without_particles_raise_by_name_before_any_device_work():
    from vpower import interp
    N = 8
    host = interp.BoxField(np.ones((N, N, N, 3)), np.ones((N, N, N)), 0.125)
    nn = interp.BoxField._from_neighbours((None, None, None), N, 0.125)
    for name in ("total_energy", "subgrid_energy", "dispersion"):
        for box, why in ((host, "four gridded channels"), (nn, "neighbour-backed")):
            with pytest.raises(Exception, match=name) as e:
                box.spctrm(name)
            assert why in str(e.value) and "deposit_to_field" in str(e.value)
            with pytest.raises(Exception, match=name):
                getattr(box, name)()
            with pytest.raises(Exception, match="Unrecognized physical quantity name"):
                box.helmholtz_spctrm(name)
        with pytest.raises(ValueError, match="density_weight"):
            host.spctrm(name, density_weight=0.5)
    assert nn._nn_src is not None and nn._nn_spectra == 0 and host._chans is None          # nothing was started
