"""The tensor quantities (VPS_SUBGRID_STRESS, VPS_DISPERSION_TENSOR) without a GPU: the float64 reference of tests/stress_ref.py
against the scalar reference it must contract to, the conservation of the diagonal, and the agreement of header, wrapper and
driver on codes and names."""
import os
import re
import sys

import numpy as np
import pytest

import second_moment_ref as smr
import stress_ref as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _particles(n=20000, N=16, L=2.0, seed=3):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3)) * L).astype(np.float32)
    vel = (rng.standard_normal((n, 3)) + np.array([3.0, -1.0, 0.5])).astype(np.float32)
    rho = np.exp(0.4 * rng.standard_normal(n)).astype(np.float32)
    return pos, vel, rho, N, L


@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
def test_trace_is_the_scalar_reference(assignment):
    pos, vel, rho, N, L = _particles()
    m = st.moments(pos, vel, rho, N, L, assignment)
    ms = smr.moments(pos, vel, rho, N, L, assignment)
    assert np.array_equal(m["n"], ms["n"]) and np.allclose(m["R"], ms["R"], rtol=1e-14)
    assert np.allclose(st.trace(m["S"]), ms["S2"], rtol=1e-12)
    assert np.allclose(m["A"], m["S"][:3], rtol=1e-14)                 # positive densities: the diagonal terms are absolute
    for q, scalar in st.SCALAR_OF.items():
        f = st.fields(m, L / N, q)
        ref = smr.quantity(ms, L / N, scalar)
        assert f.shape == (6, N, N, N) and f[:3].min() >= 0 and f[3:].min() < 0
        assert np.allclose(st.trace(f), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        assert not f[:, m["R"] == 0].any()
    if assignment == "ngp":
        f = st.fields(m, L / N, "subgrid_stress")
        assert np.abs(f[:, m["n"] == 1]).max() <= 1e-12 * np.abs(f).max()


@pytest.mark.parametrize("assignment", ["ngp", "cic", "tsc"])
def test_diagonal_plus_resolved_sums_to_the_particles(assignment):
    """sum over the cells of vol S_ii (= the unclamped sub-grid diagonal plus the resolved part vol P_i^2 / R) is
    vol sum_p rho_p v_i^2: the weights of a particle sum to 1."""
    pos, vel, rho, N, L = _particles(seed=4)
    m = st.moments(pos, vel, rho, N, L, assignment)
    vol = (L / N) ** 3
    has = m["R"] != 0
    Rs = np.where(has, m["R"], 1.0)
    for i in range(3):
        resolved = np.where(has, vol * m["P"][i] ** 2 / Rs, 0.0)
        sub = vol * m["S"][i] - resolved
        want = vol * np.sum(rho.astype(np.float64) * vel[:, i].astype(np.float64) ** 2)
        # (CIC / TSC: the reference takes the kernel's weights, each axis weight rounded once to float32, so a particle's weights
        #  sum to 1 within three float32 roundings; NGP: float64 summation only)
        assert abs(np.sum(sub + resolved) - want) <= (1e-12 if assignment == "ngp" else 4 * 2.0 ** -24) * want
        assert sub.min() >= -1e-12 * np.abs(resolved).max()           # Cauchy-Schwarz: the clamp only removes rounding


def test_contraction_table_counts_the_off_diagonals_twice():
    pos, vel, rho, N, L = _particles(n=5000)
    f = st.fields(st.moments(pos, vel, rho, N, L), L / N, "subgrid_stress")
    t = st.table(f, L, N)
    one = [smr.table(f[c], L, N) for c in range(6)]
    want = sum(o[:, 2] for o in one[:3]) + 2 * sum(o[:, 2] for o in one[3:])
    assert np.array_equal(t[:, 3], one[0][:, 3]) and np.allclose(t[:, 2], want, rtol=1e-14)


def test_codes_in_header_wrapper_and_library():
    from vpower import _ffi, device
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    for name, code in (("SUBGRID_STRESS", 10), ("DISPERSION_TENSOR", 11)):
        assert int(re.search(r"VPS_%s\s*=\s*(\d+)" % name, hdr).group(1)) == code == getattr(device, name)
        assert device.QUANTITY[name.lower()] == code and device.resolve_quantity(name.lower()) == (name.lower(), code)
        assert device.NCOMP[code] == 6 and name.lower() not in device.SCALAR_QUANTITIES
        assert device.needs_second_moment(code) and device.needs_second_moment(name.lower())
        assert device.is_tensor(code) and device.is_tensor(name.lower())
        with pytest.raises(ValueError, match="density_weight.*%s" % name.lower()):
            device.resolve_quantity(name.lower(), 0.5)
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            device.resolve_quantity(name.lower(), supported=device.VECTOR_QUANTITIES)
    assert not device.is_tensor(device.DISPERSION) and not device.is_tensor("dispersion")
    q = open(os.path.join(ROOT, "large-velocity-power-spectrum_amd", "csrc", "quantity.h")).read()
    assert "vps_quantity_tensor" in q
    # an addition within ABI 13: no new symbol, no bump
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == 13 == _ffi.ABI_VERSION


def test_driver_parser_accepts_and_refuses():
    sys.path.insert(0, os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts"))
    try:
        import parallel_optimized as po
    finally:
        sys.path.pop(0)
    from vpower import device
    p = po.build_parser()
    for name in st.QUANTITIES:
        for g in ("ngp", "cic", "tsc"):
            a = po.check_gridding(p, p.parse_args(["--quantity", name, "--gridding", g]))
            assert po.resolve_cli_quantity(a) == (name, device.QUANTITY[name])
        for argv in (["--quantity", name], ["--quantity", name, "--gridding", "nn"]):
            with pytest.raises(SystemExit):
                po.check_gridding(p, p.parse_args(argv))
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            po.resolve_cli_quantity(p.parse_args(["--quantity", name, "--gridding", "ngp", "--helmholtz"]))


def test_driver_refuses_the_helmholtz_decomposition_of_a_tensor():
    sys.path.insert(0, os.path.join(ROOT, "large-velocity-power-spectrum_amd", "scripts"))
    try:
        import parallel_optimized as po
    finally:
        sys.path.pop(0)
    from vpower import device
    z = np.zeros((4, 3), dtype=np.float32)
    for name in st.QUANTITIES:
        with pytest.raises(ValueError, match="quantity %d" % device.QUANTITY[name]):
            po.velocity_spectrum(z, z[:, 0], z, 16, 1.0, helmholtz=True, quantity=device.QUANTITY[name], density=z[:, 0] + 1,
                                 gridding="cic", kernels=object())


def test_contraction_fields_leaves_the_callers_fields_alone():
    import torch
    from vpower import device
    f = [torch.full((2, 2, 2), float(c + 1)) for c in range(6)]
    keep = [x.clone() for x in f]
    for _ in range(2):
        out = device.contraction_fields(f, device.SUBGRID_STRESS)
        assert all(torch.equal(a, b) for a, b in zip(f, keep))
        assert all(o is x for o, x in zip(out[:3], f[:3]))
        for c in range(3, 6):
            assert torch.equal(out[c], keep[c] * float(np.float32(np.sqrt(2.0))))
    assert device.contraction_fields(f[:3], device.VELOCITY) == f[:3]
    with pytest.raises(Exception, match="six fields"):
        device.contraction_fields(f[:3], "subgrid_stress")


def test_fields_without_particles_raise_by_name_before_any_device_work():
    from vpower import interp
    N = 8
    host = interp.BoxField(np.ones((N, N, N, 3)), np.ones((N, N, N)), 0.125)
    nn = interp.BoxField._from_neighbours((None, None, None), N, 0.125)
    for name in st.QUANTITIES:
        for box, why in ((host, "four gridded channels"), (nn, "neighbour-backed")):
            for call in (lambda: box.spctrm(name), lambda: box.correlation(name), lambda: box.structure_function(name),
                         lambda: getattr(box, name)()):
                with pytest.raises(Exception, match=name) as e:
                    call()
                assert why in str(e.value) and "deposit_to_field" in str(e.value)
            with pytest.raises(Exception, match="Unrecognized physical quantity name.*%s" % name):
                box.helmholtz_spctrm(name)
    assert nn._nn_src is not None and nn._nn_spectra == 0 and host._chans is None          # nothing was started
