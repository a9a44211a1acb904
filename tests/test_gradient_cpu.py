"""The velocity-gradient fields (VPS_DIVERGENCE, VPS_VORTICITY, VPS_STRAIN_RATE) and the sub-grid flux without a GPU: the
references of tests/gradient_ref.py against closed forms and identities of the central-difference operator, the flux contraction
against an explicit double loop, and the agreement of header, wrapper and quantity.h on the codes."""
import os
import re

import numpy as np
import pytest

import gradient_ref as gr
import helmholtz_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_u(N, seed):
    return np.random.default_rng(seed).standard_normal((3, N, N, N))


@pytest.mark.parametrize("N,m", [(16, 1), (24, 5), (32, 3)])
def test_shear_wave_has_the_transfer_function_of_the_scheme(N, m):
    """u_x = sin(2 pi m y / L): d_y u_x = sin(2 pi m / N) / Lcell * cos(2 pi m y / L) -- sin(k Lcell) / Lcell for k = 2 pi m / L --
    the divergence is exactly 0 and S_xy = -omega_z / 2."""
    L = 3.0
    lc = L / N
    y = (np.arange(N) * lc)[None, :, None]
    u = np.zeros((3, N, N, N))
    u[0] = np.sin(2 * np.pi * m * y / L) * np.ones((N, 1, N))
    d = gr.derivatives64(u, lc)
    want = np.sin(2 * np.pi * m / N) / lc * np.cos(2 * np.pi * m * y / L) * np.ones((N, 1, N))
    assert np.abs(d[0][1] - want).max() <= 1e-12 * np.abs(want).max()
    assert not gr.fields64(u, lc, "divergence").any()
    w, S = gr.fields64(u, lc, "vorticity"), gr.fields64(u, lc, "strain_rate")
    assert np.array_equal(S[3], -0.5 * w[2]) and np.abs(S[3]).max() > 0
    assert not w[:2].any() and not S[:3].any() and not S[4:].any()


def test_trace_of_the_strain_is_the_divergence_and_the_antisymmetric_part_the_vorticity():
    N, lc = 12, 0.25
    u = _random_u(N, 1)
    d = gr.derivatives64(u, lc)
    div, w, S = gr.fields64(u, lc, "divergence")[0], gr.fields64(u, lc, "vorticity"), gr.fields64(u, lc, "strain_rate")
    assert np.array_equal((S[0] + S[1]) + S[2], div)
    # d_j u_i = S_ij - eps_ijk omega_k / 2
    assert np.allclose(S[3] - 0.5 * w[2], d[0][1], rtol=0, atol=1e-13 * np.abs(d[0][1]).max())
    assert np.allclose(S[4] + 0.5 * w[1], d[0][2], rtol=0, atol=1e-13 * np.abs(d[0][2]).max())
    assert np.allclose(S[5] - 0.5 * w[0], d[1][2], rtol=0, atol=1e-13 * np.abs(d[1][2]).max())


def test_curl_of_a_gradient_and_divergence_of_a_curl_vanish_for_the_difference_operator():
    """The generators of tests/helmholtz_ref.py make their fields with k' = the integer mode number, which is not the wavenumber
    sin(k Lcell) / Lcell of the difference scheme: their 'gradient' field has a (small) difference vorticity.  The pair of
    identities is exact for fields made by the difference operator itself, whose three axes commute: u = grad_FD phi and
    u = curl_FD A, with the generators' smooth random fields as the potentials."""
    N, lc = 16, 0.5
    pot = hr.spectral_fields(N, "gradient", seed=2)
    A = np.stack(hr.spectral_fields(N, "curl", seed=3))
    ug = gr.gradient64(pot[0], lc)
    uc = gr.fields64(A, lc, "vorticity")
    scale_g = np.abs(np.stack([x for row in gr.derivatives64(ug, lc) for x in row])).max()
    scale_c = np.abs(np.stack([x for row in gr.derivatives64(uc, lc) for x in row])).max()
    assert np.abs(gr.fields64(ug, lc, "vorticity")).max() <= 1e-12 * scale_g
    assert np.abs(gr.fields64(uc, lc, "divergence")).max() <= 1e-12 * scale_c
    assert np.abs(gr.fields64(ug, lc, "divergence")).max() > 1e-3 * scale_g        # (and neither field is trivial)
    assert np.abs(gr.fields64(uc, lc, "vorticity")).max() > 1e-3 * scale_c
    # the generators' own curl-free field under the difference operator: NOT zero (the reason for the construction above)
    sg = np.stack(pot)
    assert np.abs(gr.fields64(sg, lc, "vorticity")).max() > 1e-6 * np.abs(gr.fields64(sg, lc, "divergence")).max()


@pytest.mark.parametrize("what", list(gr.CODES))
def test_float32_mirror_is_exact_on_integers_and_close_on_floats(what):
    N = 10
    u = gr.integer_velocity(N, 5)
    for lc in (0.5, 2.0, 0.0625):
        assert np.array_equal(gr.fields32(u, lc, what).astype(np.float64), gr.fields64(u, lc, what))
    uf = _random_u(N, 6).astype(np.float32)
    lc = 0.3
    got, ref = gr.fields32(uf, lc, what), gr.fields64(uf, lc, what)
    assert got.shape == (gr.NCH[what], N, N, N)
    assert np.abs(got - ref).max() <= gr.error_bar(uf, lc)


@pytest.mark.parametrize("what", list(gr.CODES))
def test_impulse_table_is_the_reference_of_an_impulse(what):
    N, lc, A = 6, 0.25, 3.0
    for c in range(3):
        for p in ((0, 0, 0), (N - 1, N - 1, N - 1), (2, 4, 1)):
            u = np.zeros((3, N, N, N), dtype=np.float32)
            u[(c,) + p] = A
            ref = gr.fields32(u, lc, what)
            want = gr.impulse_expect(what, c, p, A, lc, N)
            assert len(want) == {"divergence": 2, "vorticity": 4, "strain_rate": 6}[what]
            assert {tuple(i): ref[tuple(i)] for i in np.argwhere(ref != 0)} == want
    assert gr.fields32_all(u, lc)[what].tobytes() == ref.tobytes()


def test_flux_contraction_against_the_explicit_double_loop():
    import torch
    from vpower import device
    rng = np.random.default_rng(7)
    tau6, S6 = rng.standard_normal((6, 5, 4, 3)), rng.standard_normal((6, 5, 4, 3))
    tau, S = gr.full_tensor(tau6), gr.full_tensor(S6)
    want = np.zeros((5, 4, 3))
    for i in range(3):
        for j in range(3):
            want -= tau[i][j] * S[i][j]
    ref, scale = gr.flux64(tau6, S6)
    assert np.allclose(ref, want, rtol=0, atol=1e-14 * scale.max())
    t64, s64 = torch.from_numpy(tau6), torch.from_numpy(S6)
    keep = t64.clone()
    got = device.flux_contraction(t64, s64).numpy()
    assert np.allclose(got, want, rtol=0, atol=1e-14 * scale.max()) and torch.equal(t64, keep)
    # float32: one rounding per product, five per sum (the factor 2 is exact): within 6 * 2^-24 of the sum of the absolute terms
    t32, s32 = t64.float(), s64.float()
    want32, scale32 = gr.flux64(t32.numpy(), s32.numpy())
    got32 = device.flux_contraction(t32, s32)
    assert got32.dtype == torch.float32 and np.all(np.abs(got32.numpy() - want32) <= 8 * 2.0 ** -24 * scale32)
    with pytest.raises(Exception, match="six fields"):
        device.flux_contraction(t64[:3], s64[:3])


def test_codes_in_header_wrapper_and_quantity_h():
    from vpower import _ffi, device
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    q = open(os.path.join(ROOT, "large-velocity-power-spectrum_amd", "csrc", "quantity.h")).read()
    for name, code in (("DIVERGENCE", 12), ("VORTICITY", 13), ("STRAIN_RATE", 14)):
        assert int(re.search(r"VPS_%s\s*=\s*(\d+)" % name, hdr).group(1)) == code == getattr(device, name) == gr.CODES[name.lower()]
        assert device.GRADIENT_QUANTITIES[name.lower()] == code and device.NCOMP[code] == gr.NCH[name.lower()]
        assert name.lower() not in device.QUANTITY and code not in device.QUANTITY.values()
        assert not device.needs_second_moment(code) and not device.is_tensor(code)
        assert "VPS_%s" % name in q
    assert "vps_quantity_gradient" in q and "sin(k Lcell) / Lcell" in hdr
    assert "gradient.hip" in _ffi.SOURCES
    assert os.path.exists(os.path.join(ROOT, "large-velocity-power-spectrum_amd", "csrc", "gradient.hip"))


def test_abi_13_and_81_declarations_hold():
    from vpower import _ffi
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == 13 == _ffi.ABI_VERSION
    body = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vps_[a-z0-9_]+)\s*\(", body))
    assert declared == {s[0] for s in _ffi.SYMBOLS} and len(declared) == 81


@pytest.mark.parametrize("name", ["divergence", "vorticity", "strain_rate", "subgrid_flux"])
def test_the_spectrum_routes_do_not_learn_the_names(name):
    from vpower import device
    with pytest.raises(Exception, match="Unrecognized physical quantity name"):
        device.resolve_quantity(name)
    with pytest.raises(Exception, match="Unrecognized physical quantity name"):
        device.resolve_quantity(name, supported=device.VECTOR_QUANTITIES)


def test_wrapper_refuses_bad_arguments_before_the_library():
    import torch
    from vpower import device
    ch = torch.zeros((4, 4, 4, 4))
    for what in ("velocity", "subgrid_stress", 0, 11, 15):
        with pytest.raises(ValueError, match="velocity_gradient forms"):
            device.HipKernels.velocity_gradient(object(), ch, 4, 1.0, what)
    with pytest.raises(ValueError, match="whole grid"):
        device.HipKernels.velocity_gradient(object(), ch[:, :2], 4, 1.0, "divergence")


def test_subgrid_flux_raises_by_name_on_fields_without_particles():
    from vpower import interp
    N = 8
    host = interp.BoxField(np.ones((N, N, N, 3)), np.ones((N, N, N)), 0.125)
    nn = interp.BoxField._from_neighbours((None, None, None), N, 0.125)
    for box, why in ((host, "four gridded channels"), (nn, "neighbour-backed")):
        with pytest.raises(Exception, match="subgrid_flux") as e:
            box.subgrid_flux()
        assert why in str(e.value) and "deposit_to_field" in str(e.value)
    assert nn._nn_src is not None and host._chans is None          # nothing was started
