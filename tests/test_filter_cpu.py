"""The box-filter codes (VPS_FILTERED_VM, VPS_FILTERED_STRESS) without a GPU: the references of tests/filter_ref.py against
closed forms, the law of total variance that ties the sub-filter stress to the sub-grid stress of a coarser deposit, the agreement
of header, wrapper and quantity.h on the codes, and the refusals of the wrapper."""
import os
import re

import numpy as np
import pytest

import filter_ref as fr
import stress_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_chans(N, seed):
    rng = np.random.default_rng(seed)
    ch = rng.standard_normal((4, N, N, N))
    ch[3] = rng.random((N, N, N)) + 0.25
    return ch.astype(np.float32)


@pytest.mark.parametrize("m", [1, 2, 3])
def test_box_sum_is_the_sum_over_rolls(m):
    a = np.random.default_rng(m).integers(-5, 6, (8, 10, 12)).astype(np.float64)
    want = np.zeros_like(a)
    for dx in range(-m, m + 1):
        for dy in range(-m, m + 1):
            for dz in range(-m, m + 1):
                want += np.roll(a, (dx, dy, dz), axis=(0, 1, 2))
    assert np.array_equal(fr.box_sum(a, m), want)
    assert np.array_equal(fr.box_sum(np.stack([a, 2 * a]), m), np.stack([want, 2 * want]))


@pytest.mark.parametrize("N,m", [(8, 1), (12, 3), (6, 2)])
def test_constant_velocity_is_kept_and_has_no_stress(N, m):
    """Integer masses and a dyadic velocity: every sum is exact, u~ = u and tau = 0 bit for bit in the float32 mirror."""
    ch = fr.integer_chans(N, 1, holes=False)
    ch[3] += 1
    ch[0], ch[1], ch[2] = 1.5, -2.0, 0.25
    vm, tau = fr.fields32(ch, m, "vm"), fr.fields32(ch, m, "stress")
    for a in range(3):
        assert np.all(vm[a] == ch[a])
    assert not tau.any()
    assert np.array_equal(vm[3], (fr.box_sum(ch[3].astype(np.float64), m).astype(np.float32) * np.float32(1.0 / (2 * m + 1) ** 3)))


@pytest.mark.parametrize("m", [1, 2, 4])
def test_at_n_equal_2m_plus_2_a_box_is_the_grid_minus_one_plane_per_axis(m):
    N = 2 * m + 2
    ms = np.random.default_rng(m).integers(0, 3, (N, N, N)).astype(np.float64)
    M = fr.box_sum(ms, m)
    tot = ms.sum()
    for i in ((0, 0, 0), (1, N - 1, m), (m + 1, m, 0)):
        out = [(i[a] + m + 1) % N for a in range(3)]                       # the plane each axis leaves out
        keep = np.ones((N, N, N), dtype=bool)
        keep[out[0]] = False
        keep[:, out[1]] = False
        keep[:, :, out[2]] = False
        assert M[i] == ms[keep].sum()
    assert M.sum() == (2 * m + 1) ** 3 * tot


@pytest.mark.parametrize("N,m", [(8, 1), (10, 3), (16, 2)])
def test_sum_of_box_sums_and_sign_of_the_diagonals(N, m):
    ch = _random_chans(N, N + m)
    s, a = fr.sums64(ch, m)
    assert np.isclose(s[0].sum(), (2 * m + 1) ** 3 * ch[3].astype(np.float64).sum(), rtol=1e-12)
    tau64, tau32 = fr.fields64(ch, m, "stress"), fr.fields32(fr.integer_chans(N, 3), m, "stress")
    assert np.all(tau64[:3] >= 0) and np.all(tau32[:3] >= 0) and (tau64[3:] < 0).any()
    assert np.all(a >= np.abs(s)) and np.all(fr.bars(ch, m, "stress") > 0) and np.all(fr.bars(ch, m, "vm") > 0)
    # Cauchy-Schwarz: the unclamped diagonal is >= 0 in exact arithmetic, so the clamp only removes rounding
    Ms = s[0]
    for k in range(3):
        assert np.all(s[4 + k] - s[1 + k] ** 2 / Ms >= -1e-12 * a[4 + k])


def test_float32_mirror_is_exact_and_the_empty_boxes_are_zero():
    N, m = 24, 2
    ch = fr.integer_chans(N, 7)
    for what in ("vm", "stress"):
        got, ref = fr.fields32(ch, m, what), fr.fields64(ch, m, what)
        assert got.dtype == np.float32 and got.shape == (fr.NCH[what], N, N, N)
        # (exact sums: the float32 mirror differs from the float64 form by the roundings behind the sums alone, K = 0)
        assert np.all(np.abs(got - ref) <= fr.bars(ch, m, what, extra=-fr.chain(m)))
        assert np.array_equal(got, fr.fields32_all(ch, m)[what])
        empty = fr.box_sum(ch[3].astype(np.float64), m) == 0
        assert empty.any() and not got[:, empty].any()


def test_law_of_total_variance_ties_the_sub_filter_stress_to_the_coarser_deposit():
    """Two particles at every fine-cell centre of a 12^3 grid, w = 3: the second-moment stress of the coarse 4^3 deposit is
    w^3 sum_W tau_fine + w^6 tau_l at the box centres (m = 1) -- the dispersion inside the fine cells plus the stress of the fine
    grid's cell means -- with tau_fine, tau_coarse from tests/stress_ref.py and tau_l from the fine [u, mass] grid, in float64."""
    Nf, w, L = 12, 3, 2.0
    Nc, lf = Nf // w, L / Nf
    g = (np.arange(Nf) + 0.5) * lf
    centres = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = np.concatenate([centres, centres])
    rng = np.random.default_rng(3)
    vel = rng.standard_normal(pos.shape) + np.array([1.0, -0.5, 0.25])
    rho = rng.random(len(pos)) + 0.5
    mf, mc = sref.moments(pos, vel, rho, Nf, L), sref.moments(pos, vel, rho, Nc, L)
    tau_f, tau_c = sref.fields(mf, lf, "subgrid_stress"), sref.fields(mc, L / Nc, "subgrid_stress")
    assert np.abs(tau_f).min() > 0                                          # two particles per cell: a dispersion everywhere
    chans = np.concatenate([mf["P"] / mf["R"], (mf["R"] * lf ** 3)[None]])
    t = fr.terms(chans)
    s = fr.box_sum(t, 1)
    tau_l = np.stack([(s[4 + k] - s[1 + i] * s[1 + j] / s[0]) / w ** 3 for k, (i, j) in enumerate(fr.IJ)])
    centre = (slice(None), slice(1, None, w), slice(1, None, w), slice(1, None, w))
    rebuilt = w ** 3 * fr.box_sum(tau_f, 1)[centre] + w ** 6 * tau_l[centre]
    assert rebuilt.shape == tau_c.shape == (6, Nc, Nc, Nc)
    assert np.abs(rebuilt - tau_c).max() <= 1e-12 * np.abs(tau_c).max()
    assert np.abs(w ** 6 * tau_l[centre]).max() > 0.1 * np.abs(tau_c).max()   # (neither part is negligible)


def test_impulse_table_is_the_reference_of_an_impulse():
    N = 8
    for m in (1, 3):
        for p in ((0, 0, 0), (N - 1, 0, N - 1), (3, 4, 0)):
            ch = np.zeros((4, N, N, N), dtype=np.float32)
            ch[:3, p[0], p[1], p[2]] = (1, 2, 3)
            ch[(3,) + p] = 1
            mask = fr.impulse_expect(p, m, N)
            assert mask.sum() == (2 * m + 1) ** 3
            vm = fr.fields32(ch, m, "vm")
            for a in range(3):
                assert np.array_equal(vm[a], np.where(mask, np.float32(a + 1), np.float32(0)))
            assert np.array_equal(vm[3], np.where(mask, np.float32(1.0 / (2 * m + 1) ** 3), np.float32(0)))
            assert not fr.fields32(ch, m, "stress").any()


def test_codes_in_header_wrapper_and_quantity_h():
    from vpower import _ffi, device
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    q = open(os.path.join(ROOT, "large-velocity-power-spectrum_amd", "csrc", "quantity.h")).read()
    for name, code, what in (("FILTERED_VM", 16, "vm"), ("FILTERED_STRESS", 17, "stress")):
        assert int(re.search(r"VPS_%s\s*=\s*(\d+)" % name, hdr).group(1)) == code == getattr(device, name) == fr.CODES[what]
        assert device.FILTER_QUANTITIES[what] == code and device.NCOMP[code] == fr.NCH[what]
        assert code not in device.QUANTITY.values() and not device.needs_second_moment(code) and not device.is_tensor(code)
        assert "VPS_%s" % name in q
    body = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert not re.search(r"=\s*15\b", body) and 15 not in device.NCOMP                 # 15 stays unassigned
    assert "vps_quantity_filter" in q
    assert re.search(r"#define VPS_FLAG_FILTER\(m\) \(\(\(m\) & 0xfff\) << 12\)", hdr)
    assert re.search(r"#define VPS_FLAG_FILTER_MASK 0xfff000", hdr)
    assert device.FLAG_FILTER(1) == 0x1000 and device.FLAG_FILTER(8) == 0x8000 and device.FLAG_FILTER(0xfff) == device.FLAG_FILTER_MASK
    assert "sin((2m+1) k_a Lcell / 2)" in hdr and "K = 6m + 134" in hdr and fr.chain(8) == 182
    assert "filter.hip" in _ffi.SOURCES
    src = open(os.path.join(ROOT, "large-velocity-power-spectrum_amd", "csrc", "filter.hip")).read()
    assert "K = 6m + 134" in src
    internal = open(os.path.join(ROOT, "large-velocity-power-spectrum_amd", "csrc", "vps_internal.h")).read()
    assert int(re.search(r"#define VPS_FILTER_MAX_HALF_WIDTH (\d+)", internal).group(1)) == device.FILTER_MAX_HALF_WIDTH == 8


def test_abi_13_and_81_declarations_hold():
    from vpower import _ffi
    hdr = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    assert int(re.search(r"#define VPS_ABI_VERSION (\d+)", hdr).group(1)) == 13 == _ffi.ABI_VERSION
    body = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vps_[a-z0-9_]+)\s*\(", body))
    assert declared == {s[0] for s in _ffi.SYMBOLS} and len(declared) == 81


@pytest.mark.parametrize("name", ["filtered_vm", "filtered_stress", "vm", "stress", "scale_flux", "subfilter_stress"])
def test_the_spectrum_routes_do_not_learn_the_names(name):
    from vpower import device
    with pytest.raises(Exception, match="Unrecognized physical quantity name"):
        device.resolve_quantity(name)


def test_wrapper_refuses_bad_arguments_before_the_library():
    import torch
    from vpower import device
    f = device.HipKernels.box_filter
    ch = torch.zeros((4, 6, 6, 6))
    for what in ("velocity", "strain_rate", 0, 14, 15, 18):
        with pytest.raises(ValueError, match="box_filter forms"):
            f(object(), ch, 6, 1, what)
    with pytest.raises(ValueError, match="whole grid"):
        f(object(), ch[:, :2], 6, 1, "vm")                     # an x-slab of a grid
    with pytest.raises(ValueError, match="whole grid"):
        f(object(), ch[:3], 6, 1, "vm")
    with pytest.raises(ValueError, match="even N"):
        f(object(), torch.zeros((4, 5, 5, 5)), 5, 1, "vm")
    with pytest.raises(ValueError, match="even N"):
        f(object(), torch.zeros((4, 2, 2, 2)), 2, 1, "vm")
    for hw in (0, -1, 9, 1.5, 4096):
        with pytest.raises(ValueError, match="half-width"):
            f(object(), ch, 6, hw, "stress")
    with pytest.raises(ValueError, match="wider than the grid"):
        f(object(), ch, 6, 3, "vm")
