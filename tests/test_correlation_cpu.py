"""Two-point correlation and structure functions: everything that needs no GPU.
  - the FFT reference (tests/correlation_ref.py) against a direct sum over all pairs;
  - the host r tables (vpower.device.radial_edges / r_axis / binning_tables) against numpy.histogram on every lattice point;
  - the CorrelationFunction container;
  - include/vps_hip.h documents vps_fft_x modes 5 - 7 and declares what it declared before;
  - the public names exist.
"""
import os
import re

import numpy as np
import pytest

import correlation_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ the reference against a pair sum ----
@pytest.mark.parametrize("ncomp", [1, 3])
def test_fft_reference_against_direct_pair_sum(ncomp):
    N = 8
    rng = np.random.default_rng(5 + ncomp)
    fields = [rng.standard_normal((N, N, N)) + 0.3 for _ in range(ncomp)]
    xi_f, xi_d = cref.xi_grid(fields), cref.xi_direct(fields)
    scale = xi_d[0, 0, 0]
    assert np.max(np.abs(xi_f - xi_d)) <= 1e-13 * scale
    # S2 = <|f(x + r) - f(x)|^2> directly, against 2 (xi(0) - xi(r))
    s2 = np.zeros((N, N, N))
    for f in fields:
        for a in range(N):
            for b in range(N):
                for c in range(N):
                    s2[a, b, c] += np.mean((np.roll(f, (-a, -b, -c), axis=(0, 1, 2)) - f) ** 2)
    assert np.max(np.abs(s2 - 2 * (xi_d[0, 0, 0] - xi_f))) <= 1e-12 * scale
    # the shell table of the half lattice with Hermitian weights is the histogram of the full lattice
    edges = cref.default_edges(1.0, N)
    xb, cnt, xi0 = cref.correlation(fields, 1.0, edges, subtract_mean=False)
    rfull = cref.lattice_r(1.0, N, np.arange(N))
    full_cnt = np.histogram(rfull.ravel(), edges)[0]
    full_sum = np.histogram(rfull.ravel(), edges, weights=xi_d.ravel())[0]
    assert np.array_equal(cnt, full_cnt) and cnt[0] == 1
    assert np.allclose(xb * cnt, full_sum, rtol=0, atol=1e-12 * scale * cnt.max())
    assert xi0 == xi_f[0, 0, 0] and abs(xb[0] - xi0) <= 1e-13 * scale


# ------------------------------------------------------------------------------ host tables ----
def _host_decision(tables, planes):
    """The shell of every lattice point of `planes` as the library decides it: thr[b] <= s < thr[b + 1], s = (a2[x] + a2[y]) + a2[z]."""
    _, a2, thr, _, _ = tables
    s = (a2[None, None, :] + a2[None, :, None]) + a2[planes][:, None, None]
    return np.searchsorted(thr, s.ravel(), side="right") - 1


@pytest.mark.parametrize("N", [16, 96])
@pytest.mark.parametrize("case", ["default", "band", "offgrid"])
def test_host_r_tables_against_numpy_histogram(N, case):
    from vpower import device as D
    L = 1.7
    Lcell = L / N
    kw = {"default": {}, "band": dict(rmin=2.5 * Lcell, rmax=0.4 * L), "offgrid": dict(rres=0.37 * Lcell, rmax=np.sqrt(3) * L / 2 + 0.37 * Lcell)}[case]
    edges = D.radial_edges(L, N, **kw)
    tables = D.binning_tables(D.r_axis(L, N), edges)
    nb = len(edges) - 1
    assert tables[0] == N and len(tables[2]) == nb + 1
    assert np.array_equal(D.r_axis(L, N), cref.r_axis(L, N))
    planes = np.arange(N // 2 + 1)
    b = _host_decision(tables, planes)
    inside = (b >= 0) & (b < nb)
    got = np.bincount(b[inside], minlength=nb)
    ref = np.histogram(cref.lattice_r(L, N, planes).ravel(), edges)[0]
    assert np.array_equal(got, ref)
    # the first guess of the kernel, (sqrt(s) - edge0) * inv_spacing, names the same uniform edges
    assert np.allclose((edges - tables[3]) * tables[4], np.arange(nb + 1), rtol=0, atol=1e-9)
    if case == "default":
        assert np.array_equal(edges, cref.default_edges(L, N)) and nb == N // 2
        assert edges[-1] == D.r_axis(L, N)[N // 2]                       # the last bin is right-closed at L/2 itself
        assert ref[0] == 1                                               # r = 0 alone
        # every threshold sits on an integer multiple of r2[1]: the integer shell decision must be declined (vps_set_binning
        # refuses it within 1e-9 relative; tests/test_gpu_correlation.py reads vps_binning_mode)
        q = tables[2][1:] / tables[1][1]
        assert np.all(np.abs(q - np.rint(q)) <= 1e-9 * q)
    if case == "offgrid":
        w = cref.hermitian_weight(N, planes)[:, None, None]
        cnt = cref.shells(cref.lattice_r(L, N, planes), np.zeros((len(planes), N, N)), w, edges)[1]
        assert cnt.sum() == N ** 3                                       # the last edge lies beyond sqrt(3) L / 2: every lag is counted


def test_radial_edges_refuses_nonsense():
    from vpower import device as D
    for kw in (dict(rres=0.0), dict(rmin=-1.0), dict(rmin=0.3, rmax=0.2), dict(rmin=0.1, rmax=0.2, rres=0.5)):
        with pytest.raises(ValueError):
            D.radial_edges(1.0, 16, **kw)


# ------------------------------------------------------------------------------ the container ----
def test_correlation_function_round_trip(tmp_path):
    from vpower.spctrm import CorrelationFunction
    import vpower
    rng = np.random.default_rng(2)
    tab = np.column_stack((np.arange(5) + 0.5, rng.standard_normal(5), np.array([1, 6, 12, 0, 30.0])))
    xi0 = 1.0 / 3.0
    cf = CorrelationFunction(tab, xi0)
    assert vpower.CorrelationFunction is CorrelationFunction
    assert len(cf) == 5 and np.array_equal(cf.data(), tab) and cf.xi0 == xi0
    assert np.array_equal(np.array(list(cf)), tab) and np.array_equal(cf[1], tab[1])
    s2 = cf.structure_function()
    assert s2.shape == (5, 3) and np.array_equal(s2[:, 0], tab[:, 0]) and np.array_equal(s2[:, 2], tab[:, 2])
    ok = tab[:, 2] > 0
    assert np.array_equal(s2[ok, 1], 2.0 * (xi0 - tab[ok, 1])) and s2[3, 1] == 0
    cf.savetxt(str(tmp_path / "xi.txt"))
    back = CorrelationFunction.loadtxt(str(tmp_path / "xi.txt"))
    assert np.array_equal(back.data(), tab) and back.xi0 == xi0
    cf.save(str(tmp_path))
    again = CorrelationFunction.load(str(tmp_path))
    assert np.array_equal(again.data(), tab) and again.xi0 == xi0
    c2 = cf.copy()
    c2.xi[0] = 7.0
    assert cf.xi[0] == tab[0, 1]
    np.savetxt(str(tmp_path / "pk.txt"), tab)
    with pytest.raises(Exception):
        CorrelationFunction.loadtxt(str(tmp_path / "pk.txt"))


# ------------------------------------------------------------------------------ header and names ----
def test_header_documents_the_modes_and_declares_nothing_new():
    from vpower import _ffi
    text = open(os.path.join(ROOT, "include", "vps_hip.h")).read()
    assert "#define VPS_ABI_VERSION 13" in text and _ffi.ABI_VERSION == 13
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vps_[a-z0-9_]+)\s*\(", code))
    assert declared == {s[0] for s in _ffi.SYMBOLS} and len(declared) == 81
    at = text.index("int vps_fft_x(")
    comment = text[text.rindex("/*", 0, at): at]
    for word in ("mode 5:", "mode 6:", "mode 7:", "[N-kz][(N-ky)%N][(N-kx)%N]", "Re F", "nseg must be 1", "vps_set_window", "0..7"):
        assert word in comment, word


def test_public_names():
    import vpower
    from vpower import device as D, interp
    from vpower.spctrm import CorrelationFunction
    assert callable(interp.BoxField.correlation) and callable(interp.BoxField.structure_function)
    assert vpower.BoxField is interp.BoxField and "CorrelationFunction" in interp.__all__
    assert CorrelationFunction.columns == ("r", "xi", "Nsample")
    for name in ("CorrelationPipeline", "radial_edges", "r_axis", "binning_tables"):
        assert hasattr(D, name), name
    for name in ("power_grid_full", "bin_real", "fft_x_mode"):
        assert callable(getattr(D.HipKernels, name)), name


def test_k_tables_are_what_they_were():
    """binning_tables is the routine PowerPipeline builds its k tables with: the same five arguments as the expressions it replaced."""
    from vpower import device as D
    for N, L in ((16, 1.0), (96, 2.3)):
        ks = D.k_axis(L, N)
        kmin = 2 * np.pi / L
        centers, edges = D.bin_edges(kmin, np.pi / (L / N), kmin, "library")
        t = D.binning_tables(ks, edges)
        assert t[0] == N and np.array_equal(t[1], ks * ks) and np.array_equal(t[2], D.sqrt_thresholds(edges))
        assert t[3] == float(edges[0]) and t[4] == 1.0 / ((edges[-1] - edges[0]) / len(centers))
