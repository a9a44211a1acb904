"""The separable-field reference of oracle/gpu_checks.py pinned to the oracle (no GPU).

tests/test_gpu_spectrum_matrix.py checks the device spectrum at every grid size against `separable_shell_sums` and
`separable_plane`, which never materialise a field.  Here, at sizes where the oracle can follow, the same separable fields
are materialised and run through orc.vector_power / orc.scalar_power + orc.spectrum_table (the functions the goldens pin):
shell counts must agree bit for bit and shell sums to 1e-12, with both binning flavours, a custom bin width, one rank's
subset of kz planes and a CIC window table.

The custom k ranges of tests/test_gpu_krange_matrix.py (gpu_checks.K_RANGES) are pinned the same way at N = 32, Helmholtz
reference included, and the table's own properties -- consistent edges, the binning mode every row must select, the slot
kinds of the packed exchange -- are asserted for every (N, row) the GPU legs use, so that an edit of the table cannot
silently stop reaching the paths it is there for."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import vps_oracle as orc  # noqa: E402
from oracle import gpu_checks as chk  # noqa: E402

DEV = "cpu"


def _field64(factors):
    a, b, c = factors
    return np.einsum("rx,ry,rz->xyz", a, b, c)


def _tables(N, L, flavour, kres):
    from vpower import device
    kmin, kmax, _ = orc.default_k_range(L, N)
    centers, edges = device.bin_edges(kmin, kmax, kmin if kres is None else kres, flavour)
    k2 = device.k_axis(L, N) ** 2
    return edges, k2, device.sqrt_thresholds(edges)


@pytest.mark.parametrize("N,L,ncomp,flavour,kres", [(16, 1.0, 3, "library", None), (32, 2.5, 3, "script", None),
                                                    (96, 1.0, 3, "library", 0.37), (250, 1.0, 1, "library", None),
                                                    (250, 1.0, 1, "script", 1.6)])
def test_separable_shell_sums_equal_the_oracle(N, L, ncomp, flavour, kres):
    comps = [chk.separable_factors(N, 3, seed=100 * N + i) for i in range(ncomp)]
    fields = [_field64(f) for f in comps]
    kres_abs = None if kres is None else kres * 2 * np.pi / L
    P = orc.vector_power(*fields, L, N) if ncomp == 3 else orc.scalar_power(fields[0], L, N)
    ref = orc.spectrum_table(P, L, N, flavour, kres=kres_abs)
    edges, k2, thr = _tables(N, L, flavour, kres_abs)
    psum, counts = chk.separable_shell_sums(DEV, comps, N, L, k2, thr)
    assert np.array_equal(counts, ref[:, 3])
    assert np.allclose(psum, ref[:, 2], rtol=1e-12, atol=0)
    # the counts are those of shell_counts_exact, the checker of the full-size tests
    assert np.array_equal(counts, chk.shell_counts_exact(DEV, N, k2, thr))


@pytest.mark.parametrize("N", [32, 96])
def test_separable_shell_sums_kz_subset_nyquist_rows_and_window(N):
    """One rank's share: a kz subset with part of the Nyquist plane's rows, and a CIC 1/W^2 axis table (the float32 table
    the pipeline uploads, vpower.device.window_inv2_axis, itself within 1e-6 of the oracle's float64 window)."""
    from vpower import device
    L, flavour = 2.5, "library"      # (at L = 1 the reference's np.arange edges are inconsistent for N = 96)
    comps = [chk.separable_factors(N, 3, seed=7 * N + i) for i in range(3)]
    P = orc.vector_power(*[_field64(f) for f in comps], L, N)
    h = N // 2
    win = device.window_inv2_axis(N, "cic")
    w64 = win.astype(np.float64)
    assert np.allclose(w64[:, None, None] * w64[None, :, None] * w64[None, None, :], orc.window_inv2(N, "cic"), rtol=1e-6)
    edges, k2, thr = _tables(N, L, flavour, None)
    G, r = 4, 1
    kz = list(range(r, h, G)) + [h]
    nyq = (r * N // G, (r + 1) * N // G)
    for win_ in (None, win):
        Pw = P if win_ is None else P * (w64[:, None, None] * w64[None, :, None] * w64[None, None, :])
        # the full-spectrum modes the subset stands for: kz and N - kz of every plane kz < N/2, the Nyquist plane's given rows
        mask = np.zeros((N, N, N), dtype=bool)
        for k in kz:
            if k == h:
                mask[:, nyq[0]:nyq[1], h] = True
            else:
                mask[:, :, k] = True
                mask[:, :, (N - k) % N] = True
        kk = orc.pair_power(Pw, L, N)[:, 0]
        ref_ps, _ = np.histogram(kk[mask.ravel()], bins=edges, weights=Pw.ravel()[mask.ravel()])
        ref_ns, _ = np.histogram(kk[mask.ravel()], bins=edges)
        psum, counts = chk.separable_shell_sums(DEV, comps, N, L, k2, thr, kz=kz, win=win_, nyq_ky=nyq)
        assert np.array_equal(counts, ref_ns)
        assert np.allclose(psum, ref_ps, rtol=1e-12, atol=0)


@pytest.mark.parametrize("N", [16, 96, 250])
def test_separable_slab_and_plane(N):
    """separable_slab is the float64 field rounded once to float32; separable_plane is numpy's rfftn of that field."""
    f = chk.separable_factors(N, 3, seed=N)
    f64 = _field64(f)
    x0, nx = N // 4, N // 2
    slab = chk.separable_slab(DEV, f, x0, nx).numpy()
    assert slab.dtype == np.float32 and slab.shape == (nx, N, N)
    assert np.all(np.abs(slab - f64[x0:x0 + nx]) <= 2.0 ** -24 * np.abs(f64[x0:x0 + nx]))
    F = np.fft.rfftn(f64)                                                   # [kx, ky, kz <= N/2]
    for kz in (0, 1, N // 2 - 1, N // 2):
        got = chk.separable_plane(DEV, f, kz).numpy()                       # [ky, kx]
        assert np.allclose(got, F[:, :, kz].T, rtol=0, atol=1e-12 * np.abs(F).max())
    planes = chk.separable_plane(DEV, f, [0, N // 2, 1]).numpy()
    assert np.allclose(planes, F[:, :, [0, N // 2, 1]].transpose(2, 1, 0), rtol=0, atol=1e-12 * np.abs(F).max())
    rows = slice(N // 8, N // 4)
    assert np.allclose(chk.separable_plane(DEV, f, 3, ky=rows).numpy(), chk.separable_plane(DEV, f, 3).numpy()[rows],
                       rtol=0, atol=1e-14 * np.abs(F).max())


# ------------------------------------------------------------------------- custom k ranges (gpu_checks.K_RANGES) ----
def _range_tables(name, N, L=None):
    from vpower import device
    L = chk.k_range_box(name, N) if L is None else L
    flavour, kmin, kmax, kres = chk.k_range(name, N, L)
    centers, edges = device.bin_edges(kmin, kmax, kres, flavour)
    k2 = device.k_axis(L, N) ** 2
    return L, flavour, (kmin, kmax, kres), edges, k2, device.sqrt_thresholds(edges)


@pytest.mark.parametrize("name", list(chk.K_RANGES))
def test_separable_references_equal_the_oracle_at_every_k_range(name):
    """Both separable references with the thresholds of every row at N = 32 against orc.spectrum_table and
    helmholtz_ref.helmholtz_tables with the row's kmin, kmax, kres.  `zero`: the k = 0 mode is counted in bin 0 (np.histogram's
    left-closed first bin at edge 0) with its power in the total and NO compressive part (k' = 0)."""
    import helmholtz_ref as hr
    N = 32
    L, flavour, (kmin, kmax, kres), edges, k2, thr = _range_tables(name, N)
    comps = [chk.separable_factors(N, 3, seed=300 * N + i) for i in range(3)]
    fields = [_field64(f) for f in comps]
    ref = orc.spectrum_table(orc.vector_power(*fields, L, N), L, N, flavour, kmin, kmax, kres)
    psum, counts = chk.separable_shell_sums(DEV, comps, N, L, k2, thr)
    assert np.array_equal(counts, ref[:, 3]) and counts.sum() > 0
    # (a float64 FFT is good to ~1e-16 of the rms mode, not of every mode: `corner` has a bin of one weak mode, (N/2, N/2, N/2))
    floor = 1e-12 * counts * psum.sum() / counts.sum()
    assert np.all(np.abs(psum - ref[:, 2]) <= 1e-12 * ref[:, 2] + floor)
    assert np.array_equal(counts, chk.shell_counts_exact(DEV, N, k2, thr))
    t_tot, t_comp, _ = hr.helmholtz_tables(*fields, L, N, flavour, kmin, kmax, kres)
    ps_t, ps_c, ns = hr.separable_helmholtz_sums(DEV, comps, N, L, k2, thr)
    assert np.array_equal(ns, t_tot[:, 3]) and np.array_equal(ns, counts)
    assert np.all(np.abs(ps_t - t_tot[:, 2]) <= 1e-12 * ps_t + floor) and np.all(np.abs(ps_t - psum) <= 1e-12 * psum + floor)
    assert np.all(np.abs(ps_c - t_comp[:, 2]) <= 1e-12 * ps_c + floor)
    if name == "zero":
        assert edges[0] == 0.0 and thr[0] == 0.0
        # bin 0 = [0, kf) holds the k = 0 mode alone: all of its power is in the total, none in the compressive part
        p0 = 0.5 * orc.power_const(L, N) ** 2 * sum(f.sum() ** 2 for f in fields)
        assert counts[0] == 1 and p0 > 1e-3 * psum[1] and np.isclose(psum[0], p0, rtol=1e-10) and ps_c[0] == 0.0
        assert counts.sum() == N ** 3 - np.sum(orc.pair_power(np.zeros(N ** 3), L, N)[:, 0] > edges[-1])


def test_k_range_table_reaches_what_it_is_there_for():
    """Every (N, row) of the GPU legs: edges consistent at the chosen L, the binning mode the documented rule gives
    (gpu_checks.expected_binning_mode) as listed, the row cut and slot kinds of the packed exchange, the bin counts."""
    from vpower import device
    used = {(name, N) for legs in (chk.K_WHOLE, chk.K_HELMHOLTZ, chk.K_WINDOW) for N, names in legs.items() for name in names}
    used |= {(name, N) for N, _, _ in chk.K_SLABS for name in chk.K_SLAB_ROWS} | {(name, 128) for name in chk.K_ROUTE_ROWS}
    for name, N in sorted(used):
        L, flavour, (kmin, kmax, kres), edges, k2, thr = _range_tables(name, N)
        assert chk.k_range_edges(name, N, L) is not None and len(thr) == len(edges)
        if name in chk.K_ROUTE_ROWS:         # the user-facing routes bin with the library flavour
            device.bin_edges(kmin, kmax, kres, "library")
        mode = chk.expected_binning_mode(N, k2, thr, edges)
        assert mode == (1 if (name, N) in chk.K_MODE1 else 2), (name, N, mode)
        nb = len(edges) - 1
        kcut = chk.row_cut(N, k2, thr)
        h = N // 2
        if name == "deep":
            assert (kcut < 0).sum() > h // 2                        # most planes: no row kept
        if name in ("band", "many", "fine"):
            assert (kcut < 0).any()
        if name == "band":
            assert thr[0] > 4 * k2[1]                               # modes below the first edge exist
        if name == "zero":
            assert edges[0] == 0.0 and thr[0] == 0.0 and (kcut >= 0).all()
        if name == "corner":
            assert (kcut == h).all()                                # nothing cut
        if name == "fine":
            assert 0.6 * N < nb < 0.75 * N
        if name == "many":
            assert 0.9 * N < nb <= N and (N != 1024 or nb == 985)
            counts = chk.shell_counts_exact(DEV, N, k2, thr)
            assert counts[counts > 0].min() >= 18, (N, counts[counts > 0].min())
        if name == "wide":
            assert nb == 2
    for N, G, C in chk.K_SLABS:
        for name in chk.K_SLAB_ROWS:
            L, flavour, _, edges, k2, thr = _range_tables(name, N)
            mix = chk.slot_mix(chk.row_cut(N, k2, thr), N, G, C)
            assert mix["slots"] == N // 2 // G
            if name == "corner":
                assert mix["full"] == mix["slots"]
            if name == "band" or (name == "deep" and (N, G, C) != (128, 4, 2)):
                assert mix["mixed"] >= 1, (N, G, C, name)
            if name in ("deep", "band"):
                assert mix["dead"] >= 5
            if name == "zero":
                assert mix["unequal"] >= 2 and mix["dead"] == 0
