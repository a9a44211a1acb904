"""CPU tests of the Helmholtz decomposition (BoxField.helmholtz_spctrm, PowerPipeline.*_helmholtz): the float64 references
of tests/helmholtz_ref.py pinned to the oracle and to each other, and the slab choreography of the decomposition over
gloo with the oracle-backed kernel stand-in (tests/helmholtz_kernels.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import helmholtz_ref as hr
from oracle import gpu_checks as chk
from oracle import vps_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(N, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((N, N, N)).astype(np.float32).astype(np.float64) for _ in range(3)]


@pytest.mark.parametrize("N,L,flavour", [(16, 1.0, "library"), (32, 2.5, "library"), (32, 1.0, "script")])
def test_total_is_spctrm_and_parts_add_up(N, L, flavour):
    f = _fields(N, 3)
    tot, comp, sol = hr.helmholtz_tables(*f, L, N, flavour)
    ref = orc.box_spctrm(*f, np.ones((N, N, N)), L / N, "velocity", flavour=flavour)
    assert np.array_equal(tot, ref, equal_nan=True)
    for t in (comp, sol):
        assert np.array_equal(t[:, 3], ref[:, 3]) and np.array_equal(t[:, 0], ref[:, 0])
    assert np.allclose(comp[:, 2] + sol[:, 2], ref[:, 2], rtol=1e-12, atol=0)
    assert (comp[:, 2] >= 0).all() and (sol[:, 2] >= -1e-12 * ref[:, 2]).all()
    # a generic field is neither: both parts carry power in every populated shell
    full = ref[:, 3] > 0
    assert (comp[full, 2] > 0).all() and (sol[full, 2] > 0).all()


@pytest.mark.parametrize("N", [16, 32])
def test_gradient_is_compressive_and_curl_is_solenoidal(N):
    L = 1.0
    tot, comp, sol = hr.helmholtz_tables(*hr.spectral_fields(N, "gradient", 1), L, N)
    assert (np.abs(sol[:, 2]) <= 1e-12 * tot[:, 2]).all()
    assert (comp[:, 2] > 0).any()
    tot, comp, sol = hr.helmholtz_tables(*hr.spectral_fields(N, "curl", 2), L, N)
    assert (np.abs(comp[:, 2]) <= 1e-12 * tot[:, 2]).all()
    assert (sol[:, 2] > 0).any()


@pytest.mark.parametrize("N,kind", [(16, None), (32, None), (32, "gradient")])
def test_half_spectrum_with_hermitian_weights_is_the_full_grid(N, kind):
    """k' is odd under k -> -k: the rfft half spectrum with the multiplicities 1 (kz = 0, N/2) / 2 reproduces the full-grid
    sums of both parts -- the property the binning x pass relies on (it sees the half spectrum only)."""
    L = 1.0
    f = _fields(N, 4) if kind is None else hr.spectral_fields(N, kind, 5)
    tot, comp, _ = hr.helmholtz_tables(*f, L, N, "script")
    _, edges = orc.edges_script(*orc.default_k_range(L, N))
    ps_t, ps_c, ns = hr.half_spectrum_sums(*f, L, N, edges)
    assert np.array_equal(ns, tot[:, 3])
    assert np.allclose(ps_t, tot[:, 2], rtol=1e-12, atol=0)
    assert np.allclose(ps_c, comp[:, 2], rtol=1e-12, atol=1e-14 * tot[:, 2].max())


def test_kprime_nyquist_convention():
    assert list(hr.kprime(8)) == [0, 1, 2, 3, 0, -3, -2, -1]
    assert list(hr.kprime(5)) == [0, 1, 2, -2, -1]


@pytest.mark.parametrize("N", [16, 32])
def test_separable_reference_is_the_fftn_reference(N):
    """The large-N yardstick of the GPU tests (full spectrum plane by plane, separable fields) against numpy fftn."""
    from vpower import device
    L = 1.0
    comps = [chk.separable_factors(N, 3, seed=70 + i) for i in range(3)]
    fields = []
    for a, b, c in comps:
        fields.append(np.einsum("rx,ry,rz->xyz", a, b, c))
    pipe_k2 = device.k_axis(L, N) ** 2
    centers, edges = device.bin_edges(*orc.default_k_range(L, N), "script")
    thr = device.sqrt_thresholds(edges)
    ps_t, ps_c, ns = hr.separable_helmholtz_sums("cpu", comps, N, L, pipe_k2, thr)
    tot, comp, _ = hr.helmholtz_tables(*fields, L, N, "script")
    assert np.array_equal(ns, tot[:, 3])
    assert np.allclose(ps_t, tot[:, 2], rtol=1e-12, atol=0)
    assert np.allclose(ps_c, comp[:, 2], rtol=1e-12, atol=0)
    win = device.window_inv2_axis(N, "cic").astype(np.float64)
    ps_tw, ps_cw, _ = hr.separable_helmholtz_sums("cpu", comps, N, L, pipe_k2, thr, win=win)
    assert (ps_tw >= ps_t).all() and (ps_cw >= ps_c).all() and (ps_tw > ps_t).any()


# -------------------------------------------------------------------------------------- slab choreography over gloo ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, N, L, seed, out_dir, chunks, form):
    for p in (ROOT, os.path.join(ROOT, "large-velocity-power-spectrum_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["VPS_A2A_CHUNKS"] = str(chunks)
    os.environ["VPS_X_PER_COMPONENT"] = "1"          # does not apply to the decomposition: ignored there
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vpower import device
        from helmholtz_kernels import HelmholtzOracleKernels
        fields = _fields(N, seed)
        pipe = device.PowerPipeline(N, L, kernels=HelmholtzOracleKernels(), comm=device.SlabComm())
        assert pipe.comm.world == world and pipe.chunked and pipe.nchunks == chunks
        slabs = [torch.from_numpy(np.ascontiguousarray(f[pipe.x0: pipe.x0 + pipe.nx]).astype(np.float32)) for f in fields]
        if form == "spectrum":
            tabs = pipe.spectrum_helmholtz(slabs)
        else:      # two quantities through one bounded pipeline: plain velocity, then its decomposition
            k = pipe.k
            plain = pipe.new_accumulators()
            helm = pipe.new_accumulators(helmholtz=True)
            pipe.pipelined_quantities([lambda: [k.fft_z(s, N, pipe.nx) for s in slabs]] * 2, [plain, helm], counts=[True, True])
            tabs = pipe.finish_helmholtz(*helm)
            np.save(os.path.join(out_dir, f"plain_{rank}.npy"), pipe.finish(*plain))
            for t in tabs:
                t[:, 1] *= 4 * np.pi * t[:, 0] ** 2
        np.save(os.path.join(out_dir, f"tabs_{rank}.npy"), np.stack(tabs))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,N,chunks,form", [(2, 16, 1, "spectrum"), (2, 32, 2, "spectrum"), (4, 32, 2, "spectrum"),
                                                 (4, 32, 1, "pipelined")])
def test_slab_choreography_matches_one_rank_reference(tmp_path, world, N, chunks, form):
    L, seed = 1.0, 17
    mp.spawn(_worker, args=(world, _free_port(), N, L, seed, str(tmp_path), chunks, form), nprocs=world, join=True)
    ref = hr.helmholtz_tables(*_fields(N, seed), L, N, "library")
    for r in range(world):
        tabs = np.load(tmp_path / f"tabs_{r}.npy")
        for got, want in zip(tabs, ref):
            assert np.array_equal(got[:, 3], want[:, 3])
            assert np.array_equal(got[:, 0], want[:, 0])
        assert np.allclose(tabs[0][:, 2], ref[0][:, 2], rtol=1e-5)
        assert np.allclose(tabs[1][:, 2], ref[1][:, 2], rtol=1e-5)
        assert (np.abs(tabs[2][:, 2] - ref[2][:, 2]) <= 1e-5 * ref[0][:, 2]).all()
        assert np.allclose(tabs[0][:, 1], ref[0][:, 1], rtol=1e-5)
        if form == "pipelined":
            plain = np.load(tmp_path / f"plain_{r}.npy")
            assert np.array_equal(plain[:, 3], ref[0][:, 3]) and np.allclose(plain[:, 2], ref[0][:, 2], rtol=1e-5)
    assert np.array_equal(np.load(tmp_path / "tabs_0.npy"), np.load(tmp_path / f"tabs_{world - 1}.npy"))


def test_one_rank_pipeline_forms_match_reference():
    """accumulate_helmholtz (z/y passes + exchange-free x pass) and accumulate_spectra_helmholtz on one rank."""
    from vpower import device
    from helmholtz_kernels import HelmholtzOracleKernels
    N, L = 16, 1.0
    f = _fields(N, 9)
    ref = hr.helmholtz_tables(*f, L, N, "library")
    k = HelmholtzOracleKernels()
    pipe = device.PowerPipeline(N, L, kernels=k, comm=device.SlabComm(enabled=False))
    assert not pipe.chunked
    t32 = [torch.from_numpy(x.astype(np.float32)) for x in f]
    tabs = pipe.spectrum_helmholtz(t32)
    pipe.prepare()
    zy = [k.fft_zy(x, N, N) for x in t32]
    spec = torch.stack([s for s, _ in zy])
    nyq = torch.stack([q for _, q in zy])
    tabs2 = pipe.finish_helmholtz(*pipe.accumulate_spectra_helmholtz(spec, nyq))
    for got, got2, want in zip(tabs, tabs2, ref):
        assert np.array_equal(got[:, 3], want[:, 3]) and np.array_equal(got2[:, 3], want[:, 3])
        assert np.allclose(got[:, 2], want[:, 2], rtol=1e-5, atol=1e-5 * ref[0][:, 2].max())
        assert np.allclose(got2[:, 2], want[:, 2], rtol=1e-5, atol=1e-5 * ref[0][:, 2].max())
    with pytest.raises(Exception, match="three components"):
        pipe.accumulate_helmholtz(t32[:2])


def test_energy_and_unknown_quantities_refused_without_gpu():
    from vpower import interp
    bf = interp.BoxField(np.zeros((16, 16, 16, 3)), np.ones((16, 16, 16)), 1.0 / 16)
    for q in ("energy", "vorticity"):
        with pytest.raises(Exception, match="Unrecognized physical quantity name"):
            bf.helmholtz_spctrm(q)
