"""float64 references and small fixtures shared by the GPU test modules that drive the library's routes (tests/test_gpu_guarded.py,
tests/test_gpu_streams.py): constructed integer particles, the per-cell quantity fields of a [rho v, rho] grid, numpy-convention
z / zy images, the send buffer vps_fft_y owes, the exact-neighbour set-up, and a spy on the reuse token.  TEST INFRASTRUCTURE ONLY."""
import contextlib

import numpy as np
import torch

import density_ref as dref
import weighted_ref as wref
from oracle import gpu_checks as chk
from oracle import vps_oracle as orc


class P:
    """Constructed integer particles on the device."""

    def __init__(self, G, n, N, dtype, dist, seed):
        self.cells, self.pos, self.rho, self.vel = chk.constructed_particles(G.device, n, N, 1.0, dtype, dist, seed=seed)
        self.n, self.N = n, N

    def payload(self, C):
        r = self.rho.to(torch.int64)
        if C == 1:
            return r[:, None].contiguous()
        rv = r[:, None] * self.vel.to(torch.int64)
        return rv if C == 3 else torch.cat([rv, r[:, None]], dim=1)


def vec_grid(p, N, x0, nx):
    """float64 numpy [nx, N, N, 4] = exact cell totals [sum rho v, sum rho] of the rows."""
    s = chk.exact_slab_reference(p.cells, p.rho, p.vel, N, x0, nx)
    return torch.stack([s[1], s[2], s[3], s[0]], dim=-1).double().cpu().numpy().reshape(nx, N, N, 4)


ALPHA = {"weighted_third": 1.0 / 3.0, "weighted_half": 0.5, "density_1": 1.0, "density_third": 1.0 / 3.0, "density_half": 0.5}


def reference_fields(vec_grid, Lcell, name):
    """float64 component fields of quantity `name` from a [rho v, rho] grid (..., 4): the oracle's rules and the per-quantity
    references of tests/weighted_ref.py and tests/density_ref.py."""
    v, m = orc.vm_from_vec_grid(vec_grid, Lcell, zero_empty=True)
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    if name == "velocity":
        return [vx, vy, vz]
    if name == "vm":
        return [vx, vy, vz, m]
    if name in ("momentum", "momentum_bug"):
        return list(orc.momentum_fields(vx, vy, vz, m, reference_compat=name == "momentum_bug"))
    if name == "energy":
        return [orc.kinetic_energy_field(vx, vy, vz, m)]
    if name.startswith("weighted"):
        return wref.fields_from_vec_grid(vec_grid, ALPHA[name])
    return [dref.field(vec_grid, "log" if name == "log_density" else ALPHA[name])]


def zy_reference(field, N, nx):
    """(spec [N/2, N, nx], nyq [N, nx]) complex128 of a float64 field [nx, y, z]: numpy's forward transform along z (real) and y."""
    F = torch.fft.fft(torch.fft.rfft(field, dim=2), dim=1)              # [x, ky, kz <= N/2]
    return F[:, :, : N // 2].permute(2, 1, 0).contiguous(), F[:, :, N // 2].permute(1, 0).contiguous()


def z_reference(field, N):
    """The z image (flat: B[x][kz][y] for kz < N/2, then BN[x][y]) of a float64 field [nx, y, z]."""
    Z = torch.fft.rfft(field, dim=2)                                       # [x, y, kz]
    return torch.cat([Z[:, :, : N // 2].permute(0, 2, 1).reshape(-1), Z[:, :, N // 2].reshape(-1)])


def fused_refs(G, t, N, x0, nx, names):
    vec = vec_grid(t, N, x0, nx)
    out = {}
    for name in names:
        out[name] = [zy_reference(torch.as_tensor(np.ascontiguousarray(f), device=G.device), N, nx)
                     for f in reference_fields(vec, 1.0 / N, name)]
    return out


@contextlib.contextmanager
def reuse_flags(G):
    """Records what every _reuse_flag of the block returned (FLAG_REUSE_SORT: the reuse under test did happen)."""
    taken, orig = [], G._reuse_flag

    def spy(*a, **k):
        taken.append(orig(*a, **k))
        return taken[-1]
    G._reuse_flag = spy
    try:
        yield taken
    finally:
        del G._reuse_flag


def expected_chunk(spec, nyq, N, nx, R, C, c, kcut):
    """The send buffer vps_fft_y owes for chunk c of one sender slab, restated on the host from include/vps_hip.h (vps_fft_y,
    vps_set_bin_only) and the row-cut rule of oracle/gpu_checks.py: -> (values complex128 [R * block], stored bool [R * block]).
    kcut None: plain slots of N rows, everything stored.  Packed: slot j of every destination carries the 2 kc + 1 rows
    |ky| <= kc, kc the largest cut of the slot's R planes (row ky at position ky, row N - i at position 2 kc + 1 - i), or all N
    rows; of those a plane STORES the rows with min(ky, N - ky) <= its own cut -- the others, and every row of a plane no shell
    reaches, are never written.  The Nyquist rows of the last chunk obey the cut of the plane kz = N/2."""
    nkc = N // 2 // R // C
    dev = spec.device
    vals, stored = [], []
    for h in range(R):
        for j in range(nkc):
            kz = c * R * nkc + j * R + h
            ky = torch.arange(N, device=dev)
            keep = torch.ones(N, dtype=torch.bool, device=dev)
            if kcut is not None:
                cuts = [int(kcut[c * R * nkc + j * R + r]) for r in range(R)]
                kc = max(max(cuts), 0)
                if chk.slot_rows(cuts, N) < N:
                    ky = torch.cat([torch.arange(0, kc + 1, device=dev), torch.arange(N - kc, N, device=dev)])
                assert ky.numel() == chk.slot_rows(cuts, N)
                keep = torch.minimum(ky, N - ky) <= int(kcut[kz])
            vals.append(spec[kz][ky].reshape(-1))
            stored.append(keep[:, None].expand(-1, nx).reshape(-1))
        if c == C - 1:
            ky = torch.arange(h * (N // R), (h + 1) * (N // R), device=dev)
            keep = torch.ones(ky.numel(), dtype=torch.bool, device=dev) if kcut is None else torch.minimum(ky, N - ky) <= int(kcut[N // 2])
            vals.append(nyq[ky].reshape(-1))
            stored.append(keep[:, None].expand(-1, nx).reshape(-1))
    return torch.cat(vals), torch.cat(stored)


NN_REF = {}


def nn_setup(G, n, lattice, x0, nx, seed, ref=True):
    """(pos, integer payload [rho v, rho], axes, exact neighbour index or None) -- the reference once per set-up."""
    key = (n, lattice, x0, nx, seed)
    if key not in NN_REF:
        axes = chk.nn_matrix_axes(lattice, seed=7)
        taxes = [chk._axis(a, G.device) for a in axes]
        pos, _ = chk.nn_matrix_particles(G.device, n, torch.float32, axes, x0, nx, seed=seed)
        g = torch.Generator(device=G.device)
        g.manual_seed(seed)
        rho = torch.randint(1, 4, (n, 1), generator=g, device=G.device).float()
        vel = torch.randint(-3, 4, (n, 3), generator=g, device=G.device).float()
        pay = torch.cat([rho * vel, rho], dim=1).contiguous()
        ny = len(axes[1])
        idx = None
        if ref:
            idx, _ = chk.nn_brute_force(pos, chk.lattice_points(taxes, x0, nx, torch.arange(nx * ny * ny, device=G.device)), batch=4096)
        NN_REF[key] = (pos, pay, axes, idx)
    return NN_REF[key]
