"""CPU stand-in for the Helmholtz calls of vpower.device.HipKernels (include/vps_hip.h: vps_fft_x_bin_helmholtz,
vps_fft_x_bin_chunk_helmholtz): OracleKernels plus the decomposition, for the tests of the host-side slab choreography
without a GPU.  Test infrastructure, never imported by the package."""
import numpy as np
import torch

from helmholtz_ref import kprime
from oracle_kernels import OracleKernels


class HelmholtzOracleKernels(OracleKernels):
    name = "oracle-cpu-helmholtz"

    def fft_x_bin_helmholtz(self, comps, N, nlines, line0, kz0, nseg, seg_stride, psum, nsample, pcomp, count=True):
        """x pass of the three component spectra: sum_c |F_c|^2 into psum (as fft_x_bin_multi), |k'.F|^2 / |k'|^2 into pcomp."""
        assert len(comps) == 3
        Nb, k2, thr = self.binning
        assert Nb == N
        F = [np.fft.fft(self._lines(c, N, nlines, nseg, seg_stride).astype(np.complex128), axis=1) for c in comps]
        g = line0 + np.arange(nlines)
        ky, kz = g % N, kz0 + g // N
        assert kz.max() <= N // 2
        kp = kprime(N)
        D = kp[None, :] * F[0] + kp[ky][:, None] * F[1] + kp[kz][:, None] * F[2]
        kk = kp[None, :] ** 2 + (kp[ky] ** 2 + kp[kz] ** 2)[:, None]
        pc = np.where(kk > 0, np.abs(D) ** 2 / np.where(kk > 0, kk, 1.0), 0.0)
        pw = sum(f.real ** 2 + f.imag ** 2 for f in F)
        s = (k2[None, :] + k2[ky][:, None]) + k2[kz][:, None]
        w = np.where((kz == 0) | (2 * kz == N), 1, 2)[:, None] * np.ones((1, N), dtype=np.int64)
        b = np.searchsorted(thr, s, side="right") - 1
        ok = (b >= 0) & (b < len(thr) - 1)
        nb = len(thr) - 1
        psum += torch.from_numpy(np.bincount(b[ok], weights=(pw * w)[ok], minlength=nb))
        pcomp += torch.from_numpy(np.bincount(b[ok], weights=(pc * w)[ok], minlength=nb))
        if count:
            nsample += torch.from_numpy(np.rint(np.bincount(b[ok], weights=w[ok], minlength=nb)).astype(np.int64))

    def fft_x_bin_chunk_helmholtz(self, comps, N, nx, G, nchunks, chunk, rank, packed, psum, nsample, pcomp, count=True):
        """vps_fft_x_bin_chunk_helmholtz: the G received blocks per component -> planes in place (+ Nyquist rows), binned."""
        assert len(comps) == 3
        nkc, nky = N // 2 // G // nchunks, N // G
        slots = self._slots(N, G, nchunks, chunk, packed)
        blk = self.chunk_block(N, nx, G, nchunks, chunk, packed)
        rows_total = sum(r for _, r in slots)
        flats = [c.numpy().reshape(-1) for c in comps]
        for f in flats:
            assert f.size == G * blk
        r0 = 0
        for j, (kc, rows) in enumerate(slots):
            planes = []
            for flat in flats:
                plane = np.zeros((N, N), dtype=np.complex64)          # [ky][x]; rows that were not sent hold nothing binned
                keep = self._keep(N, kc)
                for g in range(G):
                    plane[keep, g * nx:(g + 1) * nx] = flat[g * blk + r0 * nx: g * blk + (r0 + rows) * nx].reshape(rows, nx)
                planes.append(torch.from_numpy(plane.reshape(-1)))
            self.fft_x_bin_helmholtz(planes, N, N, 0, chunk * G * nkc + j * G + rank, 1, N * N, psum, nsample, pcomp,
                                     count=count)
            r0 += rows
        if chunk == nchunks - 1:
            nyqs = [torch.from_numpy(np.ascontiguousarray(np.concatenate(
                [flat[g * blk + rows_total * nx: (g + 1) * blk].reshape(nky, nx) for g in range(G)], axis=1)).reshape(-1))
                for flat in flats]
            self.fft_x_bin_helmholtz(nyqs, N, nky, rank * nky, N // 2, 1, nky * N, psum, nsample, pcomp, count=count)
