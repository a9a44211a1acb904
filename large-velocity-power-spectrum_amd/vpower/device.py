"""Device pipeline: particles -> slab grid -> 3-D R2C FFT -> |f|^2 -> shell bins.

Host-side orchestration only.  All arithmetic on grids and particles is done by the
HIP kernels of libvps_hip.so through `HipKernels`; torch supplies device buffers,
streams and (for more than one GPU) `torch.distributed` collectives.

Multi-GPU: 1-D slab decomposition along x, one process per GPU.  Particles are
replicated (as the reference replicates the snapshot on every MPI rank,
scripts/parallel_optimized.py:272-276); each rank deposits / resamples its own x-slab,
runs the z pass locally, then per kz chunk the y pass straight into the send buffer of an
all-to-all (ONE message per scalar field and pair of ranks, the Nyquist-plane rows riding
behind the last chunk; the chunks only pipeline it against the passes), runs the x pass
with fused binning on the arrived chunks and finally all-reduces the (nbins,) shell sums --
the step that replaces the two comm.Reduce calls at scripts/parallel_optimized.py:455-456.

The kernel set is injectable so that the distributed choreography can be exercised on
CPU tensors by the test-suite's oracle-backed stand-in; the product default is
`HipKernels` and there is no fallback from it.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np
import torch

from . import _ffi

VELOCITY, MOMENTUM, ENERGY, VM, WEIGHTED, DENSITY, LOG_DENSITY = 0, 1, 2, 3, 4, 5, 6
# the second-moment scalars of a cell's contributions (vps_deposit_field alone forms them: NGP / CIC / TSC deposits), with
# S2 = sum w rho_p |v_p|^2, P = sum w rho v, R = sum w rho: vol S2, vol (S2 - |P|^2 / R), (S2 - |P|^2 / R) / R
TOTAL_ENERGY, SUBGRID_ENERGY, DISPERSION = 7, 8, 9
# ... and the second moment itself, S_ij = sum w rho_p v_i v_j, as six fields xx, yy, zz, xy, xz, yz: the sub-grid stress
# vol (S_ij - P_i P_j / R) and the velocity-dispersion tensor (S_ij - P_i P_j / R) / R
SUBGRID_STRESS, DISPERSION_TENSOR = 10, 11
TENSOR_QUANTITIES = {"subgrid_stress": SUBGRID_STRESS, "dispersion_tensor": DISPERSION_TENSOR}
SECOND_MOMENT_QUANTITIES = {"total_energy": TOTAL_ENERGY, "subgrid_energy": SUBGRID_ENERGY, "dispersion": DISPERSION,
                            **TENSOR_QUANTITIES}
# central differences of the velocity of a WHOLE gridded field (vps_field_algebra_out alone forms them, csrc/gradient.hip):
# the dilatation, the vorticity (x, y, z) and the strain rate (xx, yy, zz, xy, xz, yz).  Kept OUT of QUANTITY: they are fields
# (BoxField.divergence / vorticity / strain_rate, HipKernels.velocity_gradient), not names the spectrum routes take.
DIVERGENCE, VORTICITY, STRAIN_RATE = 12, 13, 14
GRADIENT_QUANTITIES = {"divergence": DIVERGENCE, "vorticity": VORTICITY, "strain_rate": STRAIN_RATE}
# the mass-weighted box filter of a WHOLE gridded field at a half-width of m cells (vps_field_algebra_out alone, csrc/filter.hip):
# the filtered [v, mass] grid and the sub-filter stress (xx, yy, zz, xy, xz, yz).  15 stays unassigned (include/vps_hip.h).  Kept
# OUT of QUANTITY like the gradient codes: spectra of a filtered field come through BoxField.filtered(m).
FILTERED_VM, FILTERED_STRESS = 16, 17
FILTER_QUANTITIES = {"vm": FILTERED_VM, "stress": FILTERED_STRESS}
FILTER_MAX_HALF_WIDTH = 8          # what the kernel's LDS plan holds (csrc/vps_internal.h: VPS_FILTER_MAX_HALF_WIDTH)
QUANTITY = {"velocity": VELOCITY, "momentum": MOMENTUM, "energy": ENERGY, "weighted_velocity": WEIGHTED,
            "density": DENSITY, "log_density": LOG_DENSITY, **SECOND_MOMENT_QUANTITIES}
FLAG_REFERENCE_MOMENTUM_BUG = 1
FLAG_INPUT_IS_VM = 2
FLAG_REUSE_SORT = 4
FLAG_SHARE_ENERGY = 8
FLAG_FILTER_MASK = 0xfff000


def FLAG_FILTER(m):
    """VPS_FLAG_FILTER(m): the half-width m of the box filter (a box of (2m+1)^3 cells) in the flags of the two filter codes."""
    return (int(m) & 0xfff) << 12


NCOMP = {VELOCITY: 3, MOMENTUM: 3, ENERGY: 1, VM: 4, WEIGHTED: 3, DENSITY: 1, LOG_DENSITY: 1,      # output channels of a quantity
         TOTAL_ENERGY: 1, SUBGRID_ENERGY: 1, DISPERSION: 1,                                        # (csrc/quantity.h: vps_quantity_channels)
         SUBGRID_STRESS: 6, DISPERSION_TENSOR: 6, DIVERGENCE: 1, VORTICITY: 3, STRAIN_RATE: 6,
         FILTERED_VM: 4, FILTERED_STRESS: 6}
SCALAR_QUANTITIES = ("energy", "density", "log_density", "total_energy", "subgrid_energy", "dispersion")      # one field each: dealt out and transformed as one unit


def needs_second_moment(quantity):
    """Whether a quantity (name or code) is one of the second-moment quantities (the three scalars, the two tensors), which
    only a particle deposit can form."""
    return quantity in SECOND_MOMENT_QUANTITIES if isinstance(quantity, str) else int(quantity) in SECOND_MOMENT_QUANTITIES.values()


def is_tensor(quantity):
    """Whether a quantity (name or code) is one of the six-field tensor quantities, 'subgrid_stress' / 'dispersion_tensor'."""
    return quantity in TENSOR_QUANTITIES if isinstance(quantity, str) else int(quantity) in TENSOR_QUANTITIES.values()


def contraction_fields(fields, quantity):
    """The fields whose summed |F|^2 is the spectrum of `quantity`, from the fields a deposit returned.  A tensor quantity's six
    fields (xx, yy, zz, xy, xz, yz) stand for the nine components of a symmetric tensor: the full contraction
    sum_ij |T_ij|^2 counts each off-diagonal field twice, so those three are replaced by COPIES scaled by sqrt(2) (float32: the
    factor's square is 2 to 3e-8; the caller's fields are left as they are) and all six then go through the component-summing
    passes, three at a time, like any list of fields.  Every other quantity: the list as it is."""
    fields = list(fields)
    if is_tensor(quantity):
        if len(fields) != 6:
            raise Exception("a tensor quantity has six fields (xx, yy, zz, xy, xz, yz), got %d" % len(fields))
        fields[3:] = [f * float(np.float32(np.sqrt(2.0))) for f in fields[3:]]
    return fields


def flux_contraction(tau, S):
    """Pi = -tau_ij S_ij from the six fields (xx, yy, zz, xy, xz, yz) of a symmetric stress tau and of the strain rate S, each
    [6, ...]: -(tau_xx S_xx + tau_yy S_yy + tau_zz S_zz + 2 tau_xy S_xy + 2 tau_xz S_xz + 2 tau_yz S_yz), elementwise in the
    tensors' dtype and in this order of additions (the off-diagonal fields stand for two components each)."""
    if tau.shape != S.shape or tau.shape[0] != 6:
        raise Exception("the flux contraction takes two tensors of six fields (xx, yy, zz, xy, xz, yz), got %s and %s"
                        % (tuple(tau.shape), tuple(S.shape)))
    acc = tau[0] * S[0]
    acc += tau[1] * S[1]
    acc += tau[2] * S[2]
    for c in (3, 4, 5):
        acc += 2.0 * (tau[c] * S[c])
    return acc.neg_()


class WeightedVelocity(int):
    """The quantity code of the density-weighted velocity w = rho^alpha v (VPS_WEIGHTED_VELOCITY = 4) TOGETHER with its
    exponent: an int, so that it goes wherever a quantity code goes (int(q), the C calls), and the kernels
    wrapper hands `alpha` to the library (vps_set_density_weight) right before every call that forms the field -- the
    context's exponent is never what an earlier field left there."""

    def __new__(cls, alpha):
        alpha = float(alpha)
        if not np.isfinite(alpha):
            raise ValueError("density_weight must be a finite number, got %r" % (alpha,))
        self = super().__new__(cls, WEIGHTED)
        self.alpha = alpha
        return self

    # As a KEY the exponent counts: two weighted quantities are equal only when their exponents are, and none equals the
    # bare code 4 -- a table, set or cache keyed by quantity keeps rho^(1/3) v and rho^(1/2) v apart.  Code that asks "is
    # this the weighted quantity" compares int(q) == WEIGHTED.
    def __eq__(self, other):
        return isinstance(other, WeightedVelocity) and self.alpha == other.alpha

    def __ne__(self, other):
        return not self.__eq__(other)

    def __hash__(self):
        return hash((WEIGHTED, self.alpha))

    def __repr__(self):
        return "WeightedVelocity(alpha=%r)" % self.alpha


class Density(int):
    """The quantity code of the scalar s = rho^alpha (VPS_DENSITY = 5) TOGETHER with its exponent, built like WeightedVelocity:
    an int that goes wherever a quantity code goes, compares and hashes by its exponent, and whose `alpha` the kernels wrapper
    hands to the library right before every call that forms the field.  Density(1.0) is the plain density."""

    def __new__(cls, alpha=1.0):
        alpha = float(alpha)
        if not np.isfinite(alpha):
            raise ValueError("density_weight must be a finite number, got %r" % (alpha,))
        self = super().__new__(cls, DENSITY)
        self.alpha = alpha
        return self

    def __eq__(self, other):
        return isinstance(other, Density) and self.alpha == other.alpha

    def __ne__(self, other):
        return not self.__eq__(other)

    def __hash__(self):
        return hash((DENSITY, self.alpha))

    def __repr__(self):
        return "Density(alpha=%r)" % self.alpha


# names BoxField.spctrm / helmholtz_spctrm take for the density-weighted velocity with a fixed exponent
WEIGHT_SHORTHANDS = {"rho13_velocity": 1.0 / 3.0, "rho12_velocity": 0.5}
VECTOR_QUANTITIES = ("velocity", "momentum", "weighted_velocity") + tuple(WEIGHT_SHORTHANDS)


def resolve_quantity(quantity, density_weight=None, supported=None):
    """(name, code) of a quantity name of BoxField.spctrm: name is 'velocity' | 'momentum' | 'energy' | 'weighted_velocity' |
    'density' | 'log_density' | 'total_energy' | 'subgrid_energy' | 'dispersion' | 'subgrid_stress' | 'dispersion_tensor', code the library's (a WeightedVelocity /
    Density carrying alpha for those two).
    'weighted_velocity' needs density_weight = alpha (finite); 'rho13_velocity' / 'rho12_velocity' are alpha = 1/3 and 1/2;
    'density' is rho^alpha with density_weight = alpha, the plain density (alpha = 1) without; density_weight with any other
    name is an error.
    `supported` restricts the names (the Helmholtz decomposition: vector quantities)."""
    names = tuple(QUANTITY) + tuple(WEIGHT_SHORTHANDS)
    if supported is not None:
        names = tuple(n for n in names if n in supported)
    if not isinstance(quantity, str) or quantity not in names:
        raise Exception("""Unrecognized physical quantity name.
        Supported%s: %s.""" % ("" if supported is None else " here", ", ".join(repr(n) for n in names)))
    if quantity in WEIGHT_SHORTHANDS:
        if density_weight is not None:
            raise ValueError("density_weight is implied by %r (alpha = %g); pass it with 'weighted_velocity' only"
                             % (quantity, WEIGHT_SHORTHANDS[quantity]))
        return "weighted_velocity", WeightedVelocity(WEIGHT_SHORTHANDS[quantity])
    if quantity == "weighted_velocity":
        if density_weight is None:
            raise ValueError("quantity 'weighted_velocity' needs density_weight=alpha (w = rho^alpha v)")
        return quantity, WeightedVelocity(density_weight)
    if quantity == "density":
        return quantity, Density(1.0 if density_weight is None else density_weight)
    if density_weight is not None:
        raise ValueError("density_weight only goes with quantity 'weighted_velocity' or 'density', not %r" % (quantity,))
    return quantity, QUANTITY[quantity]


# --------------------------------------------------------------------------- #
# host-side tables for the binning kernel
# --------------------------------------------------------------------------- #
def k_axis(Lbox, Nsize):
    """2*pi*fftfreq(N, Lcell), as interp.py:1448-1449 / parallel_optimized.py:153-154."""
    Lcell = Lbox / float(Nsize)
    return 2 * np.pi * np.fft.fftfreq(Nsize, Lcell)


def bin_edges(kmin, kmax, spacing, flavour="library"):
    """Bin centres and edges with the reference's own numpy expressions:
    library -> np.arange (interp.py:1472-1473); script -> np.linspace with
    n_bins=int((kmax-kmin)/spacing)+1 (parallel_optimized.py:178-180)."""
    if flavour == "library":
        centers = np.arange(kmin, kmax + spacing, spacing)
        edges = np.arange(kmin - spacing / 2, kmax + 3 * spacing / 2, spacing)
    elif flavour == "script":
        n_bins = int((kmax - kmin) / spacing) + 1
        centers = np.linspace(kmin, kmax, n_bins)
        edges = np.linspace(kmin - spacing / 2, kmax + spacing / 2, n_bins + 1)
    else:
        raise Exception("flavour must be 'library' or 'script'")
    if len(edges) != len(centers) + 1:
        raise Exception("bin centres and edges are inconsistent (%d, %d)" % (len(centers), len(edges)))
    return centers, edges


ASSIGNMENT_ORDER = {"ngp": 1, "cic": 2, "tsc": 3}
FLAG_ASSIGN_MASK = 0x300      # include/vps_hip.h: VPS_FLAG_ASSIGN_MASK


def FLAG_ASSIGN(assignment):
    """VPS_FLAG_ASSIGN(order) of a mass assignment, the bits vps_deposit_field takes: 0 for "ngp", 0x100 for "cic", 0x200 for
    "tsc"; any other name is a ValueError.  For callers of the C entry point, who size the workspace themselves;
    `HipKernels.deposit_field` takes assignment= (it sizes the workspace from it) and refuses these bits in its flags=."""
    if not isinstance(assignment, str) or assignment not in ASSIGNMENT_ORDER:
        raise ValueError("assignment must be 'ngp', 'cic' or 'tsc', not %r" % (assignment,))
    return ((ASSIGNMENT_ORDER[assignment] - 1) & 3) << 8


def window_inv2_axis(Nsize, assignment):
    """1 / W(k)^2 of one axis for the mass-assignment window W(k) = sinc(pi k / (2 k_Nyquist))^p, p = 1 (NGP),
    2 (CIC), 3 (TSC), indexed like fftfreq (float32).  The three axis factors multiply."""
    p = ASSIGNMENT_ORDER[assignment]
    n = np.fft.fftfreq(Nsize, 1.0 / Nsize)          # integer mode numbers
    x = np.pi * n / Nsize
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(n == 0, 1.0, np.sin(x) / x)
    return (w ** (-2.0 * p)).astype(np.float32)


def x_max_ranks(Nsize):
    """Most slab ranks the binning x pass takes for N = Nsize (include/vps_hip.h: vps_fft_x_bin_chunk): a rank's segment of a
    received x line has N / ranks points, and the lines of N = 1024, 2048 and 4096 (64, 128 and 256 lanes per line) need
    segments of at least one point per lane -- 16 ranks.  Every other supported N takes any rank count that divides N / 2."""
    return 16 if int(Nsize) in (1024, 2048, 4096) else int(Nsize)


def sqrt_thresholds(edges):
    """thr[i] = smallest float64 t with sqrt(t) >= edges[i] (i < nbins) and
    thr[nbins] = smallest t with sqrt(t) > edges[nbins], so that comparing
    s = kx^2+ky^2+kz^2 against thr reproduces numpy.histogram's comparison of
    sqrt(s) against the edges (left-closed bins, last bin right-closed) bit for bit
    without a square root on the device."""
    e = np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        t = e * e
        t[e <= 0] = 0.0
        pos = e > 0
        lo = t.copy()
        # lower thresholds: walk down while the predecessor still satisfies sqrt >= e
        for _ in range(8):
            prev = np.nextafter(lo, -np.inf)
            ok = pos & (prev >= 0) & (np.sqrt(np.maximum(prev, 0)) >= e)
            if not ok.any():
                break
            lo = np.where(ok, prev, lo)
        for _ in range(8):
            bad = pos & (np.sqrt(lo) < e)
            if not bad.any():
                break
            lo = np.where(bad, np.nextafter(lo, np.inf), lo)
        # last edge: first t with sqrt(t) > e
        hi = lo[-1]
        while np.sqrt(hi) <= e[-1]:
            hi = np.nextafter(hi, np.inf)
        while hi > 0 and np.sqrt(np.nextafter(hi, -np.inf)) > e[-1]:
            hi = np.nextafter(hi, -np.inf)
    thr = lo.copy()
    thr[-1] = hi
    return thr


def binning_tables(axis, edges):
    """The arguments of vps_set_binning -- (N, fl(a*a) axis table, thresholds, first edge, 1 / spacing) -- for uniform
    `edges` on a lattice whose axis values are `axis`: k = 2 pi fftfreq(N, Lcell) for a spectrum (`k_axis`), the lag
    r = Lcell min(i, N - i) for a correlation function (`r_axis`).  The binning kernel does not care which."""
    axis = np.asarray(axis, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    spacing = (edges[-1] - edges[0]) / (len(edges) - 1)
    return (len(axis), axis * axis, sqrt_thresholds(edges), float(edges[0]), 1.0 / spacing)


def r_axis(Lbox, Nsize):
    """Lag of lattice index i along one axis of a periodic box, Lcell * min(i, N - i): even in i and non-decreasing on
    [0, N/2], like |k| of `k_axis` -- the mirrored shell decisions of the binning x pass hold for it unchanged."""
    Lcell = Lbox / float(Nsize)
    i = np.arange(int(Nsize))
    return Lcell * np.minimum(i, int(Nsize) - i).astype(np.float64)


def radial_edges(Lbox, Nsize, rmin=None, rmax=None, rres=None):
    """Uniform r edges rmin + j rres, j = 0 .. nb, the last one <= rmax.  Defaults rmin = 0, rres = Lcell, rmax = L/2: the
    edges j Lcell, j = 0 .. N/2, the same float64 products as the lattice lags -- the first bin [0, Lcell) holds r = 0 alone
    and the last is right-closed at L/2 (numpy.histogram's rule, `sqrt_thresholds`).  rmax up to sqrt(3) L/2 reaches every
    lattice point."""
    Lcell = Lbox / float(Nsize)
    rmin = 0.0 if rmin is None else float(rmin)
    rres = Lcell if rres is None else float(rres)
    rmax = Lcell * (int(Nsize) // 2) if rmax is None else float(rmax)
    if not (rres > 0 and rmin >= 0 and rmax > rmin):
        raise ValueError("need 0 <= rmin < rmax and rres > 0 (got %r, %r, %r)" % (rmin, rmax, rres))
    nb = int(np.floor((rmax - rmin) / rres + 1e-9))
    if nb < 1:
        raise ValueError("rres = %r leaves no bin between rmin = %r and rmax = %r" % (rres, rmin, rmax))
    return rmin + rres * np.arange(nb + 1)


# --------------------------------------------------------------------------- #
# kernel set backed by libvps_hip.so
# --------------------------------------------------------------------------- #
class HipKernels:
    """Thin typed wrapper of the C ABI working on torch CUDA tensors."""

    name = "hip"

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise _ffi.VpsError("no HIP device is visible to this process; the vpower device path "
                                "needs an MI355X (there is no CPU fallback)")
        self.lib = _ffi.lib()
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device if isinstance(device, int) else device.index)
        h = C.c_void_p()
        rc = self.lib.vps_create(C.byref(h), self.device.index)
        if rc != 0:
            raise _ffi.VpsError("vps_create failed (%d): %s" % (rc, self.lib.vps_last_error(None).decode()))
        self.ctx = h
        self._work = {}
        info = (C.c_int64 * 4)()
        self._chk(self.lib.vps_device_info(self.ctx, info))
        self.num_cu, self.lds_per_cu, self.wave, self.hbm_mib = (int(x) for x in info)
        self.hist_max_bins = int(self.lib.vps_hist_max_bins(self.ctx))

    def device_info(self):
        """Device facts the host side sizes things by (vps_device_info, vps_hist_max_bins)."""
        return {"num_cu": self.num_cu, "lds_per_cu": self.lds_per_cu, "wave": self.wave, "hbm_mib": self.hbm_mib,
                "hist_max_bins": self.hist_max_bins}

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.vps_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing -------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise _ffi.VpsError("libvps_hip call failed (%d): %s" % (rc, self.lib.vps_last_error(self.ctx).decode()))

    def _stream(self):
        self._chk(self.lib.vps_set_stream(self.ctx, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _ptr(self, t, dtype=None):
        if t is None:
            return None
        if not t.is_cuda or t.device != self.device:
            raise _ffi.VpsError("tensor must live on %s (got %s)" % (self.device, t.device))
        if not t.is_contiguous():
            raise _ffi.VpsError("tensor must be contiguous")
        if dtype is not None and t.dtype != dtype:
            raise _ffi.VpsError("tensor must be %s (got %s)" % (dtype, t.dtype))
        return C.c_void_p(t.data_ptr())

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    h2d_copies = 0      # host -> device uploads made through to_device (tests assert residency with it)
    h2d_bytes = 0

    def to_device(self, arr, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(arr))
        if dtype is not None:
            t = t.to(dtype)
        self.h2d_copies += 1
        self.h2d_bytes += t.numel() * t.element_size()
        return t.to(self.device)

    def workspace(self, key, nbytes):
        w = self._work.get(key)
        if w is None or w.numel() < nbytes:
            self._work[key] = None
            w = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            self._work[key] = w
        return w

    def sync(self):
        self._chk(self.lib.vps_sync(self.ctx))

    # -- timing ---------------------------------------------------------------
    def timing(self, on):
        self._chk(self.lib.vps_timing_enable(self.ctx, 1 if on else 0))
        self._chk(self.lib.vps_timing_reset(self.ctx))

    def timing_get(self):
        out = {}
        for name, kind in _ffi.KERNEL_KINDS.items():
            n, ms = C.c_int64(), C.c_double()
            self._chk(self.lib.vps_timing_get(self.ctx, kind, C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out

    def timing_list(self, name):
        kind = _ffi.KERNEL_KINDS[name]
        n = C.c_int64()
        self._chk(self.lib.vps_timing_list(self.ctx, kind, None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), dtype=np.float64)
        self._chk(self.lib.vps_timing_list(self.ctx, kind, _ffi.as_dp(buf), n.value, C.byref(n)))
        return buf[: n.value]

    # -- stage A --------------------------------------------------------------
    def preprocess(self, pos, vel, mass, shift_to_origin=True, remove_bulk_velocity=True):
        """In place: shift positions to the origin, remove the mass-weighted bulk velocity.
        Returns (min[3], bulk[3]) that were subtracted."""
        self._stream()
        mn, bv = np.zeros(3), np.zeros(3)
        self._chk(self.lib.vps_preprocess(self.ctx, self._ptr(pos), self._pos_kind(pos),
                                          self._ptr(vel, torch.float32) if vel is not None else None,
                                          self._ptr(mass, torch.float32) if mass is not None else None,
                                          pos.shape[0], 1 if shift_to_origin else 0,
                                          1 if remove_bulk_velocity else 0, _ffi.as_dp(mn), _ffi.as_dp(bv)))
        return mn, bv

    def totals(self, v, mass, elem_stride, comp_stride, n):
        """float64 [sum m, sum m vx, sum m vy, sum m vz, sum m |v|^2] (vps_totals)."""
        self._stream()
        out = np.zeros(5)
        self._chk(self.lib.vps_totals(self.ctx, self._ptr(v, torch.float32), int(elem_stride), int(comp_stride),
                                      self._ptr(mass, torch.float32), int(n), _ffi.as_dp(out)))
        return out

    def particle_totals(self, vel, mass):
        return self.totals(vel, mass, 3, 1, vel.shape[0])

    def field_totals(self, chans):
        """chans [4, ...] = vx, vy, vz, mass of a gridded field."""
        n = chans[0].numel()
        return self.totals(chans, chans[3], 1, n, n)

    @staticmethod
    def _pos_kind(pos):
        if pos.dtype == torch.float32:
            return 0
        if pos.dtype == torch.float64:
            return 1
        raise _ffi.VpsError("positions must be float32 or float64")

    def cell_index(self, pos, N, Lbox):
        self._stream()
        out = self.empty((pos.shape[0], 3), torch.int32)
        self._chk(self.lib.vps_cell_index(self.ctx, self._ptr(pos), self._pos_kind(pos), pos.shape[0], N,
                                          float(Lbox), self._ptr(out)))
        return out

    def density_velocity_vector(self, vel, rho):
        self._stream()
        out = self.empty((vel.shape[0], 4), torch.float32)
        self._chk(self.lib.vps_density_velocity_vector(self.ctx, self._ptr(vel, torch.float32),
                                                       self._ptr(rho, torch.float32), vel.shape[0],
                                                       self._ptr(out)))
        return out

    def deposit(self, pos, payload, N, Lbox, x0, nx, out=None):
        """payload [np, C] float32 -> grid [C, nx, N, N] float32 (every cell written)."""
        self._stream()
        C_ = payload.shape[1]
        if out is None:
            out = self.empty((C_, nx, N, N), torch.float32)
        work = self.workspace("deposit", self.lib.vps_deposit_workspace_bytes(pos.shape[0], C_, N, nx))
        self._chk(self.lib.vps_deposit_ngp(self.ctx, self._ptr(pos), self._pos_kind(pos),
                                           self._ptr(payload, torch.float32), pos.shape[0], C_, N,
                                           float(Lbox), x0, nx, self._ptr(out, torch.float32), self._ptr(work)))
        return out

    def _set_weight(self, quantity):
        """Before a call that forms the fields of `quantity`: a weighted quantity's exponent goes to the context NOW."""
        if int(quantity) in (WEIGHTED, DENSITY):
            alpha = getattr(quantity, "alpha", None)
            if alpha is None:
                raise Exception("the density-weighted velocity needs its exponent: pass device.WeightedVelocity(alpha)"
                                if int(quantity) == WEIGHTED else
                                "the density power rho^alpha needs its exponent: pass device.Density(alpha)")
            self._chk(self.lib.vps_set_density_weight(self.ctx, float(alpha)))
        return int(quantity)

    def deposit_field(self, pos, vel, rho, N, Lbox, x0, nx, quantity, flags=0, out=None, assignment="ngp"):
        """Fused deposit of [rho v, rho] + field algebra -> [ncomp, nx, N, N] float32.  assignment = "cic" / "tsc": the same
        fields of the CIC / TSC cell totals on the slab (VPS_FLAG_ASSIGN: one sort record per particle, the quantity formed in
        the owner brick's epilogue), from a workspace of its own sized by vps_deposit_assign_workspace_bytes.
        TOTAL_ENERGY / SUBGRID_ENERGY / DISPERSION -> [1, nx, N, N]: the scalars of the cell's second moment
        sum w rho_p |v_p|^2 (a fifth channel of the brick's LDS tile; the same records and workspaces), with every assignment.
        SUBGRID_STRESS / DISPERSION_TENSOR -> [6, nx, N, N]: the components xx, yy, zz, xy, xz, yz of that second moment as a
        tensor (one sort, two accumulation launches with three second-moment tile channels each; the same workspaces)."""
        assign = FLAG_ASSIGN(assignment)
        if int(flags) & FLAG_ASSIGN_MASK:
            # (the workspace below is sized from `assignment`: bits arriving in `flags` would run CIC / TSC in the NGP workspace)
            raise ValueError("deposit_field: pass the mass assignment as assignment='cic' | 'tsc', not as FLAG_ASSIGN bits in flags "
                             "(flags 0x%x)" % int(flags))
        self._stream()
        quantity = self._set_weight(quantity)
        ncomp = NCOMP[quantity]
        if out is None:
            out = self.empty((ncomp, nx, N, N), torch.float32)
        if assign:
            flags = int(flags) | assign
            work = self.workspace("deposit_field_assign", self.lib.vps_deposit_assign_workspace_bytes(
                pos.shape[0], 4, int(N), ASSIGNMENT_ORDER[assignment]))
        else:
            work = self.workspace("deposit", self.lib.vps_deposit_workspace_bytes(pos.shape[0], 4, N, nx))
        self._chk(self.lib.vps_deposit_field(self.ctx, self._ptr(pos), self._pos_kind(pos),
                                             self._ptr(vel, torch.float32), self._ptr(rho, torch.float32),
                                             pos.shape[0], N, float(Lbox), x0, nx, quantity, flags,
                                             self._ptr(out, torch.float32), self._ptr(work)))
        return out

    def fused_supported(self, N, quantity):
        return bool(self.lib.vps_deposit_fft_zy_supported(self.ctx, int(N), int(quantity)))

    def deposit_fft_zy(self, pos, vel, rho, N, Lbox, x0, nx, quantity, flags=0, spec=None, nyq=None, reuse_sort=None,
                       component=None, share_energy=False):
        """Fused deposit + field algebra + z/y passes:
        -> spec [ncomp, N/2, N, nx], nyq [ncomp, N, nx] (complex64); ncomp = 1 for ENERGY, else 3.
        component = 0..2, or a collection of them: only those components of a velocity / momentum field, in ascending order
        (ncomp = their number; VPS_FLAG_COMPONENTS).
        share_energy (pass it on EVERY call of a step that asks for momentum and, later, kinetic energy): the workspace gets room
        for a fourth z image; the momentum launch -- whose rounds accumulate the very cell totals of rho v_c the energy field is
        made of -- leaves that field's z image there as well (VPS_FLAG_SHARE_ENERGY), and the energy call that follows it with a
        valid reuse_sort token only runs its y pass.  Any other order of calls simply launches the energy kernel as usual."""
        self._stream()
        quantity = self._set_weight(quantity)
        ncomp = NCOMP[quantity]
        if component is not None:
            mask = self._component_mask(quantity, component)
            flags |= mask << 4
            ncomp = bin(mask).count("1")
        if spec is None:
            spec = self.empty((ncomp, N // 2, N, nx), torch.complex64)
        if nyq is None:
            nyq = self.empty((ncomp, N, nx), torch.complex64)
        size_of = self.lib.vps_deposit_fft_zy_workspace_bytes_shared if share_energy else self.lib.vps_deposit_fft_zy_workspace_bytes
        work = self.workspace("fused", size_of(pos.shape[0], N, nx))
        flags |= self._reuse_flag(reuse_sort, pos, vel, rho, N, Lbox, x0, nx, work)
        shared_by = getattr(self, "_energy_shared_by", None)     # token of the momentum call that left the energy z image behind
        self._energy_shared_by = None
        if share_energy and component is None:
            if quantity == MOMENTUM and not (flags & FLAG_REFERENCE_MOMENTUM_BUG):
                flags |= FLAG_SHARE_ENERGY
                self._energy_shared_by = self._fused_token
            elif quantity == ENERGY and (flags & FLAG_REUSE_SORT) and shared_by is not None and reuse_sort is shared_by:
                flags |= FLAG_SHARE_ENERGY
        self._chk(self.lib.vps_deposit_fft_zy(self.ctx, self._ptr(pos), self._pos_kind(pos),
                                              self._ptr(vel, torch.float32), self._ptr(rho, torch.float32),
                                              pos.shape[0], N, float(Lbox), x0, nx, quantity, flags,
                                              self._ptr(spec), self._ptr(nyq), self._ptr(work)))
        return spec, nyq

    def share_energy_fits(self, N, nx):
        """True where the fourth z image of share_energy (4 N^2 nx bytes more: 29 N^2 nx bytes in all for a step with
        three-component quantities) still leaves a tenth of the device free."""
        total = torch.cuda.get_device_properties(self.device).total_memory
        return 30.5 * float(N) ** 2 * nx < 0.88 * total

    @staticmethod
    def _component_mask(quantity, component):
        """component: 0..2 or a collection of them -> the bit mask of VPS_FLAG_COMPONENTS."""
        comps = (component,) if isinstance(component, (int, np.integer)) else tuple(component)
        if NCOMP[int(quantity)] == 1 or not comps or any(not 0 <= int(c) <= 2 for c in comps) or len(set(comps)) != len(comps):
            raise Exception("component(s) = distinct values 0..2 of a velocity, momentum or weighted-velocity field")
        mask = 0
        for c in comps:
            mask |= 1 << int(c)
        return mask

    def _reuse_flag(self, reuse_sort, pos, vel, rho, N, Lbox, x0, nx, work, cap=None):
        """FLAG_REUSE_SORT if `reuse_sort` (a token returned by an earlier fused call) proves that the bucketed records
        of that call are still in `work`: several quantities of the SAME particle tensors then sort only once.  The
        token holds WEAK references to the tensors (a freed tensor whose address is recycled cannot pass for the old
        one, and nothing is kept alive by the library) and their in-place modification counters; any mismatch silently
        sorts again.  Records the token of THIS call."""
        # (the library options that decide the record layout are part of the state: a sort made under one value of
        #  sort_atomic / sort_staged / sort_groups cannot be reused under another)
        layout_opts = tuple(sorted((k, v) for k, v in _ffi.OPTIONS.items() if k.startswith("sort_")))
        state = (weakref.ref(pos), weakref.ref(vel), weakref.ref(rho), pos._version, vel._version, rho._version,
                 int(N), float(Lbox), int(x0), int(nx), work.data_ptr(), cap, layout_opts)
        last = getattr(self, "_fused_token", None)
        ok = (reuse_sort is not None and reuse_sort is last
              and all(r() is t for r, t in zip(last[:3], (pos, vel, rho))) and last[3:] == state[3:])
        self._fused_token = state
        return FLAG_REUSE_SORT if ok else 0

    def fused_token(self):
        """Token of the last deposit_fft_zy call (pass it as reuse_sort= to the next one)."""
        return getattr(self, "_fused_token", None)

    def nn_resample(self, pos, payload, axes, x0, nx, want_index=False, out=None):
        """Exact NN of every lattice point axes[0][x0:x0+nx] x axes[1] x axes[2]."""
        self._stream()
        ax = [np.ascontiguousarray(a, dtype=np.float64) for a in axes]
        C_ = payload.shape[1]
        if out is None:
            out = self.empty((C_, nx, len(ax[1]), len(ax[2])), torch.float32)
        idx = self.empty((nx, len(ax[1]), len(ax[2])), torch.int32) if want_index else None
        kind = self._pos_kind(pos)
        work = self.workspace("nn", self.lib.vps_nn_workspace_bytes(pos.shape[0], kind, nx * len(ax[1]) * len(ax[2])))
        self._chk(self.lib.vps_nn_resample(self.ctx, self._ptr(pos), kind, self._ptr(payload, torch.float32),
                                           pos.shape[0], C_, _ffi.as_dp(ax[0]), len(ax[0]),
                                           _ffi.as_dp(ax[1]), len(ax[1]), _ffi.as_dp(ax[2]), len(ax[2]),
                                           x0, nx, self._ptr(out), self._ptr(idx), self._ptr(work)))
        return out, idx

    def nn_plan(self, np_, pos_is_f64=False, nq_slab=0):
        """The cell-list geometry of a search over np_ particles under the current options (nn_plan below; nothing runs)."""
        return nn_plan(np_, pos_is_f64, nq_slab)

    def nn_last_search(self):
        """What the last nn_resample* call of this context ran (vps_nn_last_search): {"kind": "ring" | "scatter" | "column" (None:
        no search yet), "tiles": workgroups of the search kernel, "radii": per-tile radii precomputed, "open": lattice points left
        to the exact fallback (read back only under the option nn_stats or timing; else -1)}."""
        out = (C.c_int64 * len(_ffi.NN_LAST_SEARCH_FIELDS))()
        self._chk(self.lib.vps_nn_last_search(self.ctx, out))
        d = dict(zip(_ffi.NN_LAST_SEARCH_FIELDS, (int(v) for v in out)))
        d["kind"] = _ffi.NN_SEARCH_KINDS[d["kind"]] if d["kind"] >= 0 else None
        return d

    def nn_resample_field(self, pos, rhov, axes, x0, nx, Lcell, out=None, want_index=False):
        """Exact-NN resampling of [rho v, rho] with v = rho v / rho, mass = rho Lcell^3 formed in the search's
        epilogue: -> [4, nx, ny, nz] float32 = vx, vy, vz, mass (interp.py:246-277 without a pass over the grid)."""
        self._stream()
        ax = [np.ascontiguousarray(a, dtype=np.float64) for a in axes]
        if out is None:
            out = self.empty((4, nx, len(ax[1]), len(ax[2])), torch.float32)
        idx = self.empty((nx, len(ax[1]), len(ax[2])), torch.int32) if want_index else None
        kind = self._pos_kind(pos)
        work = self.workspace("nn", self.lib.vps_nn_workspace_bytes(pos.shape[0], kind, nx * len(ax[1]) * len(ax[2])))
        self._chk(self.lib.vps_nn_resample_field(self.ctx, self._ptr(pos), kind, self._ptr(rhov, torch.float32),
                                                 pos.shape[0], _ffi.as_dp(ax[0]), len(ax[0]), _ffi.as_dp(ax[1]), len(ax[1]),
                                                 _ffi.as_dp(ax[2]), len(ax[2]), x0, nx, float(Lcell), self._ptr(out),
                                                 self._ptr(idx), self._ptr(work)))
        return out, idx

    def nn_resample_quantity(self, pos, rhov, axes, x0, nx, Lcell, quantity, flags=0, out=None, want_index=False):
        """Exact-NN resampling of [rho v, rho] straight into the fields the spectrum of `quantity` transforms
        (vps_nn_resample_quantity): VELOCITY -> [3, ...] v; MOMENTUM -> [3, ...] p = v * mass; ENERGY -> [1, ...] mass |v|^2;
        VM -> [4, ...] (= nn_resample_field); a WeightedVelocity -> [3, ...] rho^alpha v of the nearest particle."""
        self._stream()
        quantity = self._set_weight(quantity)
        ax = [np.ascontiguousarray(a, dtype=np.float64) for a in axes]
        nout = NCOMP[quantity]
        if out is None:
            out = self.empty((nout, nx, len(ax[1]), len(ax[2])), torch.float32)
        idx = self.empty((nx, len(ax[1]), len(ax[2])), torch.int32) if want_index else None
        kind = self._pos_kind(pos)
        work = self.workspace("nn", self.lib.vps_nn_workspace_bytes(pos.shape[0], kind, nx * len(ax[1]) * len(ax[2])))
        self._chk(self.lib.vps_nn_resample_quantity(self.ctx, self._ptr(pos), kind, self._ptr(rhov, torch.float32),
                                                    pos.shape[0], _ffi.as_dp(ax[0]), len(ax[0]), _ffi.as_dp(ax[1]), len(ax[1]),
                                                    _ffi.as_dp(ax[2]), len(ax[2]), x0, nx, float(Lcell), int(quantity), int(flags),
                                                    self._ptr(out), self._ptr(idx), self._ptr(work)))
        return out, idx

    def field_algebra(self, chans, quantity, flags, Lcell):
        self._stream()
        ncell = chans[0].numel()
        quantity = self._set_weight(quantity)
        self._chk(self.lib.vps_field_algebra(self.ctx, quantity, flags, float(Lcell),
                                             self._ptr(chans, torch.float32), ncell))

    def field_algebra_out(self, chans, quantity, flags, Lcell):
        """Fields of `quantity` from the four channels, which are left untouched: -> [3 | 1 | 4, ...] float32."""
        self._stream()
        ncell = chans[0].numel()
        quantity = self._set_weight(quantity)
        nout = NCOMP[quantity]
        out = self.empty((nout,) + tuple(chans.shape[1:]), torch.float32)
        self._chk(self.lib.vps_field_algebra_out(self.ctx, quantity, flags, float(Lcell),
                                                 self._ptr(chans, torch.float32), ncell, self._ptr(out)))
        return out

    def velocity_gradient(self, chans, N, Lcell, what, out=None):
        """Central-difference fields of the velocity of a whole periodic grid (vps_field_algebra_out, csrc/gradient.hip): chans
        [4, N, N, N] float32 = vx, vy, vz, mass (the mass is not read), `what` 'divergence' | 'vorticity' | 'strain_rate' or its
        code -> [1 | 3 | 6, N, N, N] float32 (vorticity x, y, z; strain rate xx, yy, zz, xy, xz, yz), d_a u_c =
        (u_c(i + e_a) - u_c(i - e_a)) / (2 Lcell) with every index wrapped.  `out`: a tensor of that shape to write into; it must
        not overlap `chans`."""
        code = GRADIENT_QUANTITIES.get(what, what) if isinstance(what, str) else int(what)
        if code not in GRADIENT_QUANTITIES.values():
            raise ValueError("velocity_gradient forms %s, not %r" % (" | ".join(repr(n) for n in GRADIENT_QUANTITIES), what))
        N = int(N)
        if tuple(chans.shape) != (4, N, N, N):
            raise ValueError("velocity_gradient needs the [4, N, N, N] channels of a whole grid, got %s for N = %d"
                             % (tuple(chans.shape), N))
        self._stream()
        shape = (NCOMP[code], N, N, N)
        if out is None:
            out = self.empty(shape, torch.float32)
        elif tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("velocity_gradient: out must be a contiguous %s tensor" % (shape,))
        self._chk(self.lib.vps_field_algebra_out(self.ctx, code, FLAG_INPUT_IS_VM, float(Lcell),
                                                 self._ptr(chans, torch.float32), N ** 3, self._ptr(out, torch.float32)))
        return out

    def box_filter(self, chans, N, half_width, what="vm", out=None):
        """Mass-weighted box filter of a whole periodic grid (vps_field_algebra_out, csrc/filter.hip): chans [4, N, N, N] float32 =
        vx, vy, vz, mass, a box of (2 half_width + 1)^3 cells around every cell, every index wrapped.  what 'vm' (or 16) ->
        [4, N, N, N]: the Favre-filtered velocity sum(mass v) / sum(mass) (0 where the box holds no mass) and the filtered mass
        sum(mass) / (2m+1)^3, again [v, mass] channels; 'stress' (or 17) -> [6, N, N, N]: the sub-filter stress
        (sum(mass v_i v_j) - sum(mass v_i) sum(mass v_j) / sum(mass)) / (2m+1)^3 in the order xx, yy, zz, xy, xz, yz.  `out`: a
        tensor of that shape to write into; it must not overlap `chans`."""
        code = FILTER_QUANTITIES.get(what, what) if isinstance(what, str) else int(what)
        if code not in FILTER_QUANTITIES.values():
            raise ValueError("box_filter forms %s, not %r" % (" | ".join(repr(n) for n in FILTER_QUANTITIES), what))
        N = int(N)
        if tuple(chans.shape) != (4, N, N, N):
            raise ValueError("box_filter needs the [4, N, N, N] channels of a whole grid, got %s for N = %d"
                             % (tuple(chans.shape), N))
        if N < 4 or N % 2:
            raise ValueError("box_filter needs an even N >= 4, got %d" % N)
        if half_width != int(half_width) or not 1 <= int(half_width) <= FILTER_MAX_HALF_WIDTH:
            raise ValueError("box_filter: the half-width is a whole number of cells from 1 to %d, got %r"
                             % (FILTER_MAX_HALF_WIDTH, half_width))
        m = int(half_width)
        if 2 * m + 1 > N:
            raise ValueError("box_filter: the box of 2 * %d + 1 cells is wider than the grid (N = %d)" % (m, N))
        self._stream()
        shape = (NCOMP[code], N, N, N)
        if out is None:
            out = self.empty(shape, torch.float32)
        elif tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError("box_filter: out must be a contiguous %s tensor" % (shape,))
        self._chk(self.lib.vps_field_algebra_out(self.ctx, code, FLAG_INPUT_IS_VM | FLAG_FILTER(m), 1.0,
                                                 self._ptr(chans, torch.float32), N ** 3, self._ptr(out, torch.float32)))
        return out

    # -- stage B + C ------------------------------------------------------------
    def fft_supported(self, N):
        return bool(self.lib.vps_fft_supported(int(N)))

    def set_binning(self, N, k2, thr, edge0, inv_spacing):
        k2 = np.ascontiguousarray(k2, dtype=np.float64)
        thr = np.ascontiguousarray(thr, dtype=np.float64)
        self._stream()
        self._chk(self.lib.vps_set_binning(self.ctx, N, _ffi.as_dp(k2), _ffi.as_dp(thr), len(thr) - 1,
                                           float(edge0), float(inv_spacing)))

    def binning_mode(self):
        """How the binning x pass decides shells for the tables set last (vps_binning_mode): 0 general shell walk, 1 mirrored kx
        with float64 k^2 sums, 2 mirrored kx with integer ix^2 + iy^2 + iz^2 (the same shells, checked by vps_set_binning)."""
        return int(self.lib.vps_binning_mode(self.ctx))

    def binning_only(self):
        """Context manager: inside it the y passes skip rows whose modes all lie beyond the last shell edge of the
        binning tables set last (vps_set_bin_only) -- for outputs that go straight into the binning x pass."""
        k = self

        class _Scope:
            def __enter__(self_inner):
                k._chk(k.lib.vps_set_bin_only(k.ctx, 1))

            def __exit__(self_inner, *exc):
                k._chk(k.lib.vps_set_bin_only(k.ctx, 0))
                return False
        return _Scope()

    def set_window(self, N, table):
        """1/W^2 axis table (window_inv2_axis) for the binning x pass, or None to switch deconvolution off."""
        self._stream()
        if table is None:
            self._chk(self.lib.vps_set_window(self.ctx, int(N), None))
            return
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.shape != (N,):
            raise _ffi.VpsError("window table must have N entries")
        self._chk(self.lib.vps_set_window(self.ctx, int(N), t.ctypes.data_as(C.c_void_p)))

    def assign_expand(self, pos, payload, N, Lbox, assignment):
        """CIC / TSC: (pos [np,3], payload [np,C]) -> weighted sub-particles at cell centres
        (pos' float32 [np*S,3], payload' [np*S,C]); deposit them with `deposit`."""
        self._stream()
        order = ASSIGNMENT_ORDER[assignment]
        if order == 1:
            return pos, payload
        S = order ** 3
        n, C_ = payload.shape
        pos_o = self.empty((n * S, 3), torch.float32)
        pay_o = self.empty((n * S, C_), torch.float32)
        self._chk(self.lib.vps_assign_expand(self.ctx, self._ptr(pos), self._pos_kind(pos), self._ptr(payload, torch.float32),
                                             n, C_, int(N), float(Lbox), order, self._ptr(pos_o), self._ptr(pay_o)))
        return pos_o, pay_o

    def deposit_assign(self, pos, payload, N, Lbox, assignment, out=None):
        """CIC / TSC without the expansion (vps_deposit_assign): (pos [np,3], payload [np,C] float32, C in 1, 3, 4) -> the whole
        grid [C, N, N, N] float32, every cell written; one sort record per particle, each brick gathers from its own and its
        lower neighbours' buckets.  `assignment` = "ngp" is `deposit` on the whole grid."""
        order = ASSIGNMENT_ORDER[assignment]
        if order == 1:
            return self.deposit(pos, payload, N, Lbox, 0, N, out=out)
        self._stream()
        n, C_ = payload.shape
        if out is None:
            out = self.empty((C_, N, N, N), torch.float32)
        work = self.workspace("deposit_assign", self.lib.vps_deposit_assign_workspace_bytes(n, C_, int(N), order))
        self._chk(self.lib.vps_deposit_assign(self.ctx, self._ptr(pos), self._pos_kind(pos), self._ptr(payload, torch.float32),
                                              n, C_, int(N), float(Lbox), order, self._ptr(out, torch.float32), self._ptr(work)))
        return out

    def deposit_assign_plan(self, np_, C_, N, assignment):
        """Brick geometry and sort path of deposit_assign for np_ particles with C_ channels under the current options
        (vps_deposit_assign_plan; nothing runs): {field: int} over _ffi.DEPOSIT_ASSIGN_PLAN_FIELDS."""
        out = (C.c_int64 * len(_ffi.DEPOSIT_ASSIGN_PLAN_FIELDS))()
        self._chk(self.lib.vps_deposit_assign_plan(self.ctx, int(np_), int(C_), int(N), ASSIGNMENT_ORDER[assignment], out))
        return dict(zip(_ffi.DEPOSIT_ASSIGN_PLAN_FIELDS, (int(v) for v in out)))

    def fft_zy(self, field, N, nx, spec=None, nyq=None, weight=None):
        """field [nx,N,N] float32 (times `weight`, same shape, if given) -> spec [N/2,N,nx], nyq [N,nx] (complex64)."""
        self._stream()
        if spec is None:
            spec = self.empty((N // 2, N, nx), torch.complex64)
        if nyq is None:
            nyq = self.empty((N, nx), torch.complex64)
        work = self.workspace("fft", self.lib.vps_fft_workspace_bytes(N, nx))
        self._chk(self.lib.vps_fft_zy_weighted(self.ctx, N, nx, self._ptr(field, torch.float32),
                                               self._ptr(weight, torch.float32), self._ptr(spec), self._ptr(nyq),
                                               self._ptr(work)))
        return spec, nyq

    # -- split form for the chunked slab exchange --------------------------------
    def zimage_elems(self, N, nx):
        return int(self.lib.vps_fft_zimage_bytes(int(N), int(nx))) // 8

    def fft_z(self, field, N, nx, weight=None, zimg=None):
        """z pass only: field [nx,N,N] float32 (* weight) -> z image (flat complex64: B[x][kz][y] | BN[x][y])."""
        self._stream()
        if zimg is None:
            zimg = self.empty((self.zimage_elems(N, nx),), torch.complex64)
        self._chk(self.lib.vps_fft_z(self.ctx, N, nx, self._ptr(field, torch.float32), self._ptr(weight, torch.float32),
                                     self._ptr(zimg, torch.complex64)))
        return zimg

    def count_in_slab(self, pos, N, Lbox, x0, nx):
        """Particles whose (bit-exact) cell lies in the x-slab [x0, x0 + nx) (vps_count_in_slab)."""
        self._stream()
        n = int(self.lib.vps_count_in_slab(self.ctx, self._ptr(pos), self._pos_kind(pos), pos.shape[0], int(N), float(Lbox),
                                           int(x0), int(nx)))
        if n < 0:
            self._chk(n)
        return n

    def deposit_plan(self, np_, C_, N, x0, nx, pencil=False, slab_particles=None):
        """What the bucket sort of a deposit of np_ particles with C_ channels on the slab would do under the current options
        (vps_deposit_plan; nothing runs): {field: int} over _ffi.DEPOSIT_PLAN_FIELDS.  pencil: the buckets of the fused route
        (C_ = 4) instead of the bricks of deposit / deposit_field; slab_particles: as in deposit_fft_z."""
        out = (C.c_int64 * len(_ffi.DEPOSIT_PLAN_FIELDS))()
        self._chk(self.lib.vps_deposit_plan(self.ctx, int(np_), int(C_), int(N), int(x0), int(nx), 1 if pencil else 0,
                                            -1 if slab_particles is None else int(slab_particles), out))
        return dict(zip(_ffi.DEPOSIT_PLAN_FIELDS, (int(v) for v in out)))

    def deposit_fft_z(self, pos, vel, rho, N, Lbox, x0, nx, quantity, flags=0, zimg=None, reuse_sort=None, slab_particles=None,
                      component=None):
        """Fused deposit + field algebra + z pass -> z images [ncomp, zimage_elems] (ncomp = 1 for ENERGY, else 3;
        a WeightedVelocity is a three-component quantity like VELOCITY).
        slab_particles: a bound on the particles inside the slab (count_in_slab): the sort workspace is then sized for it,
        not for all of a replicated particle set.  component: as in deposit_fft_zy."""
        self._stream()
        quantity = self._set_weight(quantity)
        ncomp = NCOMP[quantity]
        if component is not None:
            mask = self._component_mask(quantity, component)
            flags |= mask << 4
            ncomp = bin(mask).count("1")
        if zimg is None:
            zimg = self.empty((ncomp, self.zimage_elems(N, nx)), torch.complex64)
        if slab_particles is None:
            work = self.workspace("fused_z", self.lib.vps_deposit_fft_z_workspace_bytes(pos.shape[0], N, nx))
        else:
            work = self.workspace("fused_z", self.lib.vps_deposit_fft_z_workspace_bytes_slab(pos.shape[0], int(slab_particles), N, nx))
        flags |= self._reuse_flag(reuse_sort, pos, vel, rho, N, Lbox, x0, nx, work, slab_particles)
        if slab_particles is None:
            self._chk(self.lib.vps_deposit_fft_z(self.ctx, self._ptr(pos), self._pos_kind(pos),
                                                 self._ptr(vel, torch.float32), self._ptr(rho, torch.float32),
                                                 pos.shape[0], N, float(Lbox), x0, nx, quantity, flags,
                                                 self._ptr(zimg, torch.complex64), self._ptr(work)))
        else:
            self._chk(self.lib.vps_deposit_fft_z_slab(self.ctx, self._ptr(pos), self._pos_kind(pos),
                                                      self._ptr(vel, torch.float32), self._ptr(rho, torch.float32),
                                                      pos.shape[0], int(slab_particles), N, float(Lbox), x0, nx, quantity, flags,
                                                      self._ptr(zimg, torch.complex64), self._ptr(work)))
        return zimg

    def y_chunk_elems(self, N, nx, G, nchunks, chunk):
        n = int(self.lib.vps_fft_y_chunk_elems(int(N), int(nx), int(G), int(nchunks), int(chunk)))
        if n < 0:
            raise _ffi.VpsError("%d ranks x %d chunks do not divide N/2 = %d" % (G, nchunks, N // 2))
        return n

    def y_packed(self, N):
        """True when fft_y_chunk packs rows now: inside a `binning_only` scope whose tables have a row cut for N."""
        return bool(self.lib.vps_fft_y_packed(self.ctx, int(N)))

    def chunk_block(self, N, nx, G, nchunks, chunk, packed):
        """Elements of ONE destination's block of chunk `chunk` (include/vps_hip.h: vps_fft_y)."""
        n = int(self.lib.vps_fft_y_chunk_block(self.ctx, int(N), int(nx), int(G), int(nchunks), int(chunk), int(bool(packed))))
        if n < 0:
            why = self.lib.vps_last_error(self.ctx).decode() if n < -1 else "bad arguments"
            raise _ffi.VpsError("vps_fft_y_chunk_block(N=%d, nx=%d, G=%d, nchunks=%d, chunk=%d, packed=%d) failed (%d): %s"
                                % (N, nx, G, nchunks, chunk, bool(packed), n, why))
        return n

    def fft_y_chunk(self, zimg, N, nx, G, nchunks, chunk, out=None):
        """y pass of one kz chunk of a z image -> the send buffer of an equal-split all-to-all over G ranks:
        [h][ F_zy[kz in h's planes of the chunk][row][x] | (last chunk) Nyquist rows of h ] (flat complex64),
        G * chunk_block(..., packed=y_packed(N)) elements (ask in the same scope)."""
        self._stream()
        n = G * self.chunk_block(N, nx, G, nchunks, chunk, self.y_packed(N))
        if out is None:
            out = self.empty((n,), torch.complex64)
        self._chk(self.lib.vps_fft_y(self.ctx, N, nx, self._ptr(zimg, torch.complex64), G, nchunks, chunk,
                                     self._ptr(out, torch.complex64)))
        return out

    def fft_x_bin(self, lines, N, nlines, line0, kz0, nseg, seg_stride, psum, nsample, count=True):
        """x pass + shell sums into psum; with `count` also the shell counts into nsample."""
        self._stream()
        self._chk(self.lib.vps_fft_x(self.ctx, N, nlines, line0, kz0, self._ptr(lines, torch.complex64), nseg,
                                     seg_stride, 0 if count else 3, self._ptr(psum, torch.float64),
                                     self._ptr(nsample, torch.int64), None))

    def fft_x_bin_multi(self, comps, N, nlines, line0, kz0, nseg, seg_stride, psum, nsample, count=True):
        """x pass of up to three component spectra, |F|^2 summed over the components, binned once."""
        self._stream()
        ptrs = (C.c_void_p * len(comps))(*[self._ptr(c, torch.complex64).value for c in comps])
        self._chk(self.lib.vps_fft_x_bin(self.ctx, N, nlines, line0, kz0, ptrs, len(comps), nseg, seg_stride,
                                         1 if count else 0, self._ptr(psum, torch.float64),
                                         self._ptr(nsample, torch.int64)))

    def fft_x_bin_chunk(self, comps, N, nx, G, nchunks, chunk, rank, packed, psum, nsample, count=True):
        """Binning x pass of one RECEIVED chunk of the slab exchange (the G blocks per component, fft_y_chunk's layout; the
        last chunk's Nyquist-plane rows included), up to three components summed before the shell search."""
        self._stream()
        ptrs = (C.c_void_p * len(comps))(*[self._ptr(c, torch.complex64).value for c in comps])
        self._chk(self.lib.vps_fft_x_bin_chunk(self.ctx, int(N), int(nx), int(G), int(nchunks), int(chunk), int(rank),
                                               int(bool(packed)), ptrs, len(comps), 1 if count else 0,
                                               self._ptr(psum, torch.float64), self._ptr(nsample, torch.int64)))

    def fft_x_bin_helmholtz(self, comps, N, nlines, line0, kz0, nseg, seg_stride, psum, nsample, pcomp, count=True):
        """fft_x_bin_multi of the three components of a vector field that also bins the compressive part of every mode,
        |k'.F|^2 / |k'|^2, into pcomp (vps_fft_x_bin_helmholtz)."""
        self._stream()
        ptrs = (C.c_void_p * len(comps))(*[self._ptr(c, torch.complex64).value for c in comps])
        self._chk(self.lib.vps_fft_x_bin_helmholtz(self.ctx, N, nlines, line0, kz0, ptrs, len(comps), nseg, seg_stride,
                                                   1 if count else 0, self._ptr(psum, torch.float64),
                                                   self._ptr(nsample, torch.int64), self._ptr(pcomp, torch.float64)))

    def fft_x_bin_chunk_helmholtz(self, comps, N, nx, G, nchunks, chunk, rank, packed, psum, nsample, pcomp, count=True):
        """fft_x_bin_chunk of the three components of a vector field with the compressive part binned into pcomp
        (vps_fft_x_bin_chunk_helmholtz)."""
        self._stream()
        ptrs = (C.c_void_p * len(comps))(*[self._ptr(c, torch.complex64).value for c in comps])
        self._chk(self.lib.vps_fft_x_bin_chunk_helmholtz(self.ctx, int(N), int(nx), int(G), int(nchunks), int(chunk), int(rank),
                                                         int(bool(packed)), ptrs, len(comps), 1 if count else 0,
                                                         self._ptr(psum, torch.float64), self._ptr(nsample, torch.int64),
                                                         self._ptr(pcomp, torch.float64)))

    # -- the slab exchange inside the library (RCCL behind the C ABI) -------------
    @staticmethod
    def comm_unique_id():
        """128 bytes from ncclGetUniqueId: made on one rank, handed to all (the host moves them)."""
        buf = C.create_string_buffer(128)
        lib = _ffi.lib()
        rc = lib.vps_comm_unique_id(buf)
        if rc != 0:
            raise _ffi.VpsError("vps_comm_unique_id failed (%d): %s" % (rc, lib.vps_last_error(None).decode()))
        return buf.raw

    def comm_create(self, rank, world, uid):
        """Collective over the job's ranks: an RCCL communicator on this context's device."""
        self._chk(self.lib.vps_comm_create(self.ctx, int(rank), int(world), bytes(uid)))
        self.comm_rank, self.comm_world = int(rank), int(world)

    def comm_destroy(self):
        self._chk(self.lib.vps_comm_destroy(self.ctx))

    def spectrum_zimages(self, zimgs, N, nx, nchunks, psum, nsample, count=True):
        """vps_spectrum_zimages: chunked y pass -> grouped ncclSend / ncclRecv -> binning x pass of up to three z images,
        all inside the library (its own communication stream and events)."""
        self._stream()
        G = self.comm_world
        ptrs = (C.c_void_p * len(zimgs))(*[self._ptr(z, torch.complex64).value for z in zimgs])
        work = self.workspace("exchange", self.lib.vps_spectrum_zimages_workspace_bytes(int(N), int(nx), G, int(nchunks), len(zimgs)))
        self._chk(self.lib.vps_spectrum_zimages(self.ctx, int(N), int(nx), ptrs, len(zimgs), int(nchunks), self._ptr(work),
                                                1 if count else 0, self._ptr(psum, torch.float64), self._ptr(nsample, torch.int64)))

    def allreduce_shells(self, psum, nsample):
        self._stream()
        self._chk(self.lib.vps_allreduce_shells(self.ctx, self._ptr(psum, torch.float64), self._ptr(nsample, torch.int64),
                                                int(psum.numel())))

    def fft_x_write(self, lines, N, nlines, nseg, seg_stride, out):
        self._stream()
        self._chk(self.lib.vps_fft_x(self.ctx, N, nlines, 0, 0, self._ptr(lines, torch.complex64), nseg,
                                     seg_stride, 1, None, None, self._ptr(out, torch.complex64)))

    def rfft3(self, field, N):
        """Half spectrum F[kz][ky][kx], kz <= N/2, of a full [N,N,N] float32 field."""
        self._stream()
        out = self.empty((N // 2 + 1, N, N), torch.complex64)
        work = self.workspace("power", self.lib.vps_power_workspace_bytes(N))
        self._chk(self.lib.vps_rfft3(self.ctx, N, self._ptr(field, torch.float32), self._ptr(work),
                                     self._ptr(out)))
        return out

    def power_grid(self, fields, N):
        """sum over fields of |F[kz][ky][kx]|^2, kz <= N/2, float32."""
        self._stream()
        out = self.zeros((N // 2 + 1, N, N), torch.float32)
        work = self.workspace("power", self.lib.vps_power_workspace_bytes(N))
        for f in fields:
            self._chk(self.lib.vps_power_grid(self.ctx, N, self._ptr(f, torch.float32), self._ptr(work),
                                              self._ptr(out)))
        return out

    def fft_x_mode(self, lines, N, nlines, line0, kz0, mode, psum=None, nsample=None, out=None, nseg=1, seg_stride=0):
        """vps_fft_x in any of its modes (include/vps_hip.h) on complex64 lines; the accumulators / output a mode does not take
        stay None."""
        self._stream()
        self._chk(self.lib.vps_fft_x(self.ctx, int(N), int(nlines), int(line0), int(kz0), self._ptr(lines, torch.complex64),
                                     int(nseg), int(seg_stride), int(mode), self._ptr(psum, torch.float64),
                                     self._ptr(nsample, torch.int64), self._ptr(out)))

    def _zy_into_power_workspace(self, field, N):
        """z and y pass of a whole [N,N,N] float32 field inside the power workspace: -> (spec [N/2,N,N], nyq [N,N]) views of
        its second half (the layout vps_power_grid uses)."""
        half = int(self.lib.vps_fft_workspace_bytes(N, N))
        work = self.workspace("power", self.lib.vps_power_workspace_bytes(N))
        nspec = (N // 2) * N * N
        img = work[half: 2 * half].view(torch.complex64)
        spec, nyq = img[:nspec].view(N // 2, N, N), img[nspec: nspec + N * N].view(N, N)
        self._chk(self.lib.vps_fft_zy(self.ctx, N, N, self._ptr(field, torch.float32), self._ptr(spec), self._ptr(nyq),
                                      self._ptr(work)))
        return spec, nyq

    def power_grid_full(self, fields, N):
        """sum over fields of |F|^2 on the FULL Hermitian grid [kz][ky][kx], N^3 float32 (vps_fft_x mode 5): a real, even field
        that the real-input z pass takes -- its forward transform is N^3 times the autocorrelation.  Every row is read: the y
        passes run outside any binning-only scope."""
        self._stream()
        self._chk(self.lib.vps_set_bin_only(self.ctx, 0))
        out = self.zeros((N, N, N), torch.float32)
        for f in fields:
            spec, nyq = self._zy_into_power_workspace(f, N)
            self.fft_x_mode(spec, N, (N // 2) * N, 0, 0, 5, out=out)
            self.fft_x_mode(nyq, N, N, 0, N // 2, 5, out=out)
        return out

    def bin_real(self, grid, N, psum, nsample):
        """Transform the real [N,N,N] float32 `grid` and ADD the shell sums of w Re F into psum (float64) and w into nsample
        (int64) with the tables set last (vps_fft_x mode 6; w the Hermitian multiplicity of the kz plane).  The y pass skips
        the rows no shell of those tables holds, as the spectrum's binning does."""
        self._stream()
        with self.binning_only():
            spec, nyq = self._zy_into_power_workspace(grid, N)
        self.fft_x_mode(spec, N, (N // 2) * N, 0, 0, 6, psum=psum, nsample=nsample)
        self.fft_x_mode(nyq, N, N, 0, N // 2, 6, psum=psum, nsample=nsample)
        return psum, nsample

    def pair_k(self, kx, ky, kz):
        self._stream()
        ax = [np.ascontiguousarray(a, dtype=np.float64) for a in (kx, ky, kz)]
        N = len(ax[0])
        out = self.empty((N * N * N,), torch.float64)
        self._chk(self.lib.vps_pair_k(self.ctx, N, _ffi.as_dp(ax[0]), _ffi.as_dp(ax[1]), _ffi.as_dp(ax[2]),
                                      self._ptr(out)))
        return out

    def hist_pairs(self, k, w, edges, psum=None, nsample=None):
        """numpy.histogram(k, edges, weights=w) and the counts, ADDED to psum / nsample if given (else to zeros); at most
        device_info()["hist_max_bins"] bins."""
        self._stream()
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        nb = len(edges) - 1
        psum = self.zeros((nb,), torch.float64) if psum is None else psum
        ns = self.zeros((nb,), torch.int64) if nsample is None else nsample
        if psum.shape != (nb,) or ns.shape != (nb,):
            raise _ffi.VpsError("psum / nsample must have one entry per bin")
        self._chk(self.lib.vps_hist_pairs(self.ctx, self._ptr(k, torch.float64),
                                          self._ptr(w, torch.float64) if w is not None else None,
                                          k.numel(), _ffi.as_dp(edges), nb, self._ptr(psum, torch.float64),
                                          self._ptr(ns, torch.int64)))
        return psum, ns


_default_kernels = {}


def nn_plan(np_, pos_is_f64=False, nq_slab=0):
    """{field: int} over _ffi.NN_PLAN_FIELDS: the cell list vps_nn_resample* would build for np_ particles under the current
    options (vps_nn_plan: host only, no context and no device needed)."""
    out = (C.c_int64 * len(_ffi.NN_PLAN_FIELDS))()
    rc = _ffi.lib().vps_nn_plan(int(np_), 1 if pos_is_f64 else 0, int(nq_slab), out)
    if rc != 0:
        raise _ffi.VpsError("vps_nn_plan failed (%d): np = %r" % (rc, np_))
    return dict(zip(_ffi.NN_PLAN_FIELDS, (int(v) for v in out)))


def default_kernels(device=None):
    """Process-wide HipKernels for a device (created on first use)."""
    if device is None:
        if not torch.cuda.is_available():
            raise _ffi.VpsError("no HIP device is visible to this process; the vpower device path "
                                "needs an MI355X (there is no CPU fallback)")
        device = torch.cuda.current_device()
    idx = device if isinstance(device, int) else torch.device(device).index
    k = _default_kernels.get(idx)
    if k is None:
        k = HipKernels(idx)
        _default_kernels[idx] = k
    return k


# --------------------------------------------------------------------------- #
# the pipeline
# --------------------------------------------------------------------------- #
class SlabComm:
    """Rank / world bookkeeping and the two collectives the path needs."""

    def __init__(self, group=None, enabled=None):
        import torch.distributed as dist
        self.dist = dist
        if enabled is None:
            enabled = dist.is_available() and dist.is_initialized()
        self.enabled = bool(enabled)
        self.group = group
        self.rank = dist.get_rank(group) if self.enabled else 0
        self.world = dist.get_world_size(group) if self.enabled else 1
        self.backend = dist.get_backend(group) if self.enabled else None
        # VPS_FORCE_COLLECTIVES=1: issue the collectives even in a one-rank group (exercises the RCCL
        # plumbing -- complex views, async work handles -- on a single GPU; tests only)
        self.force = self.enabled and os.environ.get("VPS_FORCE_COLLECTIVES") == "1"

    def all_to_all_start(self, send):
        """Begin an equal-split all-to-all along dim 0 of a contiguous tensor.  Returns
        (recv, work); `all_to_all_finish` makes `recv` usable on the current stream.  With
        RCCL the exchange runs on the communicator's stream, so kernels issued in between
        (the z/y passes of the next field, the x pass of the previous one) overlap it."""
        if self.world == 1 and not self.force:
            return send, None
        if send.is_cuda and self.backend != "nccl":
            # gloo rehearsal on a GPU box: stage through host memory (synchronous)
            h = send.cpu()
            r = torch.empty_like(h)
            self.dist.all_to_all_single(r, h, group=self.group)
            return r.to(send.device), None
        if send.is_complex():
            s = torch.view_as_real(send)
            recv = torch.empty_like(send)
            r = torch.view_as_real(recv)
            if not send.is_cuda:           # gloo wants plain contiguous real tensors
                s = s.contiguous()
                r = torch.empty_like(s)
                recv = torch.view_as_complex(r)
            work = self.dist.all_to_all_single(r, s, group=self.group, async_op=True)
            return recv, (work, s)        # keep the send view alive until the wait
        recv = torch.empty_like(send)
        work = self.dist.all_to_all_single(recv, send, group=self.group, async_op=True)
        return recv, (work, send)

    @staticmethod
    def all_to_all_finish(handle):
        recv, work = handle
        if work is not None:
            work[0].wait()
        return recv

    def all_to_all(self, send):
        """Blocking form of all_to_all_start / all_to_all_finish."""
        return self.all_to_all_finish(self.all_to_all_start(send))

    def all_reduce_sum(self, t):
        if self.world == 1 and not self.force:
            return t
        if t.is_cuda and self.backend != "nccl":
            h = t.cpu()
            self.dist.all_reduce(h, group=self.group)
            t.copy_(h)
            return t
        self.dist.all_reduce(t, group=self.group)
        return t


class FieldComm(SlabComm):
    """Field-parallel ranks: every rank holds WHOLE grids and transforms a share of the scalar fields of a step (the three
    components of a vector quantity, the energy field, several quantities); nothing but the shell tables crosses the node.
    For grids that fit one GPU's 288 GB this is the decomposition that suits point-to-point xGMI: the slab decomposition sends
    the whole half spectrum through the links once per field (at two ranks through ONE link), this one sends nbins numbers.
    To the pipeline the rank is a one-rank slab (world = 1: nx = N, no exchange); `field_rank` / `field_world` say which
    fields are this rank's (`mine`), and the closing reductions ADD the shell sums of all ranks and take the shell counts from
    whichever ranks counted (MAX: they depend on the mode lattice alone, so every rank that counted holds the same numbers)."""

    def __init__(self, group=None, enabled=None):
        super().__init__(group=group, enabled=enabled)
        self.field_rank, self.field_world = self.rank, self.world
        self.rank, self.world, self.force = 0, 1, False

    @staticmethod
    def units(quantities):
        """The scalar fields of a step, in dealing order: (quantity, component) -- component None for a scalar quantity (the
        energy, the density, the log-density: one unit each).  A quantity is a name or a code; every other one (a
        WeightedVelocity included) is dealt out by component."""
        def scalar(q):
            return q in SCALAR_QUANTITIES if isinstance(q, str) else NCOMP[int(q)] == 1
        return [(q, c) for q in quantities for c in ((None,) if scalar(q) else (0, 1, 2))]

    def mine(self, quantities):
        """This rank's fields: CONTIGUOUS blocks of the dealing order (the first n mod W ranks take one more), so that a rank's
        fields mostly belong to one quantity and go through one multi-component launch (shared rho round, one shell search)."""
        u = self.units(quantities)
        W, r = self.field_world, self.field_rank
        base, extra = divmod(len(u), W)
        lo = r * base + min(r, extra)
        return u[lo: lo + base + (1 if r < extra else 0)]

    def all_reduce_sum(self, t):
        if self.field_world == 1:
            return t
        op = self.dist.ReduceOp.SUM if t.is_floating_point() else self.dist.ReduceOp.MAX
        if t.is_cuda and self.backend != "nccl":
            h = t.cpu()
            self.dist.all_reduce(h, op=op, group=self.group)
            t.copy_(h)
            return t
        self.dist.all_reduce(t, op=op, group=self.group)
        return t


class LibraryComm(SlabComm):
    """The same two collectives, run INSIDE libvps_hip.so over RCCL (vps_comm_create / vps_spectrum_zimages /
    vps_allreduce_shells): what a host without torch.distributed uses.  `PowerPipeline` hands whole groups of z images to
    the library, which owns the chunk pipeline (communication stream, events).  rank / world / uid come from the host --
    here: from an initialised torch.distributed group (only to move the 128-byte id), or explicitly."""

    def __init__(self, kernels, rank=None, world=None, uid=None, group=None):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        if rank is None:
            if not (dist.is_available() and dist.is_initialized()):
                rank, world = 0, 1
            else:
                rank, world = dist.get_rank(group), dist.get_world_size(group)
        if uid is None:
            box = [HipKernels.comm_unique_id() if rank == 0 else None]
            if world > 1:
                dist.broadcast_object_list(box, src=0, group=group)
            uid = box[0]
        self.rank, self.world = int(rank), int(world)
        self.enabled, self.force, self.backend = True, True, "library"
        self.k = kernels
        kernels.comm_create(self.rank, self.world, uid)

    def all_reduce_shells(self, psum, nsample):
        self.k.allreduce_shells(psum, nsample)


class PowerPipeline:
    """P(k) of real fields on an N^3 grid of box length Lbox, slab-decomposed over the
    ranks of `comm` (default: the initialised torch.distributed world, else 1 rank)."""

    def __init__(self, Nsize, Lbox, kernels=None, comm=None, flavour="library",
                 kmin=None, kmax=None, kres=None, deconvolve=None):
        self.N = int(Nsize)
        self.Lbox = float(Lbox)
        self.Lcell = self.Lbox / self.N
        self.k = kernels if kernels is not None else default_kernels()
        self.comm = comm if comm is not None else SlabComm()
        G = self.comm.world
        if not self.k.fft_supported(self.N):
            raise Exception("Nsize=%d is not supported by the device FFT (powers of two 16..4096, 96, 192, 384, 768, 1536, 250, 500, 1000, 2000)" % self.N)
        if self.N % G or (self.N // 2) % G:
            raise Exception("Nsize/2=%d must be divisible by the number of ranks %d" % (self.N // 2, G))
        if G > x_max_ranks(self.N):    # refused here, before any exchange is enqueued: the x pass would refuse mid-pipeline
            raise Exception("Nsize=%d takes at most %d ranks, not %d: the x pass needs segments of at least %d points per line"
                            % (self.N, x_max_ranks(self.N), G, self.N // x_max_ranks(self.N)))
        self.nx = self.N // G
        self.x0 = self.comm.rank * self.nx
        self.flavour = flavour
        # defaults of BoxField.spctrm (interp.py:565-570) / main() (parallel_optimized.py:430)
        self.kmin = 2 * np.pi / self.Lbox if kmin is None else kmin
        self.kmax = np.pi / self.Lcell if kmax is None else kmax
        self.kres = self.kmin if kres is None else kres
        self.centers, self.edges = bin_edges(self.kmin, self.kmax, self.kres, flavour)
        self.nbins = len(self.centers)
        self._binning = binning_tables(k_axis(self.Lbox, self.N), self.edges)
        self.k2, self.thr = self._binning[1], self._binning[2]
        self.const = (self.Lbox / (2 * np.pi)) ** 1.5 / self.N ** 3   # interp.py:1381
        # deconvolve = "ngp" | "cic" | "tsc": divide every |F(k)|^2 by the assignment window W(k)^2 while binning
        self.window = None if deconvolve is None else window_inv2_axis(self.N, deconvolve)
        # Several ranks: every scalar field crosses the node as ONE message per pair of ranks (its kz rows with the
        # Nyquist-plane rows riding behind them), cut into `nchunks` kz chunks so that the exchange of a chunk
        # overlaps the y pass of the next and the x pass of the previous one.
        self.chunked = G > 1 or self.comm.force or os.environ.get("VPS_CHUNKED") == "1"
        self.nchunks = self._pick_chunks()

    def _pick_chunks(self):
        """kz chunks per field: VPS_A2A_CHUNKS (default 4), lowered until it divides the rank's kz rows and a
        chunk's pair message stays above 2 MiB (smaller messages are latency-bound on xGMI)."""
        G = self.comm.world
        nkz = self.N // 2 // G
        try:
            c = max(1, int(os.environ.get("VPS_A2A_CHUNKS", "4")))
        except ValueError:
            c = 4
        c = min(c, nkz)
        while c > 1 and (nkz % c or (os.environ.get("VPS_A2A_CHUNKS") is None
                                     and nkz // c * self.N * self.nx * 8 < (2 << 20))):
            c -= 1
        return max(c, 1)

    def kept_row_fraction(self, kz_lo=0, kz_hi=None):
        """Fraction of the (ky, kz) rows of kz planes [kz_lo, kz_hi) that the binning passes keep: a row whose modes all
        lie beyond the last shell edge -- fl(ky^2 + kz^2) >= thr[nbins] -- is neither stored by the y pass nor read by
        the x pass (same rule and 16-row rounding as vps_set_binning's cut table; 1.0 for N < 128)."""
        N = self.N
        kz_hi = N // 2 if kz_hi is None else kz_hi
        if N < 128:
            return 1.0
        k2h = self.k2[: N // 2 + 1]
        kept = 0
        for kz in range(kz_lo, kz_hi):
            ok = np.nonzero(~((k2h + self.k2[kz]) >= self.thr[-1]))[0]
            if len(ok):
                kc = min(int(ok[-1]) | 15, N // 2)
                kept += min(2 * kc + 1, N)
        return kept / float(N * max(kz_hi - kz_lo, 1))

    def prepare(self):
        """Upload this pipeline's binning (and window) tables; `self.k.binning_only()` scopes refer to them."""
        self.k.set_binning(*self._binning)
        self._set_window()

    def _bin_scope(self):
        import contextlib
        return self.k.binning_only() if hasattr(self.k, "binning_only") else contextlib.nullcontext()

    # -- the chunk pipeline of the slab exchange ------------------------------------------------------------------------
    # A JOB is one kz chunk of up to three z images (the components of a vector quantity share one binning launch): y pass
    # into fresh send buffers -> all-to-all (asynchronous) -> x pass + shell sums of the received blocks.  Jobs are started
    # in order and at most `inflight_max` of them (VPS_A2A_INFLIGHT, default 2) are between their start and their x pass:
    # job j + 1 crosses the node while job j is binned, and only TWO chunks' send / receive buffers are alive, whatever the
    # chunk count -- not the whole field twice over.  The jobs of several quantities form ONE sequence: the next quantity's
    # deposit + z pass is enqueued while the last chunks of the previous one are still travelling.
    def inflight_max(self):
        try:
            return max(1, int(os.environ.get("VPS_A2A_INFLIGHT", "2")))
        except ValueError:
            return 2

    def _stamp(self):
        """Timing event on the current stream (instrumented steps only: `self.instr` is a list)."""
        if getattr(self, "instr", None) is None or not torch.cuda.is_available():
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _start_chunk(self, comps, c, packed):
        N, nx, G = self.N, self.nx, self.comm.world
        sends = [self.k.fft_y_chunk(z, N, nx, G, self.nchunks, c) for z in comps]
        t0 = self._stamp()
        return {"handles": [self.comm.all_to_all_start(s_) for s_ in sends], "chunk": c, "packed": packed, "t0": t0}

    def _finish_chunk(self, job, psum, nsample, count, pcomp=None):
        N, nx, G, r = self.N, self.nx, self.comm.world, self.comm.rank
        t1 = self._stamp()
        recvs = [self.comm.all_to_all_finish(h) for h in job["handles"]]
        t2 = self._stamp()
        if t1 is not None:
            self.instr.append((job["t0"], t1, t2))      # exchange started | x pass ready to go | blocks there
        job["handles"] = None
        if pcomp is not None:
            self.k.fft_x_bin_chunk_helmholtz(recvs, N, nx, G, self.nchunks, job["chunk"], r, job["packed"], psum, nsample, pcomp,
                                             count=count)
            return
        self.k.fft_x_bin_chunk(recvs, N, nx, G, self.nchunks, job["chunk"], r, job["packed"], psum, nsample, count=count)

    def exchange_times(self):
        """(exposed_ms, span_ms) of the instrumented jobs so far: the time the compute stream stood still waiting for blocks,
        and -- meaningful when the jobs ran one at a time (inflight_max = 1) -- the time from a job's exchange start to its
        arrival.  Synchronises."""
        torch.cuda.synchronize()
        ex = sum(a.elapsed_time(b) for _, a, b in self.instr)
        span = sum(a.elapsed_time(b) for a, _, b in self.instr)
        return ex, span

    def pipelined_quantities(self, producers, accumulators, counts=None):
        """The jobs of several quantities of ONE particle set as one bounded pipeline: producers[i]() enqueues quantity i's
        deposit + z pass and returns its z images (one per component, which may live in the SAME buffer for every quantity:
        by then all y passes of quantity i - 1 have been enqueued); its chunks are binned into accumulators[i] =
        (psum, nsample).  counts[i] (default True): whether quantity i's shell counts are accumulated (first group only).
        Helmholtz decomposition: accumulators[i] = (psum, nsample, pcomp) bins quantity i's three components in one launch
        that also accumulates the compressive part into pcomp (VPS_X_PER_COMPONENT does not apply to it).
        What `bench.py` runs on several ranks (torch transport); one quantity: `accumulate_zimages`."""
        import collections
        if any(len(a) > 2 for a in accumulators):
            self._check_helmholtz()
        per_component = os.environ.get("VPS_X_PER_COMPONENT") == "1"
        k, C_, maxin = self.k, self.nchunks, self.inflight_max()
        inflight = collections.deque()

        def finish_oldest():
            job, qi, cnt = inflight.popleft()
            acc = accumulators[qi]
            self._finish_chunk(job, acc[0], acc[1], cnt, acc[2] if len(acc) > 2 else None)
        self.prepare()
        for qi, produce in enumerate(producers):
            zimgs = produce()
            cnt = True if counts is None else bool(counts[qi])
            helm = len(accumulators[qi]) > 2
            if helm and len(zimgs) != 3:
                raise Exception("the Helmholtz decomposition needs the three components of a vector quantity (got %d z images)"
                                % len(zimgs))
            group = 1 if per_component and not helm else 3
            for i in range(0, len(zimgs), group):
                for c in range(C_):
                    while len(inflight) >= maxin:
                        finish_oldest()
                    with self._bin_scope():   # the blocks carry only the rows a shell can reach
                        packed = k.y_packed(self.N) if hasattr(k, "y_packed") else False
                        inflight.append((self._start_chunk(zimgs[i:i + group], c, packed), qi, cnt and i == 0))
        while inflight:
            finish_oldest()
        return accumulators

    def start_zimages(self, zimgs):
        """Every chunk of every group of `zimgs` started at once (y pass + all-to-all); `finish_zimages` bins them.  All
        send / receive buffers are alive in between: the bounded form is `accumulate_zimages` / `pipelined_quantities`."""
        group = 1 if os.environ.get("VPS_X_PER_COMPONENT") == "1" else 3
        self.prepare()
        groups = []
        with self._bin_scope():
            packed = self.k.y_packed(self.N) if hasattr(self.k, "y_packed") else False
            for i in range(0, len(zimgs), group):
                groups.append([self._start_chunk(zimgs[i:i + group], c, packed) for c in range(self.nchunks)])
        return {"packed": packed, "groups": groups}

    def finish_zimages(self, started, psum=None, nsample=None, count=True):
        self.prepare()
        if psum is None:
            psum, nsample = self.new_accumulators()
        for i, jobs in enumerate(started["groups"]):
            for c in range(self.nchunks):
                self._finish_chunk(jobs[c], psum, nsample, count and i == 0)
                jobs[c] = None
        return psum, nsample

    def _check_helmholtz(self):
        """Refuse the Helmholtz decomposition where it is not implemented -- before anything is enqueued."""
        if isinstance(self.comm, LibraryComm):
            raise Exception("the Helmholtz decomposition is not available with LibraryComm (vps_spectrum_zimages bins |F|^2 "
                            "only): use the torch.distributed transport (SlabComm)")

    def accumulate_zimages_helmholtz(self, zimgs, acc=None, count=True):
        """accumulate_zimages of the three z images of a vector quantity with the Helmholtz decomposition: -> (psum, nsample,
        pcomp), pcomp the shell sums of the compressive part |k'.F|^2 / |k'|^2 (`new_accumulators(helmholtz=True)`)."""
        self._check_helmholtz()
        if len(zimgs) != 3:
            raise Exception("the Helmholtz decomposition needs the three components of a vector quantity")
        acc = self.new_accumulators(helmholtz=True) if acc is None else acc
        self.pipelined_quantities([lambda: zimgs], [acc], counts=[count])
        return acc

    def accumulate_zimages(self, zimgs, psum=None, nsample=None, count=True):
        """x-side of the transform for z images (HipKernels.fft_z / deposit_fft_z): per kz chunk, y pass into the
        send buffer, all-to-all, x pass + shell sums, two chunks in flight (`pipelined_quantities`)."""
        group = 1 if os.environ.get("VPS_X_PER_COMPONENT") == "1" else 3
        if psum is None:
            psum, nsample = self.new_accumulators()
        if isinstance(self.comm, LibraryComm):     # the whole chunk pipeline runs inside the library (RCCL, two chunk slots)
            self.prepare()
            for i in range(0, len(zimgs), group):
                self.k.spectrum_zimages(zimgs[i:i + group], self.N, self.nx, self.nchunks, psum, nsample, count=count and i == 0)
            return psum, nsample
        self.pipelined_quantities([lambda: zimgs], [(psum, nsample)], counts=[count])
        return psum, nsample

    # -- stage B + C on one or more real fields of this rank's slab ---------------
    def accumulate_helmholtz(self, fields, acc=None, count=True, weight=None):
        """`accumulate` of the three components of a vector quantity with the Helmholtz decomposition: -> (psum, nsample,
        pcomp) -- psum, nsample exactly what `accumulate` adds, pcomp the shell sums of the compressive part
        |k'.F|^2 / |k'|^2 of every mode (k' = integer mode numbers, Nyquist entries 0; `HipKernels.fft_x_bin_helmholtz`)."""
        self._check_helmholtz()
        if len(fields) != 3:
            raise Exception("the Helmholtz decomposition needs the three components of a vector quantity")
        N, nx = self.N, self.nx
        k = self.k
        k.set_binning(*self._binning)
        self._set_window()
        acc = self.new_accumulators(helmholtz=True) if acc is None else acc
        if self.chunked:
            zimgs = [k.fft_z(f, N, nx, weight=weight) for f in fields]
            return self.accumulate_zimages_helmholtz(zimgs, acc, count)
        pending = []
        with self._bin_scope():
            for f in fields:
                spec, nyq = k.fft_zy(f, N, nx) if weight is None else k.fft_zy(f, N, nx, weight=weight)
                pending.append((self.comm.all_to_all_start(spec), self.comm.all_to_all_start(nyq)))
        self._bin_exchanged(pending, acc[0], acc[1], count, pcomp=acc[2])
        return acc

    def accumulate(self, fields, psum=None, nsample=None, count=True, weight=None):
        """Add sum_w |F|^2 of every field ([nx,N,N] float32) into the shell sums, and (with
        `count`) the number of modes per shell into nsample -- once, on the first field: the
        reference histograms the component-summed P grid once (interp.py:1474-1477).
        Returns LOCAL (this rank's) accumulators; call `finish` to reduce them."""
        N, nx, G, r = self.N, self.nx, self.comm.world, self.comm.rank
        k = self.k
        k.set_binning(*self._binning)
        self._set_window()
        if psum is None:
            psum, nsample = self.new_accumulators()
        if self.chunked:
            zimgs = [k.fft_z(f, N, nx, weight=weight) for f in fields]
            return self.accumulate_zimages(zimgs, psum, nsample, count)
        nkz = N // 2 // G      # kz rows per rank after the exchange
        nky = N // G           # Nyquist-plane ky rows per rank
        # one rank: no exchange -- z/y passes of every field, then the x passes
        pending = []
        with self._bin_scope():
            for f in fields:
                spec, nyq = k.fft_zy(f, N, nx) if weight is None else k.fft_zy(f, N, nx, weight=weight)
                pending.append((self.comm.all_to_all_start(spec), self.comm.all_to_all_start(nyq)))
        self._bin_exchanged(pending, psum, nsample, count)
        return psum, nsample

    def _bin_exchanged(self, pending, psum, nsample, count, pcomp=None):
        """x pass + shell sums of exchanged spectra.  Up to three components at a time go through ONE
        launch that sums their |F|^2 before the shell search (what the reference does on the grid,
        interp.py:1386, 1474-1477); VPS_X_PER_COMPONENT=1 bins every component on its own instead.
        pcomp (Helmholtz decomposition, three components): the compressive part is binned into it by the same launch."""
        N, nx, G, r = self.N, self.nx, self.comm.world, self.comm.rank
        k = self.k
        nkz, nky = N // 2 // G, N // G
        done = [(self.comm.all_to_all_finish(hs), self.comm.all_to_all_finish(hq)) for hs, hq in pending]
        if pcomp is not None:
            specs, nyqs = [d[0] for d in done], [d[1] for d in done]
            k.fft_x_bin_helmholtz(specs, N, nkz * N, 0, r * nkz, G, nkz * N * nx, psum, nsample, pcomp, count=count)
            k.fft_x_bin_helmholtz(nyqs, N, nky, r * nky, N // 2, G, nky * nx, psum, nsample, pcomp, count=count)
            return
        group = 1 if os.environ.get("VPS_X_PER_COMPONENT") == "1" else 3
        for i in range(0, len(done), group):
            c = count and i == 0
            specs = [d[0] for d in done[i:i + group]]
            nyqs = [d[1] for d in done[i:i + group]]
            k.fft_x_bin_multi(specs, N, nkz * N, 0, r * nkz, G, nkz * N * nx, psum, nsample, count=c)
            k.fft_x_bin_multi(nyqs, N, nky, r * nky, N // 2, G, nky * nx, psum, nsample, count=c)

    def accumulate_spectra(self, spec, nyq, psum=None, nsample=None, count=True):
        """Like `accumulate`, for fields that already went through the z and y passes
        (spec [ncomp, N/2, N, nx], nyq [ncomp, N, nx], e.g. from HipKernels.deposit_fft_zy)."""
        N, nx, G, r = self.N, self.nx, self.comm.world, self.comm.rank
        if self.chunked:
            raise Exception("several ranks exchange z images chunk by chunk: use HipKernels.deposit_fft_z / fft_z "
                            "and PowerPipeline.accumulate_zimages")
        k = self.k
        k.set_binning(*self._binning)
        self._set_window()
        if psum is None:
            psum, nsample = self.new_accumulators()
        nkz, nky = N // 2 // G, N // G
        pending = [(self.comm.all_to_all_start(spec[i]), self.comm.all_to_all_start(nyq[i]))
                   for i in range(spec.shape[0])]
        self._bin_exchanged(pending, psum, nsample, count)
        return psum, nsample

    def accumulate_spectra_helmholtz(self, spec, nyq, acc=None, count=True):
        """`accumulate_spectra` of the three z/y-transformed components (spec [3, N/2, N, nx], nyq [3, N, nx]) with the
        Helmholtz decomposition: -> (psum, nsample, pcomp), as `accumulate_helmholtz`."""
        self._check_helmholtz()
        N, G = self.N, self.comm.world
        if self.chunked:
            raise Exception("several ranks exchange z images chunk by chunk: use HipKernels.deposit_fft_z / fft_z "
                            "and PowerPipeline.accumulate_zimages_helmholtz")
        if spec.shape[0] != 3 or nyq.shape[0] != 3:
            raise Exception("the Helmholtz decomposition needs the three components of a vector quantity")
        k = self.k
        k.set_binning(*self._binning)
        self._set_window()
        acc = self.new_accumulators(helmholtz=True) if acc is None else acc
        pending = [(self.comm.all_to_all_start(spec[i]), self.comm.all_to_all_start(nyq[i])) for i in range(3)]
        self._bin_exchanged(pending, acc[0], acc[1], count, pcomp=acc[2])
        return acc

    def _set_window(self):
        if hasattr(self.k, "set_window"):
            self.k.set_window(self.N, self.window)
        elif self.window is not None:
            raise Exception("this kernel set has no window deconvolution")

    def new_accumulators(self, helmholtz=False):
        """Zeroed shell sums (float64) and shell counts (int64) as two views of ONE device buffer, so that a
        step clears them with one fill and `finish` brings them to the host with one copy.  helmholtz: a third view, the
        float64 shell sums of the compressive part (`accumulate_helmholtz`), behind the other two."""
        buf = self.k.zeros(((3 if helmholtz else 2) * self.nbins,), torch.float64)
        self._acc_buf = buf
        nb = self.nbins
        if helmholtz:
            return buf[:nb], buf[nb: 2 * nb].view(torch.int64), buf[2 * nb:]
        return buf[:nb], buf[nb:].view(torch.int64)

    def finish(self, psum, nsample, buf=None):
        """Reduce over ranks and build the reference's (nbins,4) table
        [centre, P, Psum, Nsample] (interp.py:1478-1480 / parallel_optimized.py:185-188),
        before the 4 pi k^2 factor.  buf: the ONE float64 buffer of 2 nbins words that psum and nsample are the two halves
        of (as `new_accumulators` lays them out), if the caller keeps several such pairs: one device-to-host copy."""
        if isinstance(self.comm, LibraryComm):
            self.comm.all_reduce_shells(psum, nsample)
        else:
            self.comm.all_reduce_sum(psum)
            self.comm.all_reduce_sum(nsample)
        if buf is None:
            buf = getattr(self, "_acc_buf", None)
        if (buf is not None and psum.data_ptr() == buf.data_ptr()
                and nsample.data_ptr() == buf.data_ptr() + 8 * self.nbins):
            host = buf.cpu()                         # one device-to-host copy for both accumulators
            self._acc_host = host if buf is getattr(self, "_acc_buf", None) else None
            ps = host[: self.nbins].numpy() * (0.5 * self.const ** 2)
            ns = host[self.nbins: 2 * self.nbins].view(torch.int64).numpy()
        else:
            self._acc_host = None
            ps = psum.cpu().numpy() * (0.5 * self.const ** 2)
            ns = nsample.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            P = ps / ns
        if self.flavour == "library":
            P[ns == 0] = 0                      # interp.py:1479
        return np.column_stack((self.centers, P, ps, ns.astype(np.float64)))

    def finish_helmholtz(self, psum, nsample, pcomp):
        """Reduce the three accumulators of `accumulate_helmholtz` over the ranks -> (total, compressive, solenoidal) tables
        [centre, P, Psum, Nsample] before the 4 pi k^2 factor.  total is `finish`'s table; the solenoidal shell sums are the
        float64 difference total - compressive; the three share the shell counts.  (Modes with k' = 0 -- k = 0 and the
        axis-Nyquist modes such as (N/2, 0, 0) -- have no compressive part: they count as solenoidal.)"""
        self._check_helmholtz()
        self.comm.all_reduce_sum(pcomp)
        tot = self.finish(psum, nsample)        # (one copy of all three when they are new_accumulators' views)
        host = getattr(self, "_acc_host", None)
        if host is not None and pcomp.data_ptr() == self._acc_buf.data_ptr() + 16 * self.nbins:
            pc = host[2 * self.nbins: 3 * self.nbins].numpy() * (0.5 * self.const ** 2)
        else:
            pc = pcomp.cpu().numpy() * (0.5 * self.const ** 2)
        ns = tot[:, 3]
        out = [tot]
        for ps in (pc, tot[:, 2] - pc):
            with np.errstate(invalid="ignore", divide="ignore"):
                P = ps / ns
            if self.flavour == "library":
                P[ns == 0] = 0
            out.append(np.column_stack((self.centers, P, ps, ns)))
        return tuple(out)

    def spectrum_helmholtz(self, fields, weight=None):
        """(total, compressive, solenoidal) P(k) tables of the three components of a vector quantity (each multiplied cell
        by cell by `weight` if given), times 4 pi k^2 (`accumulate_helmholtz`, `finish_helmholtz`)."""
        tabs = self.finish_helmholtz(*self.accumulate_helmholtz(fields, weight=weight))
        for tab in tabs:
            tab[:, 1] *= 4 * np.pi * tab[:, 0] ** 2
        return tabs

    def spectrum(self, fields, weight=None):
        """P(k) table of the fields (each multiplied cell by cell by `weight` if given), times 4 pi k^2."""
        psum, nsample = self.accumulate(fields, weight=weight)
        tab = self.finish(psum, nsample)
        tab[:, 1] *= 4 * np.pi * tab[:, 0] ** 2   # interp.py:590 / parallel_optimized.py:434
        return tab


class CorrelationPipeline:
    """xi(r) = <f(x) . f(x + r)> of real fields on a WHOLE N^3 grid of one GPU, binned in shells of the lag r.

    xi is the transform of the power grid |F|^2, and that grid is real and even: a second FORWARD transform gives it (the
    inverse would differ by the sign of an imaginary part that is zero).  So the three passes and the exact shell histogram
    of the spectrum serve unchanged, with the lags r = Lcell min(i, N - i) as the axis table (`r_axis`, `binning_tables`).
    Like `PowerPipeline` the object owns its tables and uploads them (window off) before it bins: it leaves no state that a
    spectrum computed afterwards could pick up.  x-slabs and several GPUs are out of scope: `comm` with more than one rank
    raises."""

    def __init__(self, Nsize, Lbox, kernels=None, rmin=None, rmax=None, rres=None, comm=None):
        self.N = int(Nsize)
        self.Lbox = float(Lbox)
        self.Lcell = self.Lbox / self.N
        if comm is not None and getattr(comm, "world", 1) > 1:
            raise Exception("the correlation function takes whole grids on one GPU: no x-slabs (%d ranks)" % comm.world)
        self.k = kernels if kernels is not None else default_kernels()
        if not self.k.fft_supported(self.N):
            raise Exception("Nsize=%d is not supported by the device FFT (powers of two 16..4096, 96, 192, 384, 768, 1536, 250, 500, 1000, 2000)" % self.N)
        self.edges = radial_edges(self.Lbox, self.N, rmin, rmax, rres)
        self.centers = 0.5 * (self.edges[:-1] + self.edges[1:])      # bin centres, as the k column of a spectrum
        self.nbins = len(self.centers)
        self._binning = binning_tables(r_axis(self.Lbox, self.N), self.edges)

    def prepare(self):
        self.k.set_binning(*self._binning)
        self.k.set_window(self.N, None)       # (a k-space window on the r lattice is refused by the library)

    def correlation(self, fields, subtract_mean=True):
        """-> (table [nbins, 3] of r, xi, nsample; xi0), all float64 on the host.  `fields`: the components ([N,N,N] float32
        device tensors); a vector gives the trace sum_c xi_cc.
        The power grid's float64 sum is xi(0) N^6; its k = 0 entry (|mean|^2 N^6) is set to 0 and the grid scaled by an exact
        power of two so that it sums to at most 1: every value of the second transform is then at most 1 in magnitude,
        whatever the caller's units, and the scale is undone exactly in float64.  A first bin that holds r = 0 alone takes the
        float64 sum itself, so that xi[0] is xi0 bit for bit; shells without a lattice point hold 0."""
        import math
        N, k = self.N, self.k
        grid = k.power_grid_full(fields, N)
        p0 = float(grid[0, 0, 0])
        grid[0, 0, 0] = 0
        body = float(grid.sum(dtype=torch.float64))
        if not math.isfinite(body) or not math.isfinite(p0):
            raise Exception("the power grid left the float32 range: rescale the field")
        e = math.frexp(body)[1] if body > 0 else 0          # body = m 2^e, 1/2 <= m < 1
        for part in (-e // 2, -e - (-e // 2)):              # (two exact factors: 2^-e itself may leave the float32 range)
            if part:
                grid.mul_(math.ldexp(1.0, part))
        self.prepare()
        buf = k.zeros((2 * self.nbins,), torch.float64)
        psum, nsample = buf[:self.nbins], buf[self.nbins:].view(torch.int64)
        k.bin_real(grid, N, psum, nsample)
        host = buf.cpu()
        ps = host[:self.nbins].numpy()
        ns = host[self.nbins:].view(torch.int64).numpy()
        n6 = float(N) ** 6
        with np.errstate(invalid="ignore", divide="ignore"):
            xi = np.ldexp(ps / ns, e) / n6
        xi[ns == 0] = 0
        xi0 = body / n6
        if self.edges[0] <= 0 and ns[0] == 1:
            xi[0] = xi0
        if not subtract_mean:
            xi[ns > 0] += p0 / n6
            xi0 += p0 / n6
            if self.edges[0] <= 0 and ns[0] == 1:
                xi[0] = xi0
        return np.column_stack((self.centers, xi, ns.astype(np.float64))), xi0
