// Stage A1 (nearest-grid-point deposition) and A3 (field algebra).
//
// Replaces deposit_to_grid (vpower/interp.py:996-1015), density_velocity_vector
// (:199-213) and the elementwise steps of ann_interp_to_field /
// BoxField.{momentum,kinetic_energy}_power (:272-273, 523-525, 546).
//
// Deposition is a bucket scheme built for HBM3E + 160 KiB LDS:
//   1. sort    : the particles' records {cell-in-bucket, payload[C]} are grouped by BUCKET (a brick of
//                bx*by*bz cells whose C float channels fit an LDS tile, or a z-pass pencil on the
//                fused path) by a two-level LDS bucket sort -- chunk histograms, one scan, LDS-staged
//                runs, one workgroup per coarse group (bucket_sort.h, shared with the NN cell list).  No global
//                atomic per particle, no random 20-byte writes.  A one-atomic-per-particle ranking
//                (rank_kernel / rank_scatter_kernel) remains for bucket counts or key ranges
//                the sort does not cover.
//   2. buckets : one workgroup per bucket adds its records into an LDS tile and then either streams
//                the WHOLE tile out with full-width coalesced stores (rows of bz cells), applying the
//                field algebra (v = rho v / rho, momentum, kinetic energy) on the way out
//                (brick_accumulate_kernel), or feeds it straight into the z-pass FFT
//                (pencil_fft_z_kernel, fft_pencil.h).
// Every cell of the slab is therefore written exactly once by plain stores: there is no
// grid memset, no global float atomic and no separate algebra pass.
//
// Cell indices must be BIT EXACT with numpy's  int((pos // Lcell) % N)  (SURVEY.md
// Q13): numpy evaluates floor_divide and remainder with its divmod algorithm in the
// dtype of `pos`, so that algorithm is restated here and this translation unit is
// compiled without floating-point contraction.
#pragma clang fp contract(off)

#include <type_traits>

#include "vps_internal.h"
#include "quantity.h"
#include "scan.h"
#include "bucket_sort.h"

namespace {

template <typename F>
__device__ __forceinline__ F dev_fmod(F a, F b);
template <>
__device__ __forceinline__ float dev_fmod<float>(float a, float b) { return fmodf(a, b); }
template <>
__device__ __forceinline__ double dev_fmod<double>(double a, double b) { return fmod(a, b); }

// numpy npy_divmod: the quotient part (numpy/_core/src/npymath/npy_math_internal.h.src)
template <typename F>
__device__ __forceinline__ F np_floor_divide(F a, F b) {
  F mod = dev_fmod<F>(a, b);
  F div = (a - mod) / b;
  if (mod != F(0)) {
    if ((b < F(0)) != (mod < F(0))) {
      mod += b;
      div -= F(1);
    }
  }
  F fd;
  if (div != F(0)) {
    fd = floor(div);
    if (div - fd > F(0.5)) fd += F(1);
  } else {
    fd = copysign(F(0), a / b);
  }
  return fd;
}

// fmod(q, n) for an integer-valued q and a positive integer n, both below 2^mantissa: one division.
// Exact: a non-integer q/n is at least 1/n away from every integer while its rounding error is below
// (q/n) 2^-mantissa < 1/n, so trunc() cannot cross one; trunc(q/n) n <= |q| and the remainder are exact.
// (fmod proper is a long routine, in double a very long one.)
template <typename F>
__device__ __forceinline__ F fmod_integral(F q, F n) {
  constexpr F lim = sizeof(F) == 4 ? F(16777216.0) : F(9007199254740992.0);
  if (fabs(q) < lim && n < lim) {
    const F r = q - trunc(q / n) * n;
    return copysign(r, q);          // fmod's zero carries the sign of the dividend
  }
  return dev_fmod<F>(q, n);
}

template <typename F>
__device__ __forceinline__ int cell_of(F x, F lcell, F nsize) {
  // int((x // Lcell) % N): float -> int cast truncates.
  // Fast path (every in-range input): numpy's floor_divide returns the exact floor of the real quotient
  // x / Lcell whenever that is far below 2^mantissa ((x - fmod) / Lcell is then an exact integer), and
  // the correctly rounded q = x / Lcell has the same floor unless q itself is an integer -- where the
  // sign of the exact residual fma(-q, Lcell, x) says whether the real quotient lies just below it.
  // The remainder of the integer fd by the integer N is one more division (exact: fd / N is at least
  // 1/N from any integer it does not equal, its rounding error below that).
  constexpr F lim = sizeof(F) == 4 ? F(4194304.0) : F(2251799813685248.0);   // 2^22, 2^51
  const F q = x / lcell;
  if (fabs(q) < lim && nsize < lim && lcell > F(0) && nsize >= F(1)) {
    F fd = floor(q);
    if (fd == q && fma(-q, lcell, x) < F(0)) fd -= F(1);
    return (int)(fd - floor(fd / nsize) * nsize);
  }
  // anything else (huge, inf, NaN): numpy's npy_divmod steps verbatim
  const F fdn = np_floor_divide<F>(x, lcell);
  F mod = fmod_integral<F>(fdn, nsize);
  if (mod != F(0)) {
    if ((nsize < F(0)) != (mod < F(0))) mod += nsize;
  } else {
    mod = copysign(F(0), nsize);
  }
  return (int)mod;
}

template <typename F>
__global__ void __launch_bounds__(256) cell_index_kernel(const F* __restrict__ pos, long long np,
                                                         F lcell, F nsize, int* __restrict__ cell) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) cell[i * 3 + a] = cell_of<F>(pos[i * 3 + a], lcell, nsize);
}

// ---- brick geometry ------------------------------------------------------------
struct Bricks {
  int N, x0, nx;        // grid and slab
  int bx, by, bz;       // brick extent in cells
  int nbx, nby, nbz;    // bricks per axis of the slab
  int cells;            // bx*by*bz
  int pow2, sy, sz;     // by, bz powers of two: log2(by), log2(bz)
};

// brick id and cell-in-brick of a particle, or false when it is outside the slab
template <typename F>
__device__ __forceinline__ bool locate(const F* __restrict__ pos, long long i, F lcell, F nsize,
                                       const Bricks& b, unsigned& brick, unsigned& loc) {
  const int cx = cell_of<F>(pos[i * 3 + 0], lcell, nsize) - b.x0;
  if (cx < 0 || cx >= b.nx) return false;
  const int cy = cell_of<F>(pos[i * 3 + 1], lcell, nsize);
  const int cz = cell_of<F>(pos[i * 3 + 2], lcell, nsize);
  if ((unsigned)cy >= (unsigned)b.N || (unsigned)cz >= (unsigned)b.N) return false;  // NaN / inf
  const int ix = cx / b.bx, iy = cy / b.by, iz = cz / b.bz;
  brick = (unsigned)((ix * b.nby + iy) * b.nbz + iz);
  loc = (unsigned)(((cx - ix * b.bx) * b.by + (cy - iy * b.by)) * b.bz + (cz - iz * b.bz));
  return true;
}

// brick id -> (ix, iy, iz): the brick's first cell is (ix bx, iy by, iz bz)
__device__ __forceinline__ void brick_index(const Bricks& b, long long brick, int& ix, int& iy, int& iz) {
  iz = (int)(brick % b.nbz);
  iy = (int)((brick / b.nbz) % b.nby);
  ix = (int)(brick / ((long long)b.nbz * b.nby));
}

// cell-in-brick word -> (lx, ly, lz), by shifts where by and bz are powers of two (SHIFTS = false: the scalar stream-out of the
// shapes that are no multiple of four divides, as it always did)
template <bool SHIFTS = true>
__device__ __forceinline__ void brick_cell(const Bricks& b, int loc, int& lx, int& ly, int& lz) {
  if (SHIFTS && b.pow2) {
    lz = loc & (b.bz - 1);
    ly = (loc >> b.sz) & (b.by - 1);
    lx = loc >> (b.sz + b.sy);
  } else {
    lz = loc % b.bz; ly = (loc / b.bz) % b.by; lx = loc / (b.bz * b.by);
  }
}

// ---- the two-level bucket sort (bucket_sort.h) as the deposit uses it ----------------------------------------------------
// Records {cell-in-bucket, payload[C]} grouped by bucket + start[], the same as rank -> scan -> scatter below gives, from the
// shared kernels: two particles per thread in level 1, final records that keep their cell-in-bucket word.
#ifndef VPS_SORT_ITEMS
#define VPS_SORT_ITEMS 2
#endif
constexpr int SORT_ITEMS = VPS_SORT_ITEMS;
constexpr int SORT_CHUNK = SORT_THREADS * SORT_ITEMS;

// key of particle i: bucket * cells + cell-in-bucket through `locate`, invalid outside the slab
template <typename F, typename K>
struct DepKeyOf {
  const F* __restrict__ pos;
  F lcell, nsize;
  Bricks b;
  __device__ __forceinline__ K operator()(long long i) const {
    unsigned brick, loc;
    return locate<F>(pos, i, lcell, nsize, b, brick, loc) ? (K)brick * (unsigned)b.cells + loc : sort_invalid<K>();
  }
};

// keys that are already there (the compacted slab; the block tails of the compaction are invalid)
template <typename K>
struct StoredKeyOf {
  const K* __restrict__ keys;
  __device__ __forceinline__ K operator()(long long i) const { return keys[i]; }
};

// ---- slab compaction ---------------------------------------------------------------------------------------------------
// A rank that holds a REPLICATED particle set but deposits one x-slab of it (scripts/parallel_optimized.py:272-276 loads the
// whole snapshot on every rank) first filters: one pass over the positions keeps the particles whose cell lies in the slab and
// writes their {key, [rho v, rho]} to compact arrays -- a workgroup reserves its output range with ONE global atomic.  The
// two-level sort then runs on the compact arrays only: its tables, chunks and records are sized for the slab, and the seven
// eighths of the particles that belong to other ranks are read once instead of twice.
// 256 threads, four consecutive particles per thread: their 12 coordinates are three 16-byte loads of one contiguous 12 KB
// block per workgroup; [rho v, rho] of the ones inside is requested BEFORE the workgroup's output range is reserved, so that
// those loads and the atomic's round trip overlap.
constexpr int COMPACT_THREADS = 256;
constexpr int COMPACT_ITEMS = 4;
constexpr int COMPACT_BLOCK = 2048;            // output slots reserved per atomic (>= the particles of one trip)
constexpr int COMPACT_MAXGRID = 2048;          // workgroups of the compaction launch (each may leave one block partly unused)
template <typename F, typename K>
__global__ void __launch_bounds__(COMPACT_THREADS)
    slab_compact_kernel(const F* __restrict__ pos, const float* __restrict__ vel, const float* __restrict__ rho, long long np,
                        F lcell, F nsize, Bricks b, SortGeom g, K* __restrict__ ckeys, float4* __restrict__ cpay,
                        unsigned long long* __restrict__ counter, long long cap) {
  __shared__ unsigned wcount[COMPACT_THREADS / 64];
  __shared__ unsigned long long blk_next;        // the block reserved for the part of a trip that does not fit the current one
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // Output slots come in BLOCKS of COMPACT_BLOCK reserved with one global atomic each (a returning atomic on one word peaks
  // near 90 per microsecond: one per trip -- 10^6 of them at 10^9 particles -- would take longer than reading the particles).
  // A trip whose records do not fit the rest of the current block spills into the next; what a workgroup leaves unused at the
  // end is filled with invalid keys, which the sort skips.
  unsigned long long blk_base = 0;               // (uniform over the workgroup, kept in registers)
  unsigned blk_used = COMPACT_BLOCK;             // nothing reserved yet
  constexpr long long PER = (long long)COMPACT_THREADS * COMPACT_ITEMS;
  const long long nchunk = (np + PER - 1) / PER;
  for (long long c = blockIdx.x; c < nchunk; c += gridDim.x) {
    const long long i0 = c * PER + (long long)threadIdx.x * COMPACT_ITEMS;      // this thread's first particle
    F q[3 * COMPACT_ITEMS];
    if (i0 + COMPACT_ITEMS <= np) {
      if constexpr (sizeof(F) == 4) {
        const float4* src = reinterpret_cast<const float4*>(pos + i0 * 3);       // (i0 * 3 floats = a multiple of 48 bytes)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float4 v4 = src[k];
          q[4 * k] = v4.x; q[4 * k + 1] = v4.y; q[4 * k + 2] = v4.z; q[4 * k + 3] = v4.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3 * COMPACT_ITEMS; ++k) q[k] = pos[i0 * 3 + k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3 * COMPACT_ITEMS; ++k) q[k] = (i0 * 3 + k < np * 3) ? pos[i0 * 3 + k] : F(0);
    }
    K key[COMPACT_ITEMS];
    bool in[COMPACT_ITEMS];
    float4 pay[COMPACT_ITEMS];
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < COMPACT_ITEMS; ++k) {
      const long long i = i0 + k;
      const int cx = cell_of<F>(q[3 * k], lcell, nsize) - b.x0;
      in[k] = i < np && cx >= 0 && cx < b.nx;
      key[k] = 0;
      if (in[k]) {
        const int cy = cell_of<F>(q[3 * k + 1], lcell, nsize), cz = cell_of<F>(q[3 * k + 2], lcell, nsize);
        in[k] = (unsigned)cy < (unsigned)b.N && (unsigned)cz < (unsigned)b.N;      // NaN / inf: nowhere (as `locate`)
        if (in[k]) {
          const int ix = cx / b.bx, iy = cy / b.by, iz = cz / b.bz;
          const unsigned brick = (unsigned)((ix * b.nby + iy) * b.nbz + iz);
          const unsigned loc = (unsigned)(((cx - ix * b.bx) * b.by + (cy - iy * b.by)) * b.bz + (cz - iz * b.bz));
          key[k] = (K)brick * g.cells + loc;
          const float r = rho[i];
          pay[k] = make_float4(vel[i * 3 + 0] * r, vel[i * 3 + 1] * r, vel[i * 3 + 2] * r, r);
          ++mine;
        }
      }
    }
    // slots: thread-major inside the workgroup (a thread's particles are consecutive), one atomic per workgroup and trip
    unsigned incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) wcount[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < COMPACT_THREADS / 64; ++w) {
      const unsigned t = wcount[w];
      if (w < wave) before += t;
      total += t;
    }
    const bool spill = blk_used + total > (unsigned)COMPACT_BLOCK;        // (uniform; total <= PER <= COMPACT_BLOCK)
    if (spill && threadIdx.x == 0) blk_next = atomicAdd(counter, (unsigned long long)COMPACT_BLOCK);
    __syncthreads();
    const unsigned long long nb = spill ? blk_next : blk_base;
    unsigned p_ = before + incl - mine;            // this thread's first record inside the trip
#pragma unroll
    for (int k = 0; k < COMPACT_ITEMS; ++k) {
      if (in[k]) {
        const unsigned at = blk_used + p_;
        const unsigned long long slot = at < (unsigned)COMPACT_BLOCK ? blk_base + at : nb + (at - COMPACT_BLOCK);
        if ((long long)slot < cap) {
          ckeys[slot] = key[k];
          cpay[slot] = pay[k];
        }
        ++p_;
      }
    }
    if (spill) {
      blk_used = blk_used + total - COMPACT_BLOCK;
      blk_base = nb;
    } else {
      blk_used += total;
    }
    __syncthreads();   // wcount / blk_next are rewritten by the next trip
  }
  // the unused tail of the last block: invalid keys
  if (blk_used < (unsigned)COMPACT_BLOCK)
    for (unsigned at = blk_used + threadIdx.x; at < (unsigned)COMPACT_BLOCK; at += COMPACT_THREADS)
      if ((long long)(blk_base + at) < cap) ckeys[blk_base + at] = sort_invalid<K>();
}

// RHOV: the payload is built from velocity and density on the fly ([rho vx, rho vy, rho vz, rho], interp.py:199-213)
template <int C, bool RHOV>
__device__ __forceinline__ void load_payload(const float* __restrict__ payload, const float* __restrict__ rho,
                                             long long i, float val[C]) {
  if constexpr (RHOV) {
    static_assert(C == 4, "rho*v payload has four channels");
    const float r = rho[i];
    val[0] = payload[i * 3 + 0] * r;
    val[1] = payload[i * 3 + 1] * r;
    val[2] = payload[i * 3 + 2] * r;
    val[3] = r;
  } else if constexpr (C == 4) {
    const float4 p4 = *reinterpret_cast<const float4*>(payload + i * 4);
    val[0] = p4.x; val[1] = p4.y; val[2] = p4.z; val[3] = p4.w;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) val[c] = payload[i * C + c];
  }
}

template <int C_, bool RHOV>
struct DepPayload {
  static constexpr int C = C_;
  const float* __restrict__ payload;
  const float* __restrict__ rho;
  __device__ __forceinline__ void load(long long i, float val[C_]) const { load_payload<C_, RHOV>(payload, rho, i, val); }
};

// One-atomic-per-particle ranking with the key and payload functors of the sort (option sort_atomic, or a geometry the two-level
// sort does not cover).  Pass 1: one returning atomic per particle gives both the bucket histogram and the particle's rank inside
// its bucket; key = bucket * cells + cell-in-bucket (0xffff.. = nowhere).
template <typename KeyOf>
__global__ void __launch_bounds__(256)
    rank_kernel(KeyOf key_of, long long np, unsigned cells, unsigned* __restrict__ count,
                unsigned long long* __restrict__ keys, unsigned* __restrict__ ranks) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const unsigned long long key = key_of(i);
  keys[i] = key;
  if (key != ~0ull) ranks[i] = atomicAdd(&count[key / cells], 1u);
}

// Pass 2 (after the scan): record = {loc, payload[C]} as (C+1) 32-bit words goes to slot start[bucket] + rank.
template <typename Payload>
__global__ void __launch_bounds__(256)
    rank_scatter_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ ranks, Payload pay,
                        long long np, unsigned cells, const unsigned* __restrict__ start, unsigned* __restrict__ records) {
  constexpr int C = Payload::C;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const unsigned long long key = keys[i];
  if (key == ~0ull) return;
  float val[C];
  pay.load(i, val);
  unsigned* rec = records + (size_t)(start[key / cells] + ranks[i]) * (C + 1);
  rec[0] = (unsigned)(key % cells);
#pragma unroll
  for (int c = 0; c < C; ++c) rec[1 + c] = __float_as_uint(val[c]);
}

// Epilogue of the brick kernel: what is written for a cell from its C accumulated channels.
//   EPI_RAW      : the C channels as they are (deposit_to_grid)
//   EPI_ALGEBRA  : channels are [rho vx, rho vy, rho vz, rho] -> fields of `quantity`
enum { EPI_RAW = 0, EPI_ALGEBRA = 1 };

__device__ __forceinline__ void algebra_cell(float a, float b, float c, float rho, int quantity, int flags,
                                             float vol, float out[4]) {
  // v = (rho v)/rho; empty cells give 0 (the NaN->0 rule of interp.py:329-331)
  float vx, vy, vz, m;
  if (flags & VPS_FLAG_INPUT_IS_VM) {
    vx = a; vy = b; vz = c; m = rho;
  } else {
    // one hardware reciprocal per cell (v_rcp_f32, 1 ulp; the result is compared at 2e-5 with a
    // float64 reference) instead of three IEEE divisions (about a dozen instructions each)
    const float inv = rho != 0.f ? __builtin_amdgcn_rcpf(rho) : 0.f;
    vx = a * inv;
    vy = b * inv;
    vz = c * inv;
    m = rho * vol;
  }
  if (quantity == VPS_MOMENTUM) {
    if (!(flags & VPS_FLAG_INPUT_IS_VM)) {
      // p = v m = (rho v) vol: one rounding instead of three, no reciprocal -- what the pencil kernel's momentum launch forms
      // (exact whenever the cell total and vol are: integer data, L = 1, N a power of two).  Every caller of this epilogue
      // with [rho v, rho] channels gets it: vps_deposit_field, vps_field_algebra[_out], the NN-resample route.  A cell
      // without mass stays 0 whatever its rho v channels hold, as with v = (rho v) * 0.
      vx = a; vy = b; vz = c; m = rho != 0.f ? vol : 0.f;
    }
    out[0] = vx * m;
    out[1] = ((flags & VPS_FLAG_REFERENCE_MOMENTUM_BUG) ? vx : vy) * m;
    out[2] = ((flags & VPS_FLAG_REFERENCE_MOMENTUM_BUG) ? vx : vz) * m;
    out[3] = (flags & VPS_FLAG_INPUT_IS_VM) ? m : rho * vol;
  } else if (quantity == VPS_ENERGY) {
    out[0] = m * ((vx * vx + vy * vy) + vz * vz);
    out[1] = out[2] = 0.f;
    out[3] = m;
  } else {  // VPS_VELOCITY, VPS_VM
    out[0] = vx; out[1] = vy; out[2] = vz; out[3] = m;
  }
}

// Density-weighted velocity w = rho^alpha v (VPS_WEIGHTED_VELOCITY), 0 where there is no mass whatever alpha is.  The power is
// exp2(e log2 rho) on the transcendental units (quantity.h: vps_rho_weight, as in the pencil kernel and the NN emit):
//   channels [rho v, rho]:               w = (rho v) rho^(alpha - 1)
//   VPS_FLAG_INPUT_IS_VM [v, mass]:      w = v (mass / vol)^alpha
// alpha - 1 is formed HERE, in float, from the float alpha; the NN and pencil routes get (float)(alpha - 1.0) from the host's
// double.  The two differ in the last bit for some alpha (1/3): each route keeps the rounding it was introduced with.
__device__ __forceinline__ void weighted_cell(float a, float b, float c, float rho, int flags, float vol, float alpha,
                                              float out[4]) {
  float f;
  if (flags & VPS_FLAG_INPUT_IS_VM) {
    const float r = rho * __builtin_amdgcn_rcpf(vol);
    f = rho != 0.f ? vps_rho_weight_nz(r, alpha) : 0.f;   // (empty means no MASS, whatever r rounds to)
  } else {
    f = vps_rho_weight(rho, alpha - 1.f);
  }
  // (a zero factor must give 0, not NaN, for whatever the empty cell's velocity channels hold)
  out[0] = f != 0.f ? a * f : 0.f;
  out[1] = f != 0.f ? b * f : 0.f;
  out[2] = f != 0.f ? c * f : 0.f;
  out[3] = 0.f;
}

// What one cell of `QUANT` is made of, for every kernel that forms quantities from four channels: [rho v, rho] cell totals, or
// [v, mass] of a gridded field with VPS_FLAG_INPUT_IS_VM.  out[0 .. vps_quantity_channels(QUANT)) is the quantity.
//   par.vol   the cell volume -- for the scalar density quantities its INVERSE (all they need one for: rho = mass * inv_vol of a
//             [v, mass] field; rho is channel 3 itself otherwise)
//   par.alpha the exponent of VPS_WEIGHTED_VELOCITY / VPS_DENSITY
//   s2        the cell's second moment sum w rho_p |v_p|^2, for the quantities that need one (vps_quantity_second_moment: the
//             5-channel kernels pass it, nobody else has one)
struct CellPar {
  float vol, alpha;
};
// The contribution rho_p |v_p|^2 of one [rho v, rho] record to the second moment, formed in the accumulating lane: a correctly
// rounded division (exact for integer v and a power of two rho), 0 for a record without mass.
__device__ __forceinline__ float second_moment_term(float px, float py, float pz, float rho) {
  return rho != 0.f ? ((px * px + py * py) + pz * pz) / rho : 0.f;
}
template <int QUANT>
__device__ __forceinline__ void cell_quantity(float a, float b, float c, float rho, int flags, CellPar par, float out[4],
                                              float s2 = 0.f) {
  static_assert(vps_quantity_valid(QUANT), "a quantity code of include/vps_hip.h");
  if constexpr (vps_quantity_second_moment(QUANT)) {
    // VPS_TOTAL_ENERGY vol S2; VPS_SUBGRID_ENERGY vol (S2 - |P|^2 / R); VPS_DISPERSION (S2 - |P|^2 / R) / R.  d = S2 - |P|^2 / R
    // with the resolved part as second_moment_term of the cell totals: in a cell with ONE NGP contribution that is the same
    // expression of the same numbers as S2 and d is exactly 0.  Clamped at 0 (rounding can take the difference below it); a
    // cell without mass has S2 = 0 and gives 0.
    // The sub-grid ENERGY is the complement of VPS_ENERGY: where d > 0 it is vol S2 minus the resolved energy AS VPS_ENERGY
    // FORMS IT (algebra_cell, bit for bit: a hardware reciprocal and nine roundings of its own), so that
    // VPS_ENERGY + VPS_SUBGRID_ENERGY = VPS_TOTAL_ENERGY holds to the rounding of this one subtraction and not to the error of
    // the two epilogues against each other.
    if constexpr (QUANT == VPS_TOTAL_ENERGY) {
      out[0] = par.vol * s2;
    } else {
      const float d = s2 - second_moment_term(a, b, c, rho);
      if constexpr (QUANT == VPS_SUBGRID_ENERGY) {
        float e[4];
        algebra_cell(a, b, c, rho, VPS_ENERGY, 0, par.vol, e);
        out[0] = d > 0.f ? fmaxf(par.vol * s2 - e[0], 0.f) : 0.f;
      } else {
        out[0] = (d > 0.f && rho != 0.f) ? d / rho : 0.f;
      }
    }
    out[1] = out[2] = out[3] = 0.f;
  } else if constexpr (vps_quantity_scalar_rho(QUANT)) {
    out[0] = vps_rho_scalar((flags & VPS_FLAG_INPUT_IS_VM) ? rho * par.vol : rho, QUANT, par.alpha);
    out[1] = out[2] = out[3] = 0.f;
  } else if constexpr (QUANT == VPS_WEIGHTED_VELOCITY) {
    weighted_cell(a, b, c, rho, flags, par.vol, par.alpha, out);
  } else {
    algebra_cell(a, b, c, rho, QUANT, flags, par.vol, out);
  }
}

// The tensor quantities (VPS_SUBGRID_STRESS, VPS_DISPERSION_TENSOR) are formed by two launches, one per HALF of the six
// components: the kernels' QUANT is the quantity code for the diagonal half (xx, yy, zz) and the code | TENSOR_OFFDIAG for the
// off-diagonal half (xy, xz, yz).  The bit exists between vps_deposit_field and its kernels only.
constexpr int TENSOR_OFFDIAG = 0x100;
// The contributions rho_p v_i v_j of one [rho v, rho] record to the three second moments of a half, each a correctly rounded
// division like second_moment_term (exact for integer v and a power of two rho), 0 for a record without mass.  The epilogue
// forms the resolved part P_i P_j / R with the SAME function of the cell totals.
template <bool OFFDIAG>
__device__ __forceinline__ void tensor_terms(float px, float py, float pz, float rho, float m[3]) {
  if (rho != 0.f) {
    m[0] = (OFFDIAG ? px * py : px * px) / rho;
    m[1] = (OFFDIAG ? px * pz : py * py) / rho;
    m[2] = (OFFDIAG ? py * pz : pz * pz) / rho;
  } else {
    m[0] = m[1] = m[2] = 0.f;
  }
}
// One half of a tensor quantity in one cell: d = S_ij - P_i P_j / R from the half's three second moments m0..m2 and the four
// totals; VPS_SUBGRID_STRESS vol d, VPS_DISPERSION_TENSOR d / R.  A diagonal component is clamped at 0 from below (rounding can
// take the difference below it), an off-diagonal one has either sign; a cell without mass gives 0.  In a cell with one NGP
// contribution both sides are the same expression of the same numbers and d is exactly 0.
template <int QUANT>
__device__ __forceinline__ void cell_tensor(float a, float b, float c, float rho, float vol, float m0, float m1, float m2,
                                            float out[4]) {
  constexpr bool OFFDIAG = (QUANT & TENSOR_OFFDIAG) != 0;
  static_assert(vps_quantity_tensor(QUANT & ~TENSOR_OFFDIAG), "a tensor quantity code, with or without the half bit");
  float r[3];
  tensor_terms<OFFDIAG>(a, b, c, rho, r);
  const float m[3] = {m0, m1, m2};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = m[k] - r[k];
    const bool keep = rho != 0.f && (OFFDIAG || d > 0.f);
    if constexpr ((QUANT & ~TENSOR_OFFDIAG) == VPS_SUBGRID_STRESS) out[k] = keep ? vol * d : 0.f;
    else out[k] = keep ? d / rho : 0.f;
  }
  out[3] = 0.f;
}

// run-time quantity code -> template argument: f(std::integral_constant<int, QUANT>) of the (valid) code.  SECOND_MOMENT: the
// caller's kernels carry the second-moment tile channels (the two deposit kernels of vps_deposit_field); everybody else has no
// instantiation for those codes and gets VPS_ERR_ARG.
template <bool SECOND_MOMENT = false, typename Fn>
int dispatch_quantity(int quantity, Fn&& f) {
  switch (quantity) {
#define VPS_Q(Q) case Q: return f(std::integral_constant<int, Q>{})
    VPS_Q(VPS_VELOCITY); VPS_Q(VPS_MOMENTUM); VPS_Q(VPS_ENERGY); VPS_Q(VPS_VM);
    VPS_Q(VPS_WEIGHTED_VELOCITY); VPS_Q(VPS_DENSITY); VPS_Q(VPS_LOG_DENSITY);
  }
  if constexpr (SECOND_MOMENT) {
    switch (quantity) {
      VPS_Q(VPS_TOTAL_ENERGY); VPS_Q(VPS_SUBGRID_ENERGY); VPS_Q(VPS_DISPERSION);
      VPS_Q(VPS_SUBGRID_STRESS); VPS_Q(VPS_DISPERSION_TENSOR);
    }
  }
#undef VPS_Q
  return VPS_ERR_ARG;
}

// LDS tile of a deposit kernel that forms `quantity` from C record channels over `cells` cells: one more channel for the
// second moment (80 KiB where the 4-channel tile has 64: the launch raises the kernel's limit first), three more for one half of
// a tensor quantity (56 KiB, 112 KiB from N = 1024 on).
size_t tile_bytes(int C, int cells, int quantity) {
  return (size_t)(C + vps_quantity_moment_channels(quantity)) * cells * sizeof(float);
}
// ... and a context whose LDS does not hold the 5-channel (7-channel) tile refuses the quantity
int check_second_moment_tile(vps_ctx* ctx, int quantity, size_t lds) {
  if (vps_quantity_second_moment(quantity) && lds > ctx->lds_per_cu)
    return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_deposit_field: quantity %d (%s) needs an LDS tile of %zu bytes, the device has %zu per CU",
                    quantity, vps_second_moment_name(quantity), lds, ctx->lds_per_cu);
  return VPS_OK;
}

// ---- the stream-out of an LDS tile [CT][cells], shared by the brick kernels of every route -------------------------------------
// What the kernel's epilogue is made of, at compile time: C record channels, CT tile channels (the second-moment quantities keep
// S2 = sum w rho_p |v_p|^2 in a channel of its own behind the C record channels: the records stay [rho v, rho]), NOUT written.
// A tensor quantity's launch keeps the three second moments of its half (QUANT's TENSOR_OFFDIAG bit) there and writes three.
template <int C, int EPI, int QUANT>
struct TileOut {
  static constexpr int CODE = QUANT & ~TENSOR_OFFDIAG;
  static constexpr bool M2 = EPI == EPI_ALGEBRA && vps_quantity_second_moment(CODE);
  static constexpr bool TENSOR = EPI == EPI_ALGEBRA && vps_quantity_tensor(CODE);
  static constexpr bool OFFDIAG = TENSOR && (QUANT & TENSOR_OFFDIAG) != 0;
  static constexpr int CT = M2 ? C + vps_quantity_moment_channels(CODE) : C;
  static constexpr int NOUT = (EPI == EPI_RAW) ? C : TENSOR ? 3 : vps_quantity_channels(CODE);
  // what the direct gather adds behind the C record channels: nothing, the trace, a tensor half (assign_gather)
  static constexpr int MOMENT = TENSOR ? (OFFDIAG ? 3 : 2) : M2 ? 1 : 0;
  static_assert(EPI == EPI_RAW || C == 4, "quantities are formed from [rho v, rho] records");
};
// (algebra_cell reads the flags at run time, as it always did; the quantities of rho see their constant 0)
template <int QUANT>
__device__ __forceinline__ int tile_cflags(int flags) {
  return (vps_quantity_needs_alpha(QUANT) || vps_quantity_scalar_rho(QUANT)) ? 0 : flags;
}
typedef float vf4 __attribute__((ext_vector_type(4)));

// Four consecutive cells from `loc` on: their CT channels are read and zeroed; if the quad is inside the grid its NOUT fields go
// to out[c * plane + cell].  The quantity fields leave by streaming stores (the grid is written once; the cache should keep the
// records: -33 %).  The raw channels do so with STREAM only: the NGP deposit has always written them with plain stores, the
// direct one with streaming stores, and each keeps its own.
template <int C, int EPI, int QUANT, bool STREAM>
__device__ __forceinline__ void tile_out4(float* tile, int cells, int loc, bool inside, int cflags, CellPar cpar,
                                          float* __restrict__ out, long long plane, long long cell) {
  typedef TileOut<C, EPI, QUANT> T;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (EPI == EPI_RAW) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float4* t = reinterpret_cast<float4*>(tile + c * cells + loc);
      const float4 val = *t;
      *t = zero4;
      if (inside) {
        if constexpr (STREAM) {
          vf4 q; q.x = val.x; q.y = val.y; q.z = val.z; q.w = val.w;
          __builtin_nontemporal_store(q, reinterpret_cast<vf4*>(out + c * plane + cell));
        } else {
          *reinterpret_cast<float4*>(out + c * plane + cell) = val;
        }
      }
    }
  } else {
    float4* t0 = reinterpret_cast<float4*>(tile + loc);
    float4* t1 = reinterpret_cast<float4*>(tile + cells + loc);
    float4* t2 = reinterpret_cast<float4*>(tile + 2 * cells + loc);
    float4* t3 = reinterpret_cast<float4*>(tile + 3 * cells + loc);
    const float4 c0 = *t0, c1 = *t1, c2 = *t2, c3 = *t3;
    *t0 = zero4; *t1 = zero4; *t2 = zero4; *t3 = zero4;
    float4 c4 = zero4;                       // the second moment (M2 only: a constant elsewhere)
    if constexpr (T::M2) {
      float4* t4 = reinterpret_cast<float4*>(tile + 4 * cells + loc);
      c4 = *t4;
      *t4 = zero4;
    }
    float4 c5 = zero4, c6 = zero4;           // the second and third moment of a tensor half
    if constexpr (T::TENSOR) {
      float4* t5 = reinterpret_cast<float4*>(tile + 5 * cells + loc);
      float4* t6 = reinterpret_cast<float4*>(tile + 6 * cells + loc);
      c5 = *t5; c6 = *t6;
      *t5 = zero4; *t6 = zero4;
    }
    if (inside) {
      float rx[4], ry[4], rz[4], rw[4];
      if constexpr (T::TENSOR) {
        cell_tensor<QUANT>(c0.x, c1.x, c2.x, c3.x, cpar.vol, c4.x, c5.x, c6.x, rx);
        cell_tensor<QUANT>(c0.y, c1.y, c2.y, c3.y, cpar.vol, c4.y, c5.y, c6.y, ry);
        cell_tensor<QUANT>(c0.z, c1.z, c2.z, c3.z, cpar.vol, c4.z, c5.z, c6.z, rz);
        cell_tensor<QUANT>(c0.w, c1.w, c2.w, c3.w, cpar.vol, c4.w, c5.w, c6.w, rw);
      } else {
        cell_quantity<QUANT>(c0.x, c1.x, c2.x, c3.x, cflags, cpar, rx, c4.x);
        cell_quantity<QUANT>(c0.y, c1.y, c2.y, c3.y, cflags, cpar, ry, c4.y);
        cell_quantity<QUANT>(c0.z, c1.z, c2.z, c3.z, cflags, cpar, rz, c4.z);
        cell_quantity<QUANT>(c0.w, c1.w, c2.w, c3.w, cflags, cpar, rw, c4.w);
      }
#pragma unroll
      for (int c = 0; c < T::NOUT; ++c) {
        vf4 q; q.x = rx[c]; q.y = ry[c]; q.z = rz[c]; q.w = rw[c];
        __builtin_nontemporal_store(q, reinterpret_cast<vf4*>(out + c * plane + cell));
      }
    }
  }
}

// ... and its scalar twin for the bricks and grids that are no multiple of four: one cell.  STREAM: every store of it.
template <int C, int EPI, int QUANT, bool STREAM>
__device__ __forceinline__ void tile_out1(float* tile, int cells, int loc, bool inside, int cflags, CellPar cpar,
                                          float* __restrict__ out, long long plane, long long cell) {
  typedef TileOut<C, EPI, QUANT> T;
  float v[T::CT], r[4];
#pragma unroll
  for (int c = 0; c < T::CT; ++c) {
    v[c] = tile[c * cells + loc];
    tile[c * cells + loc] = 0.f;
  }
  if (!inside) return;
  if constexpr (T::TENSOR) cell_tensor<QUANT>(v[0], v[1], v[2], v[3], cpar.vol, v[C], v[C + 1], v[C + 2], r);
  else if constexpr (EPI == EPI_ALGEBRA) cell_quantity<QUANT>(v[0], v[1], v[2], v[3], cflags, cpar, r, T::M2 ? v[T::CT - 1] : 0.f);
#pragma unroll
  for (int c = 0; c < T::NOUT; ++c) {
    const float val = EPI == EPI_ALGEBRA ? r[c] : v[c];
    if constexpr (STREAM) __builtin_nontemporal_store(val, out + c * plane + cell);
    else out[c * plane + cell] = val;
  }
}

// QUANT is the (compile-time) quantity of the algebra epilogue; NOUT its channel count.  `par` is the ONE float that epilogue
// reads (brick_par): the channels are [rho v, rho] cell totals, never [v, mass], so a quantity needs the cell volume or alpha,
// not both.
template <int C, int EPI, int QUANT>
__global__ void __launch_bounds__(256)
    brick_accumulate_kernel(const unsigned* __restrict__ records, const unsigned* __restrict__ start,
                            Bricks b, long long nbricks, int flags, float par,
                            float* __restrict__ grid) {
  const int cflags = tile_cflags<QUANT>(flags);
  // One float, copied into both members: every quantity here reads exactly one of them.  QUANT < VPS_WEIGHTED_VELOCITY reads
  // par.vol (the volume) and never par.alpha; QUANT >= VPS_WEIGHTED_VELOCITY reads par.alpha and, with cflags = 0, never par.vol,
  // which is MEANINGLESS for them here (it holds alpha).  A two-float kernel argument would move this kernel's code.
  const CellPar cpar{par, par};
  // (the second-moment channel is compile time: nothing of it exists in the other instantiations)
  constexpr bool M2 = TileOut<C, EPI, QUANT>::M2;
  constexpr int CT = TileOut<C, EPI, QUANT>::CT;
  // Persistent workgroups walk the bricks: the streaming stores of one brick stay in flight
  // while the next bucket is being accumulated, and the tile is re-zeroed as it is read.
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tile = reinterpret_cast<float*>(smem_raw);  // [CT][cells]
  const int cells = b.cells;
  const bool vec4 = ((b.bz & 3) == 0) && ((b.N & 3) == 0);
  if ((cells & 3) == 0) {
    for (int i = threadIdx.x; i < CT * cells / 4; i += blockDim.x)
      reinterpret_cast<float4*>(tile)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int i = threadIdx.x; i < CT * cells; i += blockDim.x) tile[i] = 0.f;
  }
  const long long plane = (long long)b.nx * b.N * b.N;
  long long brick = blockIdx.x;
  unsigned s = 0, e = 0;
  if (brick < nbricks) {
    s = start[brick];
    e = start[brick + 1];
  }
  __syncthreads();
  for (; brick < nbricks; brick += gridDim.x) {
    for (unsigned j = s + threadIdx.x; j < e; j += blockDim.x) {
      const unsigned* rec = records + (size_t)j * (C + 1);
      const unsigned loc = rec[0];
#pragma unroll
      for (int c = 0; c < C; ++c) atomicAdd(&tile[c * cells + loc], __uint_as_float(rec[1 + c]));   // (vps_lds_add: slower here)
      if constexpr (TileOut<C, EPI, QUANT>::TENSOR) {
        float m[3];
        tensor_terms<TileOut<C, EPI, QUANT>::OFFDIAG>(__uint_as_float(rec[1]), __uint_as_float(rec[2]), __uint_as_float(rec[3]),
                                                      __uint_as_float(rec[4]), m);
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(&tile[(C + k) * cells + loc], m[k]);
      } else if constexpr (M2)
        atomicAdd(&tile[C * cells + loc], second_moment_term(__uint_as_float(rec[1]), __uint_as_float(rec[2]),
                                                             __uint_as_float(rec[3]), __uint_as_float(rec[4])));
    }
    // bucket bounds of the next brick: in flight during the stream-out below
    const long long nb = brick + gridDim.x;
    if (nb < nbricks) {
      s = start[nb];
      e = start[nb + 1];
    }
    __syncthreads();
    // stream the tile out: rows of bz cells are contiguous in the grid
    int ix, iy, iz;
    brick_index(b, brick, ix, iy, iz);
    const int gx0 = ix * b.bx, gy0 = iy * b.by, gz0 = iz * b.bz;
    if (vec4) {
      const int q4 = cells / 4;
      for (int i = threadIdx.x; i < q4; i += blockDim.x) {
        const int loc = i * 4;
        int lz, ly, lx;
        brick_cell(b, loc, lx, ly, lz);
        const int gx = gx0 + lx, gy = gy0 + ly, gz = gz0 + lz;
        const bool inside = gx < b.nx && gy < b.N && gz < b.N;   // partial bricks at the slab edge
        const long long cell = ((long long)gx * b.N + gy) * b.N + gz;
        tile_out4<C, EPI, QUANT, false>(tile, cells, loc, inside, cflags, cpar, grid, plane, cell);
      }
    } else {
      for (int loc = threadIdx.x; loc < cells; loc += blockDim.x) {
        int lz, ly, lx;
        brick_cell<false>(b, loc, lx, ly, lz);
        const int gx = gx0 + lx, gy = gy0 + ly, gz = gz0 + lz;
        const bool inside = gx < b.nx && gy < b.N && gz < b.N;
        const long long cell = ((long long)gx * b.N + gy) * b.N + gz;
        tile_out1<C, EPI, QUANT, false>(tile, cells, loc, inside, cflags, cpar, grid, plane, cell);
      }
    }
    __syncthreads();   // tile is all zero again
  }
}

// The quantity of an existing 4-channel grid (used after the NN resample and by BoxField.spctrm on user-supplied fields): its
// vps_quantity_channels(QUANT) channels, four cells per thread.
// `out` == nullptr: in place; else the channels of the result go to out[c][ncell] and ch is only read
// (a second quantity of the same field: no copy of the four input channels is needed).
// The scalar density quantities read channel 3 alone: rho itself, or mass * inv_vol with VPS_FLAG_INPUT_IS_VM (cell_quantity).
template <int QUANT>
__global__ void __launch_bounds__(256)
    field_quantity_kernel(float* ch, long long ncell, int flags, CellPar par, float* out) {
  constexpr int NCH = vps_quantity_channels(QUANT);
  const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= ncell) return;
  float* dst = out ? out : ch;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
  if constexpr (!vps_quantity_scalar_rho(QUANT)) {
    a = *reinterpret_cast<float4*>(ch + i0);
    b = *reinterpret_cast<float4*>(ch + ncell + i0);
    c = *reinterpret_cast<float4*>(ch + 2 * ncell + i0);
  }
  float4 m = *reinterpret_cast<float4*>(ch + 3 * ncell + i0);
  float r[4];
  cell_quantity<QUANT>(a.x, b.x, c.x, m.x, flags, par, r);
  a.x = r[0]; b.x = r[1]; c.x = r[2]; m.x = r[3];
  cell_quantity<QUANT>(a.y, b.y, c.y, m.y, flags, par, r);
  a.y = r[0]; b.y = r[1]; c.y = r[2]; m.y = r[3];
  cell_quantity<QUANT>(a.z, b.z, c.z, m.z, flags, par, r);
  a.z = r[0]; b.z = r[1]; c.z = r[2]; m.z = r[3];
  cell_quantity<QUANT>(a.w, b.w, c.w, m.w, flags, par, r);
  a.w = r[0]; b.w = r[1]; c.w = r[2]; m.w = r[3];
  *reinterpret_cast<float4*>(dst + i0) = a;
  if constexpr (NCH >= 3) {
    *reinterpret_cast<float4*>(dst + ncell + i0) = b;
    *reinterpret_cast<float4*>(dst + 2 * ncell + i0) = c;
  }
  if constexpr (NCH == 4) *reinterpret_cast<float4*>(dst + 3 * ncell + i0) = m;
}

// [rho vx, rho vy, rho vz, rho] per particle (interp.py:199-213)
__global__ void __launch_bounds__(256)
    rhov_kernel(const float* __restrict__ vel, const float* __restrict__ rho, long long np,
                float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  const float r = rho[i];
  *reinterpret_cast<float4*>(out + i * 4) =
      make_float4(vel[i * 3 + 0] * r, vel[i * 3 + 1] * r, vel[i * 3 + 2] * r, r);
}

// Periodic image in [0, N) of an integer-valued cell number held in float64, taken BEFORE the conversion to int: positions far
// outside the box (1e10, -2.9e8 cells: the NGP route wraps them, cell_of) give cell numbers beyond 2^31, whose conversion is
// not the number.  Exact below 2^53: c / n is at least 1/n from any integer it does not equal and its rounding error is
// below that, floor(c / n) n <= |c| and the remainder are exact.  In-range cell numbers come out as they went in.
__device__ __forceinline__ int wrap_cell(double c, double n) { return (int)(c - floor(c / n) * n); }

// Higher-order mass assignment (cloud-in-cell: 2 cells per axis, triangular-shaped-cloud: 3): every particle becomes
// S = 8 or 27 weighted sub-particles sitting at the centres of the cells it touches (periodic), which the NGP
// deposit then adds up -- no new deposit kernel, and with replicated particles no halo exchange between slabs.
// Not in the reference (it offers NGP interp.py:996, NN :1018 and Voxelize :280); SURVEY.md section 8(f-4).
// The cell coordinate s = x / Lcell (a division: the correctly rounded quotient, whatever the size of x) and the axis weights
// are formed in float64 and each weight is rounded to float32 ONCE: a weight is then right to 2^-24 of ITSELF, however small
// (1 - f next to a cell centre, (1/2 - d)^2 next to a face), where float32 arithmetic on a rounded offset is right to 2^-25
// of the offset only.  The kernel moves 27 records per particle; the few float64 operations per axis do not show.
template <typename F>
__global__ void __launch_bounds__(256)
    assign_expand_kernel(const F* __restrict__ pos, const float* __restrict__ payload, long long np, int C, int N,
                         double lcell, int order, float* __restrict__ pos_out, float* __restrict__ payload_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np) return;
  int c0[3];
  float w[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s = (double)pos[i * 3 + a] / lcell;
    if (order == 2) {            // CIC: cells floor(s - 1/2) and the next one, weights 1 - f, f
      const double f0 = floor(s - 0.5);
      const double f = s - 0.5 - f0;
      c0[a] = wrap_cell(f0, (double)N);
      w[a][0] = (float)(1.0 - f);
      w[a][1] = (float)f;
      w[a][2] = 0.f;
    } else {                     // TSC: the cell holding the particle and its two neighbours
      const double ic = floor(s);
      const double d = s - (ic + 0.5);
      c0[a] = wrap_cell(ic - 1.0, (double)N);
      w[a][0] = (float)(0.5 * ((0.5 - d) * (0.5 - d)));
      w[a][1] = (float)(0.75 - d * d);
      w[a][2] = (float)(0.5 * ((0.5 + d) * (0.5 + d)));
    }
  }
  const int S1 = order, S = S1 * S1 * S1;
  float pay[4];
  for (int c = 0; c < C; ++c) pay[c] = payload[i * C + c];
  for (int j = 0; j < S; ++j) {
    const int jx = j / (S1 * S1), jy = (j / S1) % S1, jz = j % S1;
    const float wt = w[0][jx] * w[1][jy] * w[2][jz];
    const int cx = ((c0[0] + jx) % N + N) % N, cy = ((c0[1] + jy) % N + N) % N, cz = ((c0[2] + jz) % N + N) % N;
    float* po = pos_out + (i * S + j) * 3;
    po[0] = (float)(((double)cx + 0.5) * lcell);
    po[1] = (float)(((double)cy + 0.5) * lcell);
    po[2] = (float)(((double)cz + 0.5) * lcell);
    for (int c = 0; c < C; ++c) payload_out[(i * S + j) * C + c] = pay[c] * wt;
  }
}

// LDS tile of one brick: 32 KiB -> four bricks resident per CU, enough workgroups in
// flight to hide the bucket-read -> LDS-add -> stream-out dependency chain of each one.  From 1024^3 on twice that
// (8 x 8 x 64 cells, two bricks per CU): a brick's stores then cover 64 rows of 256 bytes per field instead of 32, and the
// sort has half the buckets -- measured (sort + accumulate & write, ms): 1024^3 / 5e7 particles 2.34 + 3.08 against
// 2.39 + 3.53; 2048^3 / 1e8 4.6 + 16.9 against 5.6 + 20.4 (103 GB written at 6.1 instead of 5.1 TB/s); 512^3 / 1e7 0.37 + 0.36
// against 0.38 + 0.34; 128 KiB (one brick per CU) 4.8 + 20.4; rows of 512 / 1024 bytes (bz = 128 / 256) 19.0 / 19.4 at 32 KiB.
#ifndef VPS_BRICK_LDS_BYTES
#define VPS_BRICK_LDS_BYTES (32 * 1024)
#endif
#ifndef VPS_BRICK_BZ
#define VPS_BRICK_BZ 64
#endif

int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

Bricks make_bricks(int N, int x0, int nx, int C) {
  Bricks b;
  b.N = N; b.x0 = x0; b.nx = nx;
  const int max_cells = ((N >= 1024 ? 2 : 1) * (VPS_BRICK_LDS_BYTES)) / (4 * C);
  b.bz = N < VPS_BRICK_BZ ? N : VPS_BRICK_BZ;          // up to 256-byte rows
  if (b.bz > max_cells) b.bz = max_cells;
  int rest = max_cells / b.bz;
  b.by = pow2_floor(rest < 8 ? (rest < 1 ? 1 : rest) : 8);
  if (b.by > N) b.by = N;
  rest = max_cells / (b.bz * b.by);
  b.bx = pow2_floor(rest < 1 ? 1 : rest);
  if (b.bx > nx) b.bx = nx;
  b.nbx = (nx + b.bx - 1) / b.bx;
  b.nby = (N + b.by - 1) / b.by;
  b.nbz = (N + b.bz - 1) / b.bz;
  b.cells = b.bx * b.by * b.bz;
  b.pow2 = ((b.by & (b.by - 1)) == 0) && ((b.bz & (b.bz - 1)) == 0);
  b.sy = b.sz = 0;
  while ((1 << b.sy) < b.by) ++b.sy;
  while ((1 << b.sz) < b.bz) ++b.sz;
  return b;
}

// pencil buckets of the fused deposit -> z-pass path: (x, TP y-lines, all z)
Bricks make_pencils(int N, int x0, int nx, int TP) {
  Bricks b;
  b.N = N; b.x0 = x0; b.nx = nx;
  b.bx = 1; b.by = TP; b.bz = N;
  b.nbx = nx; b.nby = N / TP; b.nbz = 1;
  b.cells = TP * N;
  b.pow2 = 1;
  b.sy = b.sz = 0;
  while ((1 << b.sy) < b.by) ++b.sy;
  while ((1 << b.sz) < b.bz) ++b.sz;
  return b;
}

struct DepLayout {
  size_t count, start, tiles, keys, ranks, records, table, table_start, table_tiles, rec1, total;
  long long nbricks;
  long long cap;    // records the workspace has room for: np, or the caller's bound on the particles inside the slab
  long long cap_in; // entries of the compacted input arrays (cap + the block tails of slab_compact_kernel)
  bool recompute;   // cap < np: the slab's particles are compacted first (slab_compact_kernel); keys[] / cpay hold cap entries
  size_t cpay, counter;
  bool two_level;
  bool wide_keys;   // bucket * cells + cell does not fit 32 bits: 64-bit keys[] (the level-1 records stay 32-bit, see SortGeom)
  SortGeom geom;
};

// groups per launch the two-level sort aims for (level-2 workgroups); option sort_groups overrides (tuning)
int sort_target_groups() {
  int v = (int)vps_option("sort_groups", 512);
  if (v < 1) v = 1;
  if (v > 4096) v = 4096;
  return v;
}

bool sort_staged() { return vps_option("sort_staged", 1) != 0; }

// option sort_atomic forces the one-atomic-per-particle ranking (kept for bucket counts / key ranges the
// two-level sort does not cover, and as a cross-check in the tests)
bool sort_force_atomic() { return vps_option("sort_atomic", 0) != 0; }

// np_cap >= 0: the caller's bound on the number of particles inside the slab (vps_count_in_slab): the record arrays are sized
// for it and the key array disappears -- for ranks that hold a replicated particle set but deposit one slab of it
DepLayout dep_layout(int64_t np, int C, const Bricks& b, int64_t np_cap = -1) {
  DepLayout l;
  l.nbricks = (long long)b.nbx * b.nby * b.nbz;
  SortGeom& g = l.geom;
  g.cells = (unsigned)b.cells;
  g.cshift = -1;
  if ((b.cells & (b.cells - 1)) == 0) {
    g.cshift = 0;
    while ((1 << g.cshift) < b.cells) ++g.cshift;
  }
  g.nbuckets = l.nbricks;
  g.gshift = 3;
  while (((l.nbricks + (1ll << g.gshift) - 1) >> g.gshift) > sort_target_groups()) ++g.gshift;
  // more buckets than target x 4096 (the bricks of a 2048^3 grid: 4.2e6): rather more level-1 groups than the
  // one-atomic-per-particle ranking -- measured at 2048^3 / 1e8 particles: 5.4 ms with 1024 groups against 8.4 ms
  // (6.2 with 2048 groups, 8.6 with 4096: the group tables grow with them)
  if (g.gshift > 12 && ((l.nbricks + 4095) >> 12) <= 2048) g.gshift = 12;
  g.ngroups = (int)((l.nbricks + (1ll << g.gshift) - 1) >> g.gshift);
  g.nchunks = (np + SORT_CHUNK - 1) / SORT_CHUNK;     // (slab-sized workspaces: re-set below)
  l.wide_keys = (unsigned long long)l.nbricks * (unsigned long long)b.cells >= 0xffffffffull;
  l.two_level = !sort_force_atomic() && g.gshift <= 12 && l.nbricks < 0x7fffffffLL &&
                ((unsigned long long)b.cells << g.gshift) < 0xffffffffull;
  l.recompute = np_cap >= 0 && np_cap < np && l.two_level && sort_staged() && sort_staged_lds(g, C, SORT_ITEMS) <= 160 * 1024 && C == 4;
  l.cap = l.recompute ? np_cap : np;
  // compacted arrays: the slab's particles + one partly used block per workgroup of the compaction launch
  {
    const long long trips = (np + (long long)COMPACT_THREADS * COMPACT_ITEMS - 1) / ((long long)COMPACT_THREADS * COMPACT_ITEMS);
    const long long slack = std::min<long long>(trips, COMPACT_MAXGRID) * COMPACT_BLOCK;
    if (l.recompute && l.cap + slack >= np / 2) {     // nothing to gain: sort all particles in place, as without a bound
      l.recompute = false;
      l.cap = np;
    }
    l.cap_in = l.recompute ? l.cap + slack : l.cap;
  }
  if (l.recompute) g.nchunks = (l.cap_in + SORT_CHUNK - 1) / SORT_CHUNK;     // the sort sees the compacted particles only
  const long long ntable = (long long)g.ngroups * g.nchunks;
  auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
  size_t off = 0;
  l.count = off;   off = align(off + sizeof(unsigned) * l.nbricks);
  l.start = off;   off = align(off + sizeof(unsigned) * (l.nbricks + 1));
  l.tiles = off;   off = align(off + sizeof(unsigned) * (scan_tiles(l.nbricks) + 1));
  l.keys = off;    off = align(off + (size_t)l.cap_in * sizeof(unsigned long long));
  l.cpay = l.counter = off;
  if (l.recompute) {
    l.cpay = off;    off = align(off + (size_t)l.cap_in * sizeof(float4));
    l.counter = off; off = align(off + sizeof(unsigned long long));
  }
  l.ranks = off;   off = align(off + (size_t)l.cap_in * sizeof(unsigned));
  l.records = off; off = align(off + (size_t)l.cap_in * (C + 1) * sizeof(unsigned));
  l.table = l.table_start = l.table_tiles = l.rec1 = off;
  if (l.two_level) {
    l.table = off;        off = align(off + sizeof(unsigned) * (ntable + 1));
    l.table_start = off;  off = align(off + sizeof(unsigned) * (ntable + 1));
    l.table_tiles = off;  off = align(off + sizeof(unsigned) * (scan_tiles(ntable) + 1));
    l.rec1 = off;         off = align(off + (size_t)l.cap_in * sort_rec1_words(C) * sizeof(unsigned));
  }
  l.total = off;
  return l;
}

// a kernel whose dynamic LDS exceeds the 64 KiB every kernel may have is allowed its `lds` bytes first
template <typename Kern>
int raise_lds_limit(vps_ctx* ctx, Kern kern, size_t lds) {
  if (lds > 64 * 1024)
    VPS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return VPS_OK;
}

// persistent workgroups of a brick kernel with an LDS tile of `lds` bytes: what a CU holds of them (1 .. 8), at most one per brick
unsigned brick_launch_grid(const vps_ctx* ctx, size_t lds, long long nbricks) {
  long long per_cu = (long long)(ctx->lds_per_cu / (lds ? lds : 1));
  if (per_cu > 8) per_cu = 8;
  if (per_cu < 1) per_cu = 1;
  return (unsigned)std::min<long long>((long long)ctx->num_cu * per_cu, nbricks);
}

// The sort driver of every deposit route: n particles -> records {cell-in-bucket, payload[Pay::C]} grouped by bucket +
// start[nbuckets + 1], in the workspace `l` lays out.  pay: the payload functor (DepPayload, AssignPayload); key_of(K{}): the key
// functor for keys of type K (DepKeyOf, StoredKeyOf, AssignKeyOf).  The caller holds the launch timer.
template <typename KeyMaker, typename Pay>
int sort_records(vps_ctx* ctx, KeyMaker key_of, const Pay& pay, long long n, const DepLayout& l, char* work) {
  constexpr int CR = Pay::C;
  unsigned* count = reinterpret_cast<unsigned*>(work + l.count);
  unsigned* start = reinterpret_cast<unsigned*>(work + l.start);
  unsigned* records = reinterpret_cast<unsigned*>(work + l.records);
  const SortGeom& g = l.geom;
  if (n == 0) {     // (nothing to sort: start[] is all zero)
    VPS_HIP_CHECK(ctx, hipMemsetAsync(start, 0, sizeof(unsigned) * (l.nbricks + 1), ctx->stream));
    return VPS_OK;
  }
  if (l.two_level) {
    unsigned* table = reinterpret_cast<unsigned*>(work + l.table);
    unsigned* table_start = reinterpret_cast<unsigned*>(work + l.table_start);
    unsigned* table_tiles = reinterpret_cast<unsigned*>(work + l.table_tiles);
    unsigned* rec1 = reinterpret_cast<unsigned*>(work + l.rec1);
    const size_t lds1 = sort_hist_lds(g), lds2 = sort_fine_lds(g);
    const size_t lds_staged = sort_staged_lds(g, CR, SORT_ITEMS);
    const bool staged = sort_staged() && lds_staged <= ctx->lds_per_cu;
    auto level1 = [&](auto* keys) -> int {
      typedef typename std::remove_pointer<decltype(keys)>::type K;
      const auto key = key_of(K{});
      typedef typename std::remove_const<decltype(key)>::type Key;
      // (keys that are already stored are not written again)
      hipLaunchKernelGGL((sort_hist_kernel<SORT_ITEMS, K, Key>), dim3((unsigned)g.nchunks), dim3(SORT_THREADS), lds1, ctx->stream,
                         key, n, g, std::is_same<Key, StoredKeyOf<K>>::value ? (K*)nullptr : keys, table);
      launch_exclusive_scan(ctx->stream, table, (long long)g.ngroups * g.nchunks, table_tiles, table_start);
      if (staged) {
        auto kern = sort_scatter_staged_kernel<SORT_ITEMS, K, Pay>;
        if (int rcl = raise_lds_limit(ctx, kern, lds_staged)) return rcl;
        hipLaunchKernelGGL(kern, dim3((unsigned)(8 * ((g.nchunks + 7) / 8))), dim3(SORT_THREADS), lds_staged, ctx->stream,
                           (const K*)keys, pay, n, g, table_start, rec1);
      } else {
        hipLaunchKernelGGL((sort_scatter_kernel<SORT_ITEMS, K, Pay>), dim3((unsigned)g.nchunks), dim3(SORT_THREADS), lds1, ctx->stream,
                           (const K*)keys, pay, n, g, table_start, rec1);
      }
      return VPS_OK;
    };
    // (the keys[] region holds 8 bytes per particle either way: the atomic-rank path's keys are 64-bit)
    const int rc1 = l.wide_keys ? level1(reinterpret_cast<unsigned long long*>(work + l.keys))
                                : level1(reinterpret_cast<unsigned*>(work + l.keys));
    if (rc1) return rc1;
    hipLaunchKernelGGL((sort_fine_kernel<CR, true>), dim3((unsigned)g.ngroups), dim3(FINE_THREADS), lds2, ctx->stream, rec1, g,
                       table_start, start, records);
  } else {
    const auto key = key_of((unsigned long long)0);
    typedef typename std::remove_const<decltype(key)>::type Key;
    unsigned* tiles = reinterpret_cast<unsigned*>(work + l.tiles);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(work + l.keys);
    unsigned* ranks = reinterpret_cast<unsigned*>(work + l.ranks);
    VPS_HIP_CHECK(ctx, hipMemsetAsync(count, 0, sizeof(unsigned) * l.nbricks, ctx->stream));
    const unsigned pblocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(rank_kernel<Key>, dim3(pblocks), dim3(256), 0, ctx->stream, key, n, g.cells, count, keys, ranks);
    launch_exclusive_scan(ctx->stream, count, l.nbricks, tiles, start);
    hipLaunchKernelGGL(rank_scatter_kernel<Pay>, dim3(pblocks), dim3(256), 0, ctx->stream, keys, ranks, pay, n, g.cells, start,
                       records);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

// The pre-stage of a slab-sized workspace (l.recompute): {key, [rho v, rho]} of the slab's particles, compact, into keys[] / cpay;
// *n_sort: the slots handed out -- the slab's particles + at most one partly used block per workgroup.  One host synchronisation.
template <typename F, int C, bool RHOV>
int compact_slab(vps_ctx* ctx, const F* pos, const float* vel, const float* rho, int64_t np, F lcell, F nsz, const Bricks& b,
                 const DepLayout& l, char* work, long long* n_sort) {
  if (!(sort_staged() && sort_staged_lds(l.geom, C, SORT_ITEMS) <= ctx->lds_per_cu))
    return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "slab-sized sort workspace needs the LDS-staged scatter");
  if constexpr (C == 4 && RHOV) {
    unsigned long long* counter = reinterpret_cast<unsigned long long*>(work + l.counter);
    float4* cpay = reinterpret_cast<float4*>(work + l.cpay);
    VPS_HIP_CHECK(ctx, hipMemsetAsync(counter, 0, sizeof(unsigned long long), ctx->stream));
    const long long nch = (np + (long long)COMPACT_THREADS * COMPACT_ITEMS - 1) / ((long long)COMPACT_THREADS * COMPACT_ITEMS);
    const unsigned cgrid = (unsigned)std::min<long long>(std::min<long long>(nch, (long long)ctx->num_cu * 8), COMPACT_MAXGRID);
    auto launch = [&](auto* keys) {
      typedef typename std::remove_pointer<decltype(keys)>::type K;
      hipLaunchKernelGGL((slab_compact_kernel<F, K>), dim3(cgrid), dim3(COMPACT_THREADS), 0, ctx->stream, pos, vel, rho,
                         (long long)np, lcell, nsz, b, l.geom, keys, cpay, counter, l.cap_in);
    };
    if (l.wide_keys) launch(reinterpret_cast<unsigned long long*>(work + l.keys));
    else launch(reinterpret_cast<unsigned*>(work + l.keys));
    unsigned long long reserved = 0;
    VPS_HIP_CHECK(ctx, hipMemcpyAsync(&reserved, counter, sizeof(reserved), hipMemcpyDeviceToHost, ctx->stream));
    VPS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if ((long long)reserved > l.cap_in)
      return vps_fail(ctx, VPS_ERR_ARG, "more particles lie inside the slab than the workspace was sized for (%lld; vps_count_in_slab)",
                      l.cap);
    *n_sort = (long long)reserved;
    return VPS_OK;
  } else {
    return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "slab-sized sort workspace: [rho v, rho] records only");
  }
}

// particles -> records {cell-in-bucket, payload[C]} grouped by bucket + start[nbuckets + 1]
template <typename F, int C, bool RHOV>
int sort_into_buckets(vps_ctx* ctx, const F* pos, const float* payload, const float* rho, int64_t np, F lcell,
                      F nsz, const Bricks& b, const DepLayout& l, char* work) {
  vps_launch_timer tm(ctx, VPS_K_DEPOSIT);
  if constexpr (C == 4) {     // (dep_layout: no other record is compacted)
    if (np > 0 && l.recompute) {
      // filter first; the sort proper then sees the compacted arrays only: the stored keys, [rho v, rho] as stored
      long long n_sort = 0;
      if (int rc = compact_slab<F, C, RHOV>(ctx, pos, payload, rho, np, lcell, nsz, b, l, work, &n_sort)) return rc;
      return sort_records(ctx, [&](auto k) { return StoredKeyOf<decltype(k)>{reinterpret_cast<const decltype(k)*>(work + l.keys)}; },
                          DepPayload<4, false>{reinterpret_cast<const float*>(work + l.cpay), rho}, n_sort, l, work);
    }
  }
  return sort_records(ctx, [&](auto k) { return DepKeyOf<F, decltype(k)>{pos, lcell, nsz, b}; }, DepPayload<C, RHOV>{payload, rho},
                      (long long)np, l, work);
}

// The float each route's kernel receives for a quantity is decided here, one function per route, and nowhere else:
//   brick epilogue  alpha for the quantities that need it (alpha - 1 is formed on the device, in float: weighted_cell), else
//                   the cell volume (unused by VPS_LOG_DENSITY: 0)
//   grid kernel     the cell volume and alpha; the scalar density quantities get 1 / volume instead (CellPar)
//   pencil launch   pencil_quantity, below; NN emit: nn.hip, nn_emit_of
float brick_par(const vps_ctx* ctx, int quantity, float vol) {
  return vps_quantity_needs_alpha(quantity) ? (float)ctx->weight_alpha : quantity == VPS_LOG_DENSITY ? 0.f : vol;
}
CellPar grid_par(const vps_ctx* ctx, int quantity, double Lcell) {
  const double vol = Lcell * Lcell * Lcell;
  if (vps_quantity_scalar_rho(quantity)) return CellPar{(float)(1.0 / vol), quantity == VPS_DENSITY ? (float)ctx->weight_alpha : 1.f};
  return CellPar{(float)vol, quantity == VPS_WEIGHTED_VELOCITY ? (float)ctx->weight_alpha : 0.f};
}

template <typename F, int C, bool RHOV, int EPI>
int deposit_run(vps_ctx* ctx, const void* pos_v, const float* payload, const float* rho, int64_t np, int N,
                double Lbox, int x0, int nx, int quantity, int flags, float* grid, void* work_v) {
  const F* pos = reinterpret_cast<const F*>(pos_v);
  // Lcell = Lbox/float(N) in double, then cast to the dtype of pos: what numpy's weak
  // Python-float scalar does in `pos // Lcell`
  const F lcell = (F)(Lbox / (double)N);
  const F nsz = (F)N;
  const Bricks b = make_bricks(N, x0, nx, C);
  const DepLayout l = dep_layout(np, C, b);
  char* work = reinterpret_cast<char*>(work_v);
  unsigned* start = reinterpret_cast<unsigned*>(work + l.start);
  unsigned* records = reinterpret_cast<unsigned*>(work + l.records);
  const float vol = (float)((Lbox / (double)N) * (Lbox / (double)N) * (Lbox / (double)N));
  // (the fifth channel of the second-moment quantities: the records and the sort know nothing of it, the tile does)
  const size_t lds = tile_bytes(C, b.cells, EPI == EPI_ALGEBRA ? quantity : VPS_VELOCITY);
  if (int rcl = check_second_moment_tile(ctx, quantity, lds)) return rcl;      // before anything is enqueued
  const int rc = sort_into_buckets<F, C, RHOV>(ctx, pos, payload, rho, np, lcell, nsz, b, l, work);
  if (rc) return rc;
  {
    vps_launch_timer tm(ctx, VPS_K_ALGEBRA);
    auto launch_one = [&](auto q, float* dst) -> int {
      auto kern = brick_accumulate_kernel<C, EPI, decltype(q)::value>;
      if (int rcl = raise_lds_limit(ctx, kern, lds)) return rcl;
      hipLaunchKernelGGL(kern, dim3(brick_launch_grid(ctx, lds, l.nbricks)), dim3(256), lds, ctx->stream,
                         records, start, b, l.nbricks, flags, brick_par(ctx, decltype(q)::value & ~TENSOR_OFFDIAG, vol), dst);
      return VPS_OK;
    };
    // (a tensor quantity: the diagonal half into channels 0..2, then the off-diagonal half into 3..5, from the same records)
    auto launch = [&](auto q) -> int {
      constexpr int Q = decltype(q)::value;
      if (int rcl = launch_one(q, grid)) return rcl;
      if constexpr (EPI == EPI_ALGEBRA && vps_quantity_tensor(Q))
        return launch_one(std::integral_constant<int, Q | TENSOR_OFFDIAG>{}, grid + 3 * (size_t)nx * N * N);
      return VPS_OK;
    };
    if constexpr (EPI == EPI_RAW) {
      if (int rcl = launch(std::integral_constant<int, VPS_VELOCITY>{})) return rcl;   // (no quantity: the one raw instantiation)
    } else if (int rcq = dispatch_quantity<true>(quantity, launch)) {
      return rcq == VPS_ERR_HIP ? rcq : vps_fail(ctx, rcq, "deposit: quantity %d", quantity);
    }
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

// rank -> scan -> scatter of [rho v, rho] records into the buckets `b`; returns the layout used
template <typename F>
int sort_rhov_records(vps_ctx* ctx, const F* pos, const float* vel, const float* rho, int64_t np, int N,
                      double Lbox, const Bricks& b, char* work, DepLayout* lay, int64_t np_cap = -1) {
  const F lcell = (F)(Lbox / (double)N);
  const F nsz = (F)N;
  *lay = dep_layout(np, 4, b, np_cap);
  return sort_into_buckets<F, 4, true>(ctx, pos, vel, rho, np, lcell, nsz, b, *lay, work);
}

// particles whose bit-exact cell lies inside the slab (the rule of `locate`)
template <typename F>
__global__ void __launch_bounds__(256) count_in_slab_kernel(const F* __restrict__ pos, long long np, F lcell, F nsize, Bricks b,
                                                            unsigned long long* __restrict__ out) {
  unsigned n = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (long long)gridDim.x * blockDim.x) {
    unsigned brick, loc;
    n += locate<F>(pos, i, lcell, nsize, b, brick, loc) ? 1u : 0u;
  }
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(out, (unsigned long long)n);
}

int check_deposit_args(vps_ctx* ctx, const char* who, int64_t np, int N, double Lbox, int x0, int nx) {
  if (np < 0 || N < 1 || !(Lbox > 0)) return vps_fail(ctx, VPS_ERR_ARG, "%s: bad np/N/Lbox", who);
  if (x0 < 0 || nx < 1 || x0 + nx > N) return vps_fail(ctx, VPS_ERR_ARG, "%s: slab [%d,%d) outside [0,%d)", who, x0, x0 + nx, N);
  if ((np + 255) / 256 > 0x7fffffffLL) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "%s: np too large for one launch", who);
  if (np > 0xffffffffLL) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "%s: np exceeds 32-bit bucket offsets", who);
  return VPS_OK;
}

// ---- direct CIC / TSC deposit: one record per PARTICLE, owner-computes accumulation --------------------------------------
// The expansion above moves 8 / 27 records per particle through the sort.  Here a particle is sorted ONCE, into the brick of its
// base cell c0 (the lowest cell it touches on each axis), with a record {cell-in-brick, payload[C], 6 weight words}; the brick
// that OWNS a grid cell then gathers: it walks its own bucket and the buckets of the bricks that hold the order - 1 cells below
// its range on every axis (usually the -1 neighbour: at most 8 buckets), and adds payload * wx * wy * wz into its LDS tile for
// every (record, offset) whose target cell (c0 + j) mod N lies in its own range.  Every (particle, offset) pair has exactly one
// owner, so it is counted exactly once; every grid cell is written exactly once, by plain streaming stores, as in the NGP route:
// no grid memset, no global float atomic.  vps_deposit_assign writes the whole grid (x0 = 0, nx = N) of raw channels; an x-slab
// of quantity fields comes from the fused form further down (assign_field_kernel), which keeps this key geometry and drops the
// particles without a target row in the slab -- with replicated particles no halo is exchanged.
//
// c0 is the float64 rule of assign_expand_kernel -- s = (double)pos / lcell, floor(s - 1/2) for CIC, floor(s) - 1 for TSC,
// wrapped into [0, N) BEFORE the conversion to int (wrap_cell's expression) -- never cell_of<F>, the NGP rule in the particle's
// dtype, which can differ by a cell at a face: the particle would then sit in a bucket its targets' owners do not read.
// A position whose s is not finite (NaN, inf), or so large (beyond 2^53 cells) that the wrapped cell number does not come out in
// [0, N), gets sort_invalid and is SKIPPED: it deposits nowhere.  (The expansion route makes no promise for such positions.)
template <int ORDER>
__device__ __forceinline__ double assign_base_cell(double s) {
  return ORDER == 2 ? floor(s - 0.5) : floor(s) - 1.0;
}

// The slab window of the fused form (vps_deposit_field with VPS_FLAG_ASSIGN): one more way of being invalid, a particle none of
// whose ORDER target rows (c0x + j) mod N lies in [x0, x0 + nx).  Those rows are in the slab exactly when c0x lies in the window
// [x0 - (ORDER - 1), x0 + nx - 1] mod N, i.e. (c0x - xlo) mod N < span with xlo = x0 - (ORDER - 1), span = nx + ORDER - 1; with
// span >= N every particle passes.  The whole grid has no window: nothing of the test exists in its key.
struct WholeGrid {
  __device__ __forceinline__ bool keeps(int, int) const { return true; }
};
struct SlabWindow {
  int xlo, span;
  __device__ __forceinline__ bool keeps(int c0x, int N) const {
    int d = c0x - xlo;                               // in (-N, N + ORDER - 1)
    if (d < 0) d += N;
    if (d >= N) d -= N;
    return d < span;
  }
};

template <typename F, typename K, int ORDER, typename Window>
struct AssignKeyOf {
  const F* __restrict__ pos;
  double lcell, n;
  Bricks b;       // make_bricks(N, 0, N, C): the whole grid's, whatever the window
  Window window;
  __device__ __forceinline__ K operator()(long long i) const {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double f0 = assign_base_cell<ORDER>((double)pos[i * 3 + a] / lcell);
      const double r = f0 - floor(f0 / n) * n;          // wrap_cell, before its conversion
      if (!(r >= 0.0 && r < n)) return sort_invalid<K>();   // NaN, inf, beyond 2^53
      c[a] = (int)r;
      if (a == 0 && !window.keeps(c[0], b.N)) return sort_invalid<K>();         // no target row in the slab
    }
    const int ix = c[0] / b.bx, iy = c[1] / b.by, iz = c[2] / b.bz;
    const unsigned brick = (unsigned)((ix * b.nby + iy) * b.nbz + iz);
    const unsigned loc = (unsigned)(((c[0] - ix * b.bx) * b.by + (c[1] - iy * b.by)) * b.bz + (c[2] - iz * b.bz));
    return (K)brick * (unsigned)b.cells + loc;
  }
};

// Per axis TWO float32 numbers each rounded once from float64, so that a small weight keeps its relative precision (a weight of
// 1e-9 next to a cell centre would lose all of it if 1 - f were formed in float32 from a rounded f):
//   CIC: (float)(1 - f), (float)f                         -- the two weights themselves
//   TSC: a = (float)(1/2 - d), b = (float)(1/2 + d)       -- weights a a / 2, 1/2 + a b (= 3/4 - d^2), b b / 2 (assign_axis_weights)
template <int ORDER, typename F>
__device__ __forceinline__ void assign_weight_words(const F* __restrict__ pos, long long i, double lcell, float out6[6]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double s = (double)pos[i * 3 + a] / lcell;
    if constexpr (ORDER == 2) {
      const double f = s - 0.5 - floor(s - 0.5);
      out6[2 * a] = (float)(1.0 - f);
      out6[2 * a + 1] = (float)f;
    } else {
      const double d = s - (floor(s) + 0.5);
      out6[2 * a] = (float)(0.5 - d);
      out6[2 * a + 1] = (float)(0.5 + d);
    }
  }
}

// payload[CP] (RHOV: [rho v, rho] built on the fly from `payload` = vel and rho, load_payload) and the six weight words
template <typename F, int CP, bool RHOV, int ORDER>
struct AssignPayload {
  static constexpr int C = CP + 6;
  const F* __restrict__ pos;
  const float* __restrict__ payload;
  const float* __restrict__ rho;
  double lcell;
  __device__ __forceinline__ void load(long long i, float val[CP + 6]) const {
    load_payload<CP, RHOV>(payload, rho, i, val);
    assign_weight_words<ORDER>(pos, i, lcell, val + CP);
  }
};

template <int ORDER>
__device__ __forceinline__ void assign_axis_weights(float a, float b, float w[ORDER]) {
  if constexpr (ORDER == 2) {
    w[0] = a;
    w[1] = b;
  } else {
    w[0] = 0.5f * (a * a);
    w[1] = 0.5f + a * b;
    w[2] = 0.5f * (b * b);
  }
}

// The bricks along one axis whose buckets brick i gathers from: itself, then the bricks holding the cells lo - 1 .. lo - (order - 1)
// (periodic), distinct.  With one brick on the axis that is the brick itself, with two the -1 and the +1 neighbour are the same
// brick, and where the last, partial brick is narrower than order - 1 cells (one cell at N = 65, TSC) brick 0 also reads the one
// before it: the set is formed from the cells, so no grid needs refusing.  Returns the count (<= 3).
__host__ __device__ inline int assign_axis_sources(int i, int bw, int N, int order, int src[3]) {
  int n = 0;
  src[n++] = i;
  const int lo = i * bw;
  for (int k = 1; k < order; ++k) {
    const int cell = ((lo - k) % N + N) % N;
    const int s = cell / bw;
    bool seen = false;
    for (int m = 0; m < n; ++m) seen = seen || src[m] == s;
    if (!seen) src[n++] = s;
  }
  return n;
}

// The owner-computes gather of brick (ix, iy, iz): records {cell-in-brick of c0, payload[C], 6 weight words} of its source buckets
// -> LDS float adds into tile [CT][cells].  The brick owns the cells of its range (the last brick of an axis may be partial) on
// the x rows [cx0, cx1): the whole range, or its part inside a slab -- the other rows of the tile are never added to.  CT = C + 1:
// the second-moment channel, rho_p |v_p|^2 of [rho v, rho] records, behind the C record channels (TileOut); CT = C + 3 with
// MOMENT = 2 / 3: the diagonal / off-diagonal half of rho_p v_i v_j (TileOut::MOMENT).
// (`b` by reference: by value the kernels lose 1 - 2 % of their instructions and take up to 4 more VGPRs; DESIGN.md has both)
template <int C, int CT, int ORDER, int MOMENT = (CT > C ? 1 : 0)>
__device__ __forceinline__ void assign_gather(const unsigned* __restrict__ records, const unsigned* __restrict__ start,
                                              const Bricks& b, int ix, int iy, int iz, int cx0, int cx1, float* tile) {
  constexpr int W = C + 7;
  const int cells = b.cells, N = b.N;
  const int gx0 = ix * b.bx, gy0 = iy * b.by, gz0 = iz * b.bz;
  const int gy1 = min(gy0 + b.by, N), gz1 = min(gz0 + b.bz, N);
  int srcx[3], srcy[3], srcz[3];
  const int nsx = assign_axis_sources(ix, b.bx, N, ORDER, srcx);
  const int nsy = assign_axis_sources(iy, b.by, N, ORDER, srcy);
  const int nsz = assign_axis_sources(iz, b.bz, N, ORDER, srcz);
  for (int sx = 0; sx < nsx; ++sx)
    for (int sy = 0; sy < nsy; ++sy)
      for (int sz = 0; sz < nsz; ++sz) {
        const long long sb = ((long long)srcx[sx] * b.nby + srcy[sy]) * b.nbz + srcz[sz];
        const unsigned s = start[sb], e = start[sb + 1];
        const int ox = srcx[sx] * b.bx, oy = srcy[sy] * b.by, oz = srcz[sz] * b.bz;     // first cell of the source brick
        for (unsigned j = s + threadIdx.x; j < e; j += blockDim.x) {
          const unsigned* rec = records + (size_t)j * W;
          int lz, ly, lx;
          brick_cell(b, (int)rec[0], lx, ly, lz);
          // target cells per axis, relative to this brick; a record none of whose targets on some axis is ours is dropped
          // before its payload and weights are read (most records of a neighbour's bucket)
          int tx[ORDER], ty[ORDER], tz[ORDER];
          bool anyx = false, anyy = false, anyz = false;
#pragma unroll
          for (int k = 0; k < ORDER; ++k) {
            int t = ox + lx + k;
            if (t >= N) t %= N;
            tx[k] = (t >= cx0 && t < cx1) ? t - gx0 : -1;
            anyx = anyx || tx[k] >= 0;
            t = oy + ly + k;
            if (t >= N) t %= N;
            ty[k] = (t >= gy0 && t < gy1) ? t - gy0 : -1;
            anyy = anyy || ty[k] >= 0;
            t = oz + lz + k;
            if (t >= N) t %= N;
            tz[k] = (t >= gz0 && t < gz1) ? t - gz0 : -1;
            anyz = anyz || tz[k] >= 0;
          }
          if (!(anyx && anyy && anyz)) continue;
          float pay[CT], wx[ORDER], wy[ORDER], wz[ORDER];
#pragma unroll
          for (int c = 0; c < C; ++c) pay[c] = __uint_as_float(rec[1 + c]);
          // (the particle's rho_p |v_p|^2, once per record: it takes the same weight product as the four channels)
          if constexpr (MOMENT >= 2) tensor_terms<MOMENT == 3>(pay[0], pay[1], pay[2], pay[3], pay + C);
          else if constexpr (CT > C) pay[C] = second_moment_term(pay[0], pay[1], pay[2], pay[3]);
          assign_axis_weights<ORDER>(__uint_as_float(rec[1 + C]), __uint_as_float(rec[2 + C]), wx);
          assign_axis_weights<ORDER>(__uint_as_float(rec[3 + C]), __uint_as_float(rec[4 + C]), wy);
          assign_axis_weights<ORDER>(__uint_as_float(rec[5 + C]), __uint_as_float(rec[6 + C]), wz);
#pragma unroll
          for (int kx = 0; kx < ORDER; ++kx) {
            if (tx[kx] < 0) continue;
#pragma unroll
            for (int ky = 0; ky < ORDER; ++ky) {
              if (ty[ky] < 0) continue;
#pragma unroll
              for (int kz = 0; kz < ORDER; ++kz) {
                if (tz[kz] < 0) continue;
                const float wt = wx[kx] * wy[ky] * wz[kz];      // (the product order of assign_expand_kernel)
                const int at = (tx[kx] * b.by + ty[ky]) * b.bz + tz[kz];
#pragma unroll
                for (int c = 0; c < CT; ++c) atomicAdd(&tile[c * cells + at], pay[c] * wt);
              }
            }
          }
        }
      }
}

// records grouped by the brick of c0 -> grid [C][N][N][N] of raw channels, every cell written
template <int C, int ORDER>
__global__ void __launch_bounds__(256)
    assign_accumulate_kernel(const unsigned* __restrict__ records, const unsigned* __restrict__ start, Bricks b,
                             long long nbricks, float* __restrict__ grid) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tile = reinterpret_cast<float*>(smem_raw);  // [C][cells]
  const int cells = b.cells, N = b.N;
  const bool vec4 = ((b.bz & 3) == 0) && ((N & 3) == 0);
  for (int i = threadIdx.x; i < C * cells; i += blockDim.x) tile[i] = 0.f;
  const long long plane = (long long)N * N * N;
  __syncthreads();
  for (long long brick = blockIdx.x; brick < nbricks; brick += gridDim.x) {
    int ix, iy, iz;
    brick_index(b, brick, ix, iy, iz);
    const int gx0 = ix * b.bx, gy0 = iy * b.by, gz0 = iz * b.bz;
    assign_gather<C, C, ORDER>(records, start, b, ix, iy, iz, gx0, min(gx0 + b.bx, N), tile);
    __syncthreads();
    // stream the tile out (rows of bz cells are contiguous in the grid) and zero it for the next brick
    if (vec4) {
      for (int i = threadIdx.x; i < cells / 4; i += blockDim.x) {
        const int loc = i * 4;
        int lz, ly, lx;
        brick_cell(b, loc, lx, ly, lz);
        const int gx = gx0 + lx, gy = gy0 + ly, gz = gz0 + lz;
        const bool inside = gx < N && gy < N && gz < N;      // (N and bz multiples of 4: a quad is inside or outside as a whole)
        const long long cell = ((long long)gx * N + gy) * N + gz;
        tile_out4<C, EPI_RAW, VPS_VELOCITY, true>(tile, cells, loc, inside, 0, CellPar{}, grid, plane, cell);
      }
    } else {
      for (int loc = threadIdx.x; loc < cells; loc += blockDim.x) {
        int lz, ly, lx;
        brick_cell<false>(b, loc, lx, ly, lz);
        const int gx = gx0 + lx, gy = gy0 + ly, gz = gz0 + lz;
        const bool inside = gx < N && gy < N && gz < N;
        const long long cell = ((long long)gx * N + gy) * N + gz;
        tile_out1<C, EPI_RAW, VPS_VELOCITY, true>(tile, cells, loc, inside, 0, CellPar{}, grid, plane, cell);
      }
    }
    __syncthreads();   // tile is all zero again
  }
}

// The fused form of the direct route on an x-slab: records {cell-in-brick of c0, [rho v, rho], 6 weight words} grouped by the
// brick of c0 in the WHOLE grid's geometry `b` (x0 = 0, nx = N) -> the fields of QUANT on the rows [x0, x0 + nx), out
// [NOUT][nx][N][N], every cell written exactly once; `par`: brick_par.  Three things differ from the whole grid: only the bricks
// [first, first + nbricks) whose x range meets the slab are walked; a brick owns its cells on the rows [cx0, cx1) = its x range
// clipped to the slab only (the other rows of its tile are never added to and never read); and the stream-out addresses row
// gx - x0 with plane stride nx N N.
template <int ORDER, int QUANT>
__global__ void __launch_bounds__(256)
    assign_field_kernel(const unsigned* __restrict__ records, const unsigned* __restrict__ start, Bricks b, long long first,
                        long long nbricks, int x0, int nx, int flags, float par, float* __restrict__ out) {
  constexpr int C = 4, CT = TileOut<C, EPI_ALGEBRA, QUANT>::CT;
  const int cflags = tile_cflags<QUANT>(flags);
  const CellPar cpar{par, par};     // (one float, copied into both members: brick_accumulate_kernel)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* tile = reinterpret_cast<float*>(smem_raw);  // [CT][cells]
  const int cells = b.cells, N = b.N;
  const bool vec4 = ((b.bz & 3) == 0) && ((N & 3) == 0);
  for (int i = threadIdx.x; i < CT * cells; i += blockDim.x) tile[i] = 0.f;
  const long long plane = (long long)nx * N * N;
  const int rowcells = b.by * b.bz;       // cells of one x row of the tile
  __syncthreads();
  for (long long t = blockIdx.x; t < nbricks; t += gridDim.x) {
    int ix, iy, iz;
    brick_index(b, first + t, ix, iy, iz);
    const int gx0 = ix * b.bx, gy0 = iy * b.by, gz0 = iz * b.bz;
    const int cx0 = max(gx0, x0), cx1 = min(min(gx0 + b.bx, N), x0 + nx);
    assign_gather<C, CT, ORDER, TileOut<C, EPI_ALGEBRA, QUANT>::MOMENT>(records, start, b, ix, iy, iz, cx0, cx1, tile);
    __syncthreads();
    // stream the owned rows out (rows of bz cells are contiguous in the slab) and zero them for the next brick
    const int loc_lo = (cx0 - gx0) * rowcells, loc_hi = (cx1 - gx0) * rowcells;
    if (vec4) {
      for (int loc = loc_lo + 4 * (int)threadIdx.x; loc < loc_hi; loc += 4 * (int)blockDim.x) {
        int lz, ly, lx;
        brick_cell(b, loc, lx, ly, lz);
        const int gx = gx0 + lx, gy = gy0 + ly, gz = gz0 + lz;
        const bool inside = gy < N && gz < N;      // (gx is inside by the loop's bounds; N and bz multiples of 4: whole quads)
        const long long cell = ((long long)(gx - x0) * N + gy) * N + gz;
        tile_out4<C, EPI_ALGEBRA, QUANT, true>(tile, cells, loc, inside, cflags, cpar, out, plane, cell);
      }
    } else {
      for (int loc = loc_lo + (int)threadIdx.x; loc < loc_hi; loc += (int)blockDim.x) {
        int lz, ly, lx;
        brick_cell<false>(b, loc, lx, ly, lz);
        const int gx = gx0 + lx, gy = gy0 + ly, gz = gz0 + lz;
        const bool inside = gy < N && gz < N;
        const long long cell = ((long long)(gx - x0) * N + gy) * N + gz;
        tile_out1<C, EPI_ALGEBRA, QUANT, true>(tile, cells, loc, inside, cflags, cpar, out, plane, cell);
      }
    }
    __syncthreads();   // the owned rows are all zero again (the others were never touched)
  }
}

// brick geometry and sort layout of the direct route: the bricks of the NGP deposit of C channels (the LDS tile holds the C
// payload channels only), records of C + 6 channels
struct AssignPlan {
  Bricks b;
  DepLayout l;
};
AssignPlan assign_plan(int64_t np, int C, int N) {
  AssignPlan p;
  p.b = make_bricks(N, 0, N, C);
  p.l = dep_layout(np, C + 6, p.b);
  return p;
}

int check_assign_args(vps_ctx* ctx, const char* who, int64_t np, int C, int N, int order) {
  if (np < 0 || N < 1) return vps_fail(ctx, VPS_ERR_ARG, "%s: bad np/N", who);
  if (order != 2 && order != 3) return vps_fail(ctx, VPS_ERR_ARG, "%s: order must be 2 (CIC) or 3 (TSC)", who);
  if (C != 1 && C != 3 && C != 4) return vps_fail(ctx, VPS_ERR_ARG, "%s: C=%d channels (supported: 1,3,4)", who, C);
  if ((np + 255) / 256 > 0x7fffffffLL) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "%s: np too large for one launch", who);
  if (np > 0xffffffffLL) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "%s: np exceeds 32-bit bucket offsets", who);
  return VPS_OK;
}

template <typename F, int C, int ORDER>
int deposit_assign_run(vps_ctx* ctx, const void* pos_v, const float* payload, int64_t np, int N, double Lbox, float* grid,
                       void* work_v) {
  const AssignPlan p = assign_plan(np, C, N);
  char* work = reinterpret_cast<char*>(work_v);
  const double lcell = Lbox / (double)N;      // float64 whatever the dtype of pos (assign_expand_kernel's)
  const F* pos = reinterpret_cast<const F*>(pos_v);
  {
    vps_launch_timer tm(ctx, VPS_K_DEPOSIT);
    const int rc = sort_records(ctx, [&](auto k) { return AssignKeyOf<F, decltype(k), ORDER, WholeGrid>{pos, lcell, (double)N, p.b, {}}; },
                                AssignPayload<F, C, false, ORDER>{pos, payload, nullptr, lcell}, (long long)np, p.l, work);
    if (rc) return rc;
  }
  {
    vps_launch_timer tm(ctx, VPS_K_ALGEBRA);
    const size_t lds = (size_t)C * p.b.cells * sizeof(float);
    hipLaunchKernelGGL((assign_accumulate_kernel<C, ORDER>), dim3(brick_launch_grid(ctx, lds, p.l.nbricks)), dim3(256), lds, ctx->stream,
                       reinterpret_cast<const unsigned*>(work + p.l.records), reinterpret_cast<const unsigned*>(work + p.l.start),
                       p.b, p.l.nbricks, grid);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

template <typename F, int C>
int deposit_assign_order(vps_ctx* ctx, const void* pos, const float* payload, int64_t np, int N, double Lbox, int order,
                         float* grid, void* work) {
  return order == 2 ? deposit_assign_run<F, C, 2>(ctx, pos, payload, np, N, Lbox, grid, work)
                    : deposit_assign_run<F, C, 3>(ctx, pos, payload, np, N, Lbox, grid, work);
}

// vps_deposit_field with VPS_FLAG_ASSIGN(ORDER): the direct route's sort keyed by the whole grid's bricks with the slab's
// window in the key, then assign_field_kernel over the bricks whose x range meets [x0, x0 + nx)
template <typename F, int ORDER>
int deposit_assign_field_run(vps_ctx* ctx, const void* pos_v, const float* vel, const float* rho, int64_t np, int N, double Lbox,
                             int x0, int nx, int quantity, int flags, float* fields, void* work_v) {
  const AssignPlan p = assign_plan(np, 4, N);
  const Bricks& b = p.b;
  char* work = reinterpret_cast<char*>(work_v);
  const double lcell = Lbox / (double)N;      // float64 whatever the dtype of pos, as in the direct route
  const F* pos = reinterpret_cast<const F*>(pos_v);
  const int xlo = x0 - (ORDER - 1);
  const int span = nx + ORDER - 1 >= N ? 0x7fffffff : nx + ORDER - 1;     // (the whole ring: every particle passes)
  const size_t lds = tile_bytes(4, b.cells, quantity);       // (five channels for the second-moment scalars, seven for a tensor half)
  if (int rcl = check_second_moment_tile(ctx, quantity, lds)) return rcl;      // before anything is enqueued
  {
    vps_launch_timer tm(ctx, VPS_K_DEPOSIT);
    const int rc = sort_records(ctx, [&](auto k) { return AssignKeyOf<F, decltype(k), ORDER, SlabWindow>{pos, lcell, (double)N, b, {xlo, span}}; },
                                AssignPayload<F, 4, true, ORDER>{pos, vel, rho, lcell}, (long long)np, p.l, work);
    if (rc) return rc;
  }
  const float vol = (float)(lcell * lcell * lcell);
  {
    vps_launch_timer tm(ctx, VPS_K_ALGEBRA);
    const int ix_lo = x0 / b.bx, ix_hi = (x0 + nx - 1) / b.bx;
    const long long per_x = (long long)b.nby * b.nbz;
    const long long first = ix_lo * per_x, nbricks = (ix_hi - ix_lo + 1) * per_x;
    auto launch_one = [&](auto q, float* dst) -> int {
      auto kern = assign_field_kernel<ORDER, decltype(q)::value>;
      if (int rcl = raise_lds_limit(ctx, kern, lds)) return rcl;
      hipLaunchKernelGGL(kern, dim3(brick_launch_grid(ctx, lds, nbricks)), dim3(256), lds, ctx->stream,
                         reinterpret_cast<const unsigned*>(work + p.l.records), reinterpret_cast<const unsigned*>(work + p.l.start),
                         b, first, nbricks, x0, nx, flags, brick_par(ctx, decltype(q)::value & ~TENSOR_OFFDIAG, vol), dst);
      return VPS_OK;
    };
    // (a tensor quantity: two gathers over the one sort's records, deposit_run)
    const int rcq = dispatch_quantity<true>(quantity, [&](auto q) -> int {
      constexpr int Q = decltype(q)::value;
      if (int rcl = launch_one(q, fields)) return rcl;
      if constexpr (vps_quantity_tensor(Q))
        return launch_one(std::integral_constant<int, Q | TENSOR_OFFDIAG>{}, fields + 3 * (size_t)nx * N * N);
      return VPS_OK;
    });
    if (rcq) return rcq == VPS_ERR_HIP ? rcq : vps_fail(ctx, rcq, "vps_deposit_field: quantity %d", quantity);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

// no entry point but vps_deposit_field takes the assignment bits: they would be silently ignored and the caller get NGP
int refuse_assign_flags(vps_ctx* ctx, const char* who, int flags) {
  if (flags & VPS_FLAG_ASSIGN_MASK)
    return vps_fail(ctx, VPS_ERR_ARG, "%s: VPS_FLAG_ASSIGN is taken by vps_deposit_field only (flags 0x%x)", who, flags);
  return VPS_OK;
}

}  // namespace

extern "C" {

int vps_cell_index(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, int64_t np, int N, double Lbox,
                   int32_t* cell_dev) {
  VPS_ENTER(ctx);
  if (np < 0 || N < 1 || !(Lbox > 0)) return vps_fail(ctx, VPS_ERR_ARG, "vps_cell_index: bad np/N/Lbox");
  if (np == 0) return VPS_OK;
  if (!pos_dev || !cell_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_cell_index: null buffer");
  const unsigned blocks = (unsigned)((np + 255) / 256);
  {
    vps_launch_timer tm(ctx, VPS_K_MISC);
    if (pos_is_f64)
      hipLaunchKernelGGL(cell_index_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream,
                         reinterpret_cast<const double*>(pos_dev), (long long)np,
                         Lbox / (double)N, (double)N, cell_dev);
    else
      hipLaunchKernelGGL(cell_index_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream,
                         reinterpret_cast<const float*>(pos_dev), (long long)np,
                         (float)(Lbox / (double)N), (float)N, cell_dev);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

size_t vps_deposit_workspace_bytes(int64_t np, int C, int N, int nx) {
  if (np < 0 || C < 1 || N < 1 || nx < 1) return 0;
  const Bricks b = make_bricks(N, 0, nx, C);
  return dep_layout(np, C, b).total;
}

int vps_deposit_ngp(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* payload_dev,
                    int64_t np, int C, int N, double Lbox, int x0, int nx, float* grid_dev,
                    void* work_dev) {
  VPS_ENTER(ctx);
  int rc = check_deposit_args(ctx, "vps_deposit_ngp", np, N, Lbox, x0, nx);
  if (rc) return rc;
  if (!grid_dev || !work_dev || (np > 0 && (!pos_dev || !payload_dev)))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_ngp: null buffer");
#define VPS_DEP(CC)                                                                                        \
  (pos_is_f64 ? deposit_run<double, CC, false, EPI_RAW>(ctx, pos_dev, payload_dev, nullptr, np, N, Lbox, x0, \
                                                        nx, 0, 0, grid_dev, work_dev)                       \
              : deposit_run<float, CC, false, EPI_RAW>(ctx, pos_dev, payload_dev, nullptr, np, N, Lbox, x0,  \
                                                       nx, 0, 0, grid_dev, work_dev))
  switch (C) {
    case 1: return VPS_DEP(1);
    case 3: return VPS_DEP(3);
    case 4: return VPS_DEP(4);
    default: return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_deposit_ngp: C=%d channels (supported: 1,3,4)", C);
  }
#undef VPS_DEP
}

int vps_deposit_field(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                      const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx, int quantity,
                      int flags, float* fields_dev, void* work_dev) {
  VPS_ENTER(ctx);
  int rc = check_deposit_args(ctx, "vps_deposit_field", np, N, Lbox, x0, nx);
  if (rc) return rc;
  if (!vps_quantity_valid(quantity)) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_field: quantity %d", quantity);
  if ((rc = vps_refuse_grid_only(ctx, "vps_deposit_field", quantity, "a brick's epilogue does not see the neighbouring cells"))) return rc;
  if ((rc = vps_check_weighted(ctx, "vps_deposit_field", quantity, flags))) return rc;
  if (vps_quantity_second_moment(quantity) && (flags & (VPS_FLAG_REFERENCE_MOMENTUM_BUG | VPS_FLAG_INPUT_IS_VM)))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_field: quantity %d (%s) takes neither VPS_FLAG_REFERENCE_MOMENTUM_BUG nor VPS_FLAG_INPUT_IS_VM",
                    quantity, vps_second_moment_name(quantity));
  if (vps_quantity_tensor(quantity) && (flags & VPS_FLAG_COMPONENT_MASK))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_field: quantity %d (%s) does not take VPS_FLAG_COMPONENTS: its six fields come from two launches",
                    quantity, vps_second_moment_name(quantity));
  if (flags & VPS_FLAG_INPUT_IS_VM) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_field: VPS_FLAG_INPUT_IS_VM is meaningless here");
  if (!fields_dev || !work_dev || (np > 0 && (!pos_dev || !vel_dev || !rho_dev)))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_field: null buffer");
  if (flags & VPS_FLAG_ASSIGN_MASK) {
    const int order = ((flags & VPS_FLAG_ASSIGN_MASK) >> 8) + 1;
    if (order != 2 && order != 3)
      return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_field: VPS_FLAG_ASSIGN(order): order must be 2 (CIC) or 3 (TSC), flags 0x%x", flags);
    const int eflags = flags & ~VPS_FLAG_ASSIGN_MASK;
#define VPS_DAF(FF, OO) deposit_assign_field_run<FF, OO>(ctx, pos_dev, vel_dev, rho_dev, np, N, Lbox, x0, nx, quantity, eflags, fields_dev, work_dev)
    if (pos_is_f64) return order == 2 ? VPS_DAF(double, 2) : VPS_DAF(double, 3);
    return order == 2 ? VPS_DAF(float, 2) : VPS_DAF(float, 3);
#undef VPS_DAF
  }
  return pos_is_f64 ? deposit_run<double, 4, true, EPI_ALGEBRA>(ctx, pos_dev, vel_dev, rho_dev, np, N, Lbox, x0,
                                                               nx, quantity, flags, fields_dev, work_dev)
                    : deposit_run<float, 4, true, EPI_ALGEBRA>(ctx, pos_dev, vel_dev, rho_dev, np, N, Lbox, x0,
                                                              nx, quantity, flags, fields_dev, work_dev);
}

int vps_deposit_fft_zy_supported(vps_ctx* ctx, int N, int quantity) {
  if (!ctx) return 0;
  // (VPS_VM is four fields of two kinds: not a pencil launch; the second-moment quantities need a fifth tile channel, which the
  //  pencil kernel does not have; the gradient quantities need a cell's neighbours in x and y, which a pencil does not hold)
  return vps_quantity_valid(quantity) && quantity != VPS_VM && !vps_quantity_second_moment(quantity) &&
         !vps_quantity_gradient(quantity) && !vps_quantity_filter(quantity) && vps_pencil_supported(ctx, N) ? 1 : 0;
}

size_t vps_deposit_fft_zy_workspace_bytes(int64_t np, int N, int nx) {
  if (np < 0 || N < 16 || nx < 1) return 0;
  const Bricks b = make_pencils(N, 0, nx, vps_pencil_tp(N));
  const size_t sort = dep_layout(np, 4, b).total;
  const size_t images = 3 * ((size_t)nx * (N / 2) * N + (size_t)nx * N) * sizeof(float2);
  return sort + images;
}

size_t vps_deposit_fft_zy_workspace_bytes_shared(int64_t np, int N, int nx) {
  const size_t base = vps_deposit_fft_zy_workspace_bytes(np, N, nx);
  return base ? base + ((size_t)nx * (N / 2) * N + (size_t)nx * N) * sizeof(float2) : 0;
}

static int deposit_fft_impl(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                            const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx, int quantity,
                            int flags, void* spec_dev, void* nyq_dev, void* zimg_dev, void* work_dev, int64_t np_cap = -1);

// What the pencil launch of (quantity, flags) forms: the components and their record channels, the launch form, and the
// exponent it reads -- (float)(alpha - 1.0) from the host's double for the weighted velocity, alpha for the density (alpha = 1,
// the plain density: no per-cell function at all).
static int pencil_quantity(vps_ctx* ctx, int quantity, int flags, PencilQuantity* pq) {
  PencilQuantity q;
  const int bug = (quantity == VPS_MOMENTUM) && (flags & VPS_FLAG_REFERENCE_MOMENTUM_BUG);
  if (bug) q.chan[1] = q.chan[2] = 0;
  q.ncomp = vps_quantity_scalar_rho(quantity) ? 1 : 3;   // (the energy launch makes its one field from three components)
  q.divide = (quantity == VPS_MOMENTUM || vps_quantity_scalar_rho(quantity)) ? 0 : 1;
  q.energy = quantity == VPS_ENERGY;
  q.weighted = quantity == VPS_WEIGHTED_VELOCITY;
  if (q.weighted) q.wexp = (float)(ctx->weight_alpha - 1.0);
  if (quantity == VPS_LOG_DENSITY) q.scalar = PENCIL_SCALAR_LOG;
  if (quantity == VPS_DENSITY) {
    q.sexp = (float)ctx->weight_alpha;
    q.scalar = q.sexp == 1.f ? PENCIL_SCALAR_RHO : PENCIL_SCALAR_POW;
  }
  const int only = (flags & VPS_FLAG_COMPONENT_MASK) >> 4;   // bit c: component c is wanted (VPS_FLAG_COMPONENTS); 0: all
  if (flags & VPS_FLAG_SHARE_ENERGY) {
    if (quantity == VPS_MOMENTUM && !bug && !only) q.with_energy = 1;
    else if (quantity == VPS_ENERGY && (flags & VPS_FLAG_REUSE_SORT)) q.with_energy = 2;
    else return vps_fail(ctx, VPS_ERR_ARG, "VPS_FLAG_SHARE_ENERGY: a whole momentum field (no component mask, no reference bug), then "
                                           "the energy field with VPS_FLAG_REUSE_SORT");
  }
  if (only) {
    if (quantity == VPS_ENERGY) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_fft_zy: VPS_FLAG_COMPONENTS with the (scalar) energy field");
    const int all[3] = {q.chan[0], q.chan[1], q.chan[2]};
    q.ncomp = 0;
    for (int c = 0; c < 3; ++c)
      if (only & (1 << c)) q.chan[q.ncomp++] = all[c];
  }
  *pq = q;
  return VPS_OK;
}

int vps_deposit_fft_zy(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                       const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx, int quantity,
                       int flags, void* spec_dev, void* nyq_dev, void* work_dev) {
  VPS_ENTER(ctx);
  if (!spec_dev || !nyq_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_fft_zy: null buffer");
  return deposit_fft_impl(ctx, pos_dev, pos_is_f64, vel_dev, rho_dev, np, N, Lbox, x0, nx, quantity, flags, spec_dev,
                          nyq_dev, nullptr, work_dev);
}

size_t vps_deposit_fft_z_workspace_bytes(int64_t np, int N, int nx) {
  if (np < 0 || N < 16 || nx < 1) return 0;
  return dep_layout(np, 4, make_pencils(N, 0, nx, vps_pencil_tp(N))).total;
}

int vps_deposit_fft_z(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                      const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx, int quantity,
                      int flags, void* zimg_dev, void* work_dev) {
  VPS_ENTER(ctx);
  if (!zimg_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_fft_z: null buffer");
  return deposit_fft_impl(ctx, pos_dev, pos_is_f64, vel_dev, rho_dev, np, N, Lbox, x0, nx, quantity, flags, nullptr,
                          nullptr, zimg_dev, work_dev);
}

int64_t vps_count_in_slab(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, int64_t np, int N, double Lbox, int x0, int nx) {
  if (!ctx) return VPS_ERR_ARG;
  vps_device_guard guard(ctx);
  int rc = check_deposit_args(ctx, "vps_count_in_slab", np, N, Lbox, x0, nx);
  if (rc) return rc;
  if (np == 0) return 0;
  if (!pos_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_count_in_slab: null buffer");
  const Bricks b = make_pencils(N, x0, nx, 1);
  unsigned long long* d = nullptr;
  VPS_HIP_CHECK(ctx, hipMalloc(&d, sizeof(unsigned long long)));
  hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), ctx->stream);
  const unsigned grid = (unsigned)std::min<long long>((np + 255) / 256, 4096);
  if (e == hipSuccess) {
    if (pos_is_f64)
      hipLaunchKernelGGL(count_in_slab_kernel<double>, dim3(grid), dim3(256), 0, ctx->stream, reinterpret_cast<const double*>(pos_dev),
                         (long long)np, Lbox / (double)N, (double)N, b, d);
    else
      hipLaunchKernelGGL(count_in_slab_kernel<float>, dim3(grid), dim3(256), 0, ctx->stream, reinterpret_cast<const float*>(pos_dev),
                         (long long)np, (float)(Lbox / (double)N), (float)N, b, d);
    e = hipGetLastError();
  }
  unsigned long long h = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return vps_fail(ctx, VPS_ERR_HIP, "vps_count_in_slab: %s", hipGetErrorString(e));
  return (int64_t)h;
}

int vps_deposit_plan(vps_ctx* ctx, int64_t np, int C, int N, int x0, int nx, int pencil, int64_t np_slab,
                     int64_t out[VPS_DEPOSIT_PLAN_FIELDS]) {
  if (!ctx) return VPS_ERR_ARG;
  if (!out) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_plan: null buffer");
  int rc = check_deposit_args(ctx, "vps_deposit_plan", np, N, 1.0, x0, nx);
  if (rc) return rc;
  if (C != 1 && C != 3 && C != 4) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_deposit_plan: C=%d channels (supported: 1,3,4)", C);
  if (pencil && (C != 4 || N < 16 || !vps_pencil_supported(ctx, N)))
    return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_deposit_plan: pencil buckets carry [rho v, rho] records (C = 4) at an N the fused path supports");
  if (np_slab >= 0 && !pencil) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_plan: a slab-sized workspace exists for pencil buckets only");
  const Bricks b = pencil ? make_pencils(N, x0, nx, vps_pencil_tp(N)) : make_bricks(N, x0, nx, C);
  const DepLayout l = dep_layout(np, C, b, np_slab >= 0 ? np_slab : -1);
  const SortGeom& g = l.geom;
  const size_t lds_staged = sort_staged_lds(g, C, SORT_ITEMS);
  out[0] = b.bx; out[1] = b.by; out[2] = b.bz;
  out[3] = l.nbricks;
  out[4] = b.cells;
  out[5] = g.cshift >= 0;
  out[6] = l.two_level;
  out[7] = l.wide_keys;
  out[8] = g.gshift;
  out[9] = g.ngroups;
  out[10] = g.nchunks;
  out[11] = l.two_level && sort_staged() && lds_staged <= ctx->lds_per_cu;   // (sort_records' rule)
  out[12] = (int64_t)lds_staged;
  out[13] = l.recompute;
  out[14] = l.cap_in;
  return VPS_OK;
}

size_t vps_deposit_fft_z_workspace_bytes_slab(int64_t np, int64_t np_slab, int N, int nx) {
  if (np < 0 || np_slab < 0 || N < 16 || nx < 1) return 0;
  return dep_layout(np, 4, make_pencils(N, 0, nx, vps_pencil_tp(N)), np_slab).total;
}

int vps_deposit_fft_z_slab(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                           const float* rho_dev, int64_t np, int64_t np_slab, int N, double Lbox, int x0, int nx, int quantity,
                           int flags, void* zimg_dev, void* work_dev) {
  VPS_ENTER(ctx);
  if (!zimg_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_fft_z_slab: null buffer");
  if (np_slab < 0) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_fft_z_slab: np_slab < 0");
  return deposit_fft_impl(ctx, pos_dev, pos_is_f64, vel_dev, rho_dev, np, N, Lbox, x0, nx, quantity, flags, nullptr,
                          nullptr, zimg_dev, work_dev, np_slab);
}

// zimg_dev != NULL: stop after the z pass, the images [component][B | BN] go to zimg_dev (work_dev then only holds the sort)
static int deposit_fft_impl(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                            const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx, int quantity,
                            int flags, void* spec_dev, void* nyq_dev, void* zimg_dev, void* work_dev, int64_t np_cap) {
  int rc = check_deposit_args(ctx, "vps_deposit_fft_zy", np, N, Lbox, x0, nx);
  if (rc) return rc;
  if ((rc = refuse_assign_flags(ctx, "vps_deposit_fft_zy", flags))) return rc;
  if ((rc = vps_refuse_second_moment(ctx, "vps_deposit_fft_zy", quantity, "the pencil kernel has no fifth channel"))) return rc;
  if ((rc = vps_refuse_grid_only(ctx, "vps_deposit_fft_zy", quantity, "a pencil does not hold a cell's neighbours in x and y"))) return rc;
  if (!vps_deposit_fft_zy_supported(ctx, N, quantity))
    return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_deposit_fft_zy: N=%d quantity=%d not supported by the fused path", N, quantity);
  if ((rc = vps_check_weighted(ctx, "vps_deposit_fft_zy", quantity, flags))) return rc;
  if (!work_dev || (np > 0 && (!pos_dev || !vel_dev || !rho_dev)))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_fft_zy: null buffer");
  const Bricks b = make_pencils(N, x0, nx, vps_pencil_tp(N));
  char* work = reinterpret_cast<char*>(work_dev);
  DepLayout l;
  if (flags & VPS_FLAG_REUSE_SORT) {
    l = dep_layout(np, 4, b, np_cap);     // the caller vouches that the records of the previous call are still there
  } else {
    rc = pos_is_f64 ? sort_rhov_records<double>(ctx, reinterpret_cast<const double*>(pos_dev), vel_dev, rho_dev, np, N, Lbox, b, work, &l, np_cap)
                    : sort_rhov_records<float>(ctx, reinterpret_cast<const float*>(pos_dev), vel_dev, rho_dev, np, N, Lbox, b, work, &l, np_cap);
    if (rc) return rc;
  }
  PencilQuantity pq;
  if ((rc = pencil_quantity(ctx, quantity, flags, &pq))) return rc;
  const double lc = Lbox / (double)N;
  // (the sort's rank array -- one word per particle, dead once the records are in place -- is the kernel's per-record scratch)
  return vps_fft_pencil_zy(ctx, N, nx, reinterpret_cast<const unsigned*>(work + l.records),
                           reinterpret_cast<const unsigned*>(work + l.start), reinterpret_cast<float*>(work + l.ranks), pq,
                           (float)(lc * lc * lc), spec_dev, nyq_dev, zimg_dev ? zimg_dev : (void*)(work + l.total));
}

int vps_density_velocity_vector(vps_ctx* ctx, const float* vel_dev, const float* rho_dev, int64_t np,
                                float* out_dev) {
  VPS_ENTER(ctx);
  if (np < 0) return vps_fail(ctx, VPS_ERR_ARG, "vps_density_velocity_vector: np < 0");
  if (np == 0) return VPS_OK;
  if (!vel_dev || !rho_dev || !out_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_density_velocity_vector: null buffer");
  if ((np + 255) / 256 > 0x7fffffffLL) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "np too large for one launch");
  {
    vps_launch_timer tm(ctx, VPS_K_MISC);
    hipLaunchKernelGGL(rhov_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, vel_dev,
                       rho_dev, (long long)np, out_dev);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

int vps_assign_expand(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* payload_dev, int64_t np,
                      int C, int N, double Lbox, int order, float* pos_out_dev, float* payload_out_dev) {
  VPS_ENTER(ctx);
  if (np < 0 || N < 1 || !(Lbox > 0) || C < 1 || C > 4) return vps_fail(ctx, VPS_ERR_ARG, "vps_assign_expand: bad np/N/Lbox/C");
  if (order != 2 && order != 3) return vps_fail(ctx, VPS_ERR_ARG, "vps_assign_expand: order must be 2 (CIC) or 3 (TSC)");
  if (np == 0) return VPS_OK;
  if (!pos_dev || !payload_dev || !pos_out_dev || !payload_out_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_assign_expand: null buffer");
  if ((np + 255) / 256 > 0x7fffffffLL) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "np too large for one launch");
  const double lcell = Lbox / (double)N;
  {
    vps_launch_timer tm(ctx, VPS_K_DEPOSIT);
    const unsigned blocks = (unsigned)((np + 255) / 256);
    if (pos_is_f64)
      hipLaunchKernelGGL(assign_expand_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream,
                         reinterpret_cast<const double*>(pos_dev), payload_dev, (long long)np, C, N, lcell,
                         order, pos_out_dev, payload_out_dev);
    else
      hipLaunchKernelGGL(assign_expand_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream,
                         reinterpret_cast<const float*>(pos_dev), payload_dev, (long long)np, C, N, lcell,
                         order, pos_out_dev, payload_out_dev);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

size_t vps_deposit_assign_workspace_bytes(int64_t np, int C, int N, int order) {
  if (np < 0 || N < 1 || (C != 1 && C != 3 && C != 4) || (order != 2 && order != 3)) return 0;
  return assign_plan(np, C, N).l.total;
}

int vps_deposit_assign(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* payload_dev, int64_t np, int C, int N,
                       double Lbox, int order, float* grid_dev, void* work_dev) {
  VPS_ENTER(ctx);
  int rc = check_assign_args(ctx, "vps_deposit_assign", np, C, N, order);
  if (rc) return rc;
  if (!(Lbox > 0)) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_assign: bad Lbox");
  if (!grid_dev || !work_dev || (np > 0 && (!pos_dev || !payload_dev)))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_assign: null buffer");
#define VPS_DEP(CC)                                                                                              \
  (pos_is_f64 ? deposit_assign_order<double, CC>(ctx, pos_dev, payload_dev, np, N, Lbox, order, grid_dev, work_dev) \
              : deposit_assign_order<float, CC>(ctx, pos_dev, payload_dev, np, N, Lbox, order, grid_dev, work_dev))
  switch (C) {
    case 1: return VPS_DEP(1);
    case 3: return VPS_DEP(3);
    default: return VPS_DEP(4);
  }
#undef VPS_DEP
}

int vps_deposit_assign_plan(vps_ctx* ctx, int64_t np, int C, int N, int order, int64_t out[VPS_DEPOSIT_ASSIGN_PLAN_FIELDS]) {
  if (!ctx) return VPS_ERR_ARG;
  if (!out) return vps_fail(ctx, VPS_ERR_ARG, "vps_deposit_assign_plan: null buffer");
  int rc = check_assign_args(ctx, "vps_deposit_assign_plan", np, C, N, order);
  if (rc) return rc;
  const AssignPlan p = assign_plan(np, C, N);
  const Bricks& b = p.b;
  const size_t lds_staged = sort_staged_lds(p.l.geom, C + 6, SORT_ITEMS);
  // the largest set of source buckets any brick gathers from (8 unless a partial last brick is narrower than order - 1 cells)
  int most[3] = {1, 1, 1};
  const int bw[3] = {b.bx, b.by, b.bz}, nb[3] = {b.nbx, b.nby, b.nbz};
  for (int a = 0; a < 3; ++a)
    for (int i = 0; i < nb[a]; ++i) {
      int src[3];
      most[a] = std::max(most[a], assign_axis_sources(i, bw[a], N, order, src));
    }
  out[0] = b.bx; out[1] = b.by; out[2] = b.bz;
  out[3] = b.nbx; out[4] = b.nby; out[5] = b.nbz;
  out[6] = p.l.nbricks;
  out[7] = b.cells;
  out[8] = p.l.two_level;
  out[9] = p.l.wide_keys;
  out[10] = C + 7;
  out[11] = p.l.two_level && sort_staged() && lds_staged <= ctx->lds_per_cu;   // (sort_records' rule)
  out[12] = p.l.geom.gshift;
  out[13] = (int64_t)most[0] * most[1] * most[2];
  return VPS_OK;
}

int vps_field_algebra_out(vps_ctx* ctx, int quantity, int flags, double Lcell, const float* chans_dev,
                          int64_t ncell, float* out_dev);

int vps_field_algebra(vps_ctx* ctx, int quantity, int flags, double Lcell, float* chans_dev,
                      int64_t ncell) {
  return vps_field_algebra_out(ctx, quantity, flags, Lcell, chans_dev, ncell, nullptr);
}

// The velocity-gradient codes of vps_field_algebra_out (include/vps_hip.h, "Velocity-gradient fields"): every refusal names the
// quantity and comes before anything is enqueued; then one stencil launch (gradient.hip).
static int field_gradient(vps_ctx* ctx, int quantity, int flags, double Lcell, const float* chans_dev, int64_t ncell,
                          float* out_dev) {
  const char* name = vps_gradient_name(quantity);
#define VPS_GRAD_FAIL(fmt, ...) vps_fail(ctx, VPS_ERR_ARG, "vps_field_algebra: quantity %d (%s) " fmt, quantity, name, ##__VA_ARGS__)
  if (!out_dev) return VPS_GRAD_FAIL("has no in-place form: it reads a cell's neighbours, out_dev is required (vps_field_algebra_out)");
  if (flags != VPS_FLAG_INPUT_IS_VM)
    return VPS_GRAD_FAIL("takes the [v, mass] channels of a gridded field: VPS_FLAG_INPUT_IS_VM and no other flag (flags 0x%x)", flags);
  const float h = (float)(1.0 / (2.0 * Lcell));
  if (!(Lcell > 0) || !(h > 0.f) || !std::isfinite(h))
    return VPS_GRAD_FAIL("needs a positive, finite Lcell whose h = (float)(1 / (2 Lcell)) is positive and finite too");
  if (!chans_dev) return VPS_GRAD_FAIL("null buffer");
  // N: the integer cube root, checked exactly (cbrt is within an ulp: N^3 < 2^63 for every candidate)
  int64_t N = ncell > 0 ? (int64_t)std::llround(std::cbrt((double)ncell)) : 0;
  if (ncell <= 0 || (ncell & 3) || N < 4 || N > 32768 || N * N * N != ncell)
    return VPS_GRAD_FAIL("needs a whole periodic grid: ncell = N^3 for an integer N >= 4 and a multiple of 4 (ncell %lld)", (long long)ncell);
  if (((uintptr_t)chans_dev | (uintptr_t)out_dev) & 15) return VPS_GRAD_FAIL("needs 16-byte aligned buffers");
  const uintptr_t c0 = (uintptr_t)chans_dev, c1 = c0 + 4 * (uintptr_t)ncell * sizeof(float);
  const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)vps_quantity_channels(quantity) * (uintptr_t)ncell * sizeof(float);
  if (o0 < c1 && c0 < o1) return VPS_GRAD_FAIL("out_dev overlaps chans_dev: the stencil reads what a neighbour's store would change");
#undef VPS_GRAD_FAIL
  {
    vps_launch_timer tm(ctx, VPS_K_ALGEBRA);
    vps_gradient_launch(ctx, quantity, (int)N, h, chans_dev, out_dev);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

// The box-filter codes of vps_field_algebra_out (include/vps_hip.h, "Box-filtered fields"): every refusal names the quantity and
// comes before anything is enqueued; then one launch (filter.hip).
static int field_filter(vps_ctx* ctx, int quantity, int flags, double Lcell, const float* chans_dev, int64_t ncell,
                        float* out_dev) {
  const char* name = vps_filter_name(quantity);
#define VPS_FILT_FAIL(code, fmt, ...) vps_fail(ctx, code, "vps_field_algebra: quantity %d (%s) " fmt, quantity, name, ##__VA_ARGS__)
  if (!out_dev) return VPS_FILT_FAIL(VPS_ERR_ARG, "has no in-place form: it reads a box of cells, out_dev is required (vps_field_algebra_out)");
  if (!(flags & VPS_FLAG_INPUT_IS_VM) || (flags & ~(VPS_FLAG_INPUT_IS_VM | VPS_FLAG_FILTER_MASK)))
    return VPS_FILT_FAIL(VPS_ERR_ARG, "takes the [v, mass] channels of a gridded field: VPS_FLAG_INPUT_IS_VM, VPS_FLAG_FILTER(m) and no other flag (flags 0x%x)", flags);
  if (!(Lcell > 0) || !std::isfinite(Lcell)) return VPS_FILT_FAIL(VPS_ERR_ARG, "needs a positive, finite Lcell");
  if (!chans_dev) return VPS_FILT_FAIL(VPS_ERR_ARG, "null buffer");
  int64_t N = ncell > 0 ? (int64_t)std::llround(std::cbrt((double)ncell)) : 0;
  if (ncell <= 0 || (N & 1) || N < 4 || N > 32768 || N * N * N != ncell)
    return VPS_FILT_FAIL(VPS_ERR_ARG, "needs a whole periodic grid: ncell = N^3 for an even N >= 4 (ncell %lld)", (long long)ncell);
  const int m = (flags & VPS_FLAG_FILTER_MASK) >> 12;
  if (m < 1) return VPS_FILT_FAIL(VPS_ERR_ARG, "needs a half-width: VPS_FLAG_FILTER(m) with m >= 1 (flags 0x%x)", flags);
  if (2 * (int64_t)m + 1 > N) return VPS_FILT_FAIL(VPS_ERR_ARG, "the box of 2m + 1 = %d cells is wider than the grid (N = %lld)", 2 * m + 1, (long long)N);
  if (((uintptr_t)chans_dev | (uintptr_t)out_dev) & 15) return VPS_FILT_FAIL(VPS_ERR_ARG, "needs 16-byte aligned buffers");
  const uintptr_t c0 = (uintptr_t)chans_dev, c1 = c0 + 4 * (uintptr_t)ncell * sizeof(float);
  const uintptr_t o0 = (uintptr_t)out_dev, o1 = o0 + (uintptr_t)vps_quantity_channels(quantity) * (uintptr_t)ncell * sizeof(float);
  if (o0 < c1 && c0 < o1) return VPS_FILT_FAIL(VPS_ERR_ARG, "out_dev overlaps chans_dev: a box sum reads what a neighbour's store would change");
  if (m > VPS_FILTER_MAX_HALF_WIDTH)
    return VPS_FILT_FAIL(VPS_ERR_UNSUPPORTED, "half-width m = %d: the largest half-width taken is %d (the LDS plan of the kernel)", m, VPS_FILTER_MAX_HALF_WIDTH);
#undef VPS_FILT_FAIL
  const double w = 2.0 * m + 1.0;
  const float c = (float)(1.0 / (w * w * w));
  {
    vps_launch_timer tm(ctx, VPS_K_ALGEBRA);
    vps_filter_launch(ctx, quantity, (int)N, m, c, chans_dev, out_dev);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

int vps_field_algebra_out(vps_ctx* ctx, int quantity, int flags, double Lcell, const float* chans_dev,
                          int64_t ncell, float* out_dev) {
  VPS_ENTER(ctx);
  if (!vps_quantity_valid(quantity)) return vps_fail(ctx, VPS_ERR_ARG, "vps_field_algebra: quantity %d", quantity);
  if (vps_quantity_filter(quantity)) return field_filter(ctx, quantity, flags, Lcell, chans_dev, ncell, out_dev);
  if (vps_quantity_gradient(quantity)) return field_gradient(ctx, quantity, flags, Lcell, chans_dev, ncell, out_dev);
  if (int rc = vps_refuse_second_moment(ctx, "vps_field_algebra", quantity, "a 4-channel grid does not hold a second moment")) return rc;
  if (int rc = vps_check_weighted(ctx, "vps_field_algebra", quantity, flags)) return rc;
  if (int rc = refuse_assign_flags(ctx, "vps_field_algebra", flags)) return rc;
  if (ncell < 0 || (ncell & 3)) return vps_fail(ctx, VPS_ERR_ARG, "vps_field_algebra: ncell must be a multiple of 4");
  if (ncell == 0) return VPS_OK;
  if (!chans_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_field_algebra: null buffer");
  const long long nthreads = ncell / 4;
  const unsigned blocks = (unsigned)((nthreads + 255) / 256);
  {
    vps_launch_timer tm(ctx, VPS_K_ALGEBRA);
    const int rcq = dispatch_quantity(quantity, [&](auto q) {
      hipLaunchKernelGGL(field_quantity_kernel<decltype(q)::value>, dim3(blocks), dim3(256), 0, ctx->stream,
                         const_cast<float*>(chans_dev), (long long)ncell, flags, grid_par(ctx, quantity, Lcell), out_dev);
      return VPS_OK;
    });
    if (rcq) return vps_fail(ctx, rcq, "vps_field_algebra: quantity %d", quantity);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

}  // extern "C"
