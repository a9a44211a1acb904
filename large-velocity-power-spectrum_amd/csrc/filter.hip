// Box-filtered fields of a whole periodic grid (include/vps_hip.h, "Box-filtered fields"): VPS_FILTERED_VM and
// VPS_FILTERED_STRESS, the mass-weighted box filter of half-width m (a box of (2m+1)^3 cells) of the [u, mass] channels.  The one
// spatial filter of the library; its tiling is that of the stencil kernel (gradient.hip).
//
// A workgroup of 256 threads owns a tile of FT_TY = 16 rows (y) by 16 lanes x VEC cells (z: 64 cells with 16-byte stores, 32 with
// 8-byte stores where N % 4 == 2) and MARCHES ALONG X over a chunk of at most 64 planes.  The sums are NS = 5 (VM: M, P_x, P_y,
// P_z and the COUNT of cells with mass) or 11 (stress: those and S_xx, S_yy, S_zz, S_xy, S_xz, S_yz); the template over the code
// carries no more.  The count is a sum of ones: exact in float32, so an empty box is found exactly and gives exact zeros even
// where the running sums of M and P keep a rounding residue from the mass that has left the box.  Per plane x:
//   1. the four input channels of plane x + m of the tile plus a halo of m cells, (16 + 2m) x (16 VEC + 2m) cells, go through
//      registers into LDS once (4-byte loads, every index wrapped; fetched one phase ahead of their use);
//   2. a thread takes the rows ly and ly + 16 of that region and its VEC cells of them: the products p_c = mass u_c and
//      s_ij = p_i u_j are formed on the fly from LDS -- no product ever goes to HBM -- and summed along z, the first cell of the
//      group directly over its 2m + 1 cells, the next ones by a sliding sum (+ the cell that enters, - the cell that leaves);
//   3. the z sums of the plane are ADDED to the thread's running x sums R (2 rows x NS x VEC registers); the same two steps for
//      plane x - m - 1 SUBTRACT it.  At the start of a chunk R is the direct sum of the planes x - m .. x + m - 1: the chain of
//      roundings is bounded by the chunk, not by N;
//   4. R goes to LDS, six sums at a time (the stress: two rounds), and the owner of an output cell adds the 2m + 1 rows of its
//      column directly, then forms the quotient / the stress and stores VEC cells per channel.
// Every output element has exactly one writer; there are no atomics; the call allocates nothing.
//
// Traffic model, bytes per cell: writes 16 (VM) / 24 (stress); reads 2 x 16 x A(m) x (1 + (2m + 1) / (2 XC)) with the halo
// amplification A(m) = (16 + 2m)(TZ + 2m) / (16 TZ) -- plane x + m and plane x - m - 1 are each read once per tile, and a chunk
// of XC planes reads 2m planes ahead of its first output; TZ = 64: A = 1.16 (m = 1), 1.69 (m = 4), 2.50 (m = 8).  The second
// read of a plane comes 2m + 1 planes after the first and the halos are shared with the neighbouring tiles, so HBM is
// EXPECTED to see little more than the floor of one read and one write, 32 B (VM) / 40 B (stress) per cell, and the model to be
// what L2 and the LDS fill see: a supposition, no memory counter was read.
// LDS: ONE buffer that holds the input region (4 x 32 x (16 VEC + 16) floats) and then the rounds of R (6 x 32 x 16 VEC floats):
// 49,152 B (VEC 4) / 24,576 B (VEC 2); eight barriers per plane for the stress, six for VM.  VGPRs: VM 192 (VEC 4) / 110
// (VEC 2), stress 256 / 156, no spills -- two waves per SIMD with VEC 4 (two workgroups per CU), four / three with VEC 2.  The
// measurements and what keeps the kernel from the floor are in DESIGN.md section 3.
//
// Rounding chain of one box sum, K = 6m + 134: two roundings in a product (p_c, then s_ij); 2m additions for the first z sum and
// 2 (VEC - 1) <= 6 for the sliding steps behind it; 2m additions for the direct x sum at the start of a chunk and 2 per plane
// after it, 2 (64 - 1) = 126 at most; 2m additions along y.  A rounding of a sliding sum is relative to the window sum it is made
// at, NOT to the window sum of the cell that is finally written: with A(i) = sum_W(i) |terms|,
//   |error of a box sum at (x, y, z)| <= K 2^-24 max A(x', y, z'),  x' <= x in the chunk of x,  z' <= z in the VEC group of z
// (the z sums of a plane are the same numbers when it enters and when it leaves, so their roundings leave with it; the roundings
// of the x steps stay until the chunk ends).  Where the mass falls by many orders of magnitude within a chunk's planes, the sums
// in the faint region are only as good as that: M there may be off by more than itself.  Emptiness does not depend on it: the
// count is exact.  The quotient, the product P_i P_j, the subtraction and the scaling by c add one rounding each, in the fixed
// order of the header (tests/filter_ref.py: bars carries all of it through to the outputs).
#pragma clang fp contract(off)

#include <algorithm>

#include "vps_internal.h"
#include "quantity.h"

namespace {

constexpr int FT_TY = 16;                      // rows of a tile = rows of threads
constexpr int FT_LZ = 16;                      // lanes along z; a lane holds VEC consecutive cells
constexpr int FT_THREADS = FT_TY * FT_LZ;
constexpr int FT_MMAX = VPS_FILTER_MAX_HALF_WIDTH;
constexpr int FT_RY = FT_TY + 2 * FT_MMAX;     // rows of the largest region
constexpr int FT_ITEMS = FT_RY / FT_TY;        // region rows a thread sums along z: ly, ly + 16
constexpr int FT_XCHUNK_MAX = 64;              // the longest chunk: the x part of K
constexpr int FT_XCHUNK_MIN = 32;              // ... and the shortest one where N allows (a chunk reads 2m planes ahead of itself)
constexpr int FT_ROUND = 6;                    // sums per y round: the stress's 11 in two rounds, VM's 5 in one
static_assert(FT_RY % FT_TY == 0, "whole rows of threads");

template <int VEC>
__device__ __forceinline__ void ft_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
}
template <int VEC>
__device__ __forceinline__ void ft_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  }
}

// the NS terms of one cell, in the order M, P_x, P_y, P_z, [S_xx, S_yy, S_zz, S_xy, S_xz, S_yz,] and LAST the count: 1 where the
// cell holds mass, else 0 -- a sum of at most 17^3 ones is exact in float32 in any order of additions and subtractions, so
// "the box holds no mass" is decided exactly, whatever residue the running sums of M keep from cells that have left the box
template <int NS>
__device__ __forceinline__ void ft_terms(const float* img, int chan_stride, int at, float (&t)[NS]) {
  const float ux = img[at], uy = img[chan_stride + at], uz = img[2 * chan_stride + at], ms = img[3 * chan_stride + at];
  t[0] = ms;
  t[1] = ms * ux;
  t[2] = ms * uy;
  t[3] = ms * uz;
  t[NS - 1] = ms != 0.f ? 1.f : 0.f;
  if constexpr (NS == 11) {
    t[4] = t[1] * ux;
    t[5] = t[2] * uy;
    t[6] = t[3] * uz;
    t[7] = t[1] * uy;
    t[8] = t[1] * uz;
    t[9] = t[2] * uz;
  }
}

template <int QUANT, int VEC>
__global__ void __launch_bounds__(FT_THREADS) __attribute__((amdgpu_waves_per_eu(2)))
    filter_kernel(const float* __restrict__ chans, float* __restrict__ out, int N, int m, int xchunk, float c) {
  constexpr int TZ = FT_LZ * VEC, RZ = TZ + 2 * FT_MMAX, NS = QUANT == VPS_FILTERED_VM ? 5 : 11;
  constexpr int CS = FT_RY * RZ;                                  // floats of one channel's region image
  constexpr int CPT = (CS + FT_THREADS - 1) / FT_THREADS;         // region cells a thread fetches, at most
  constexpr int NR = (NS + FT_ROUND - 1) / FT_ROUND;              // y rounds
  constexpr int LDS_FLOATS = 4 * CS > FT_ROUND * FT_RY * TZ ? 4 * CS : FT_ROUND * FT_RY * TZ;   // the input region, then a round of R
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];

  const int tid = threadIdx.x, lz = tid % FT_LZ, ly = tid / FT_LZ;
  const int z0 = blockIdx.x * TZ, y0 = blockIdx.y * FT_TY;
  const int xs = blockIdx.z * xchunk, len = min(xchunk, N - xs);
  const int ry = FT_TY + 2 * m, rz = TZ + 2 * m, ncr = ry * rz, w2 = 2 * m + 1;
  const size_t plane = (size_t)N * N, ncell = plane * N;
  const bool own = z0 + lz * VEC < N && y0 + ly < N;              // N is a multiple of VEC: the whole group or none of it
  const size_t own_off = (size_t)(y0 + ly) * N + z0 + lz * VEC;

  // the region cells this thread fetches: in-plane offset (wrapped; N may be far smaller than the region) and LDS offset
  int goff[CPT], loff[CPT];
#pragma unroll
  for (int j = 0; j < CPT; ++j) {
    const int idx = tid + j * FT_THREADS;
    loff[j] = -1;
    goff[j] = 0;
    if (idx < ncr) {
      const int r = idx / rz, k = idx - r * rz;
      int y = (y0 - m + r) % N, z = (z0 - m + k) % N;
      y += y < 0 ? N : 0;
      z += z < 0 ? N : 0;
      goff[j] = y * N + z;
      loff[j] = r * RZ + k;
    }
  }

  float g[CPT][4];
  auto fetch = [&](int x) {                                        // x in [-N, 2N): wrapped
    const size_t base = (size_t)(x < 0 ? x + N : x >= N ? x - N : x) * plane;
#pragma unroll
    for (int j = 0; j < CPT; ++j)
      if (loff[j] >= 0) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) g[j][ch] = chans[ch * ncell + base + goff[j]];
      }
  };
  auto stage = [&]() {                                             // the fetched plane -> LDS (the readers of the buffer have passed a barrier)
#pragma unroll
    for (int j = 0; j < CPT; ++j)
      if (loff[j] >= 0) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) lds[ch * CS + loff[j]] = g[j][ch];
      }
  };

  float R[FT_ITEMS][NS][VEC];
#pragma unroll
  for (int i = 0; i < FT_ITEMS; ++i)
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int v = 0; v < VEC; ++v) R[i][s][v] = 0.f;

  // z sums of the staged plane, added to (sign > 0) or subtracted from the running x sums
  auto zpass = [&](bool add) {
#pragma unroll
    for (int i = 0; i < FT_ITEMS; ++i) {
      const int r = ly + i * FT_TY;
      if (r < ry) {
        const int at0 = r * RZ + lz * VEC;
        float acc[NS], t[NS];
        ft_terms<NS>(lds, CS, at0, acc);
        for (int k = 1; k < w2; ++k) {
          ft_terms<NS>(lds, CS, at0 + k, t);
#pragma unroll
          for (int s = 0; s < NS; ++s) acc[s] += t[s];
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          if (v > 0) {
            ft_terms<NS>(lds, CS, at0 + v + 2 * m, t);
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] += t[s];
            ft_terms<NS>(lds, CS, at0 + v - 1, t);
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s] -= t[s];
          }
#pragma unroll
          for (int s = 0; s < NS; ++s) R[i][s][v] = add ? R[i][s][v] + acc[s] : R[i][s][v] - acc[s];
        }
      }
    }
  };

  // the chunk's start: R = the direct sum of the planes xs - m .. xs + m - 1
  fetch(xs - m);
  for (int p = 0; p < 2 * m; ++p) {
    stage();
    __syncthreads();
    fetch(xs - m + p + 1);                                         // (the last one: plane xs + m, the first iteration's)
    zpass(true);
    __syncthreads();
  }

  for (int it = 0; it < len; ++it) {
    const int x = xs + it;
    stage();                                                       // plane x + m
    __syncthreads();
    if (it > 0) fetch(x - m - 1);
    else if (len > 1) fetch(x + m + 1);
    zpass(true);
    __syncthreads();
    if (it > 0) {
      stage();                                                     // plane x - m - 1
      __syncthreads();
      if (it + 1 < len) fetch(x + m + 1);
      zpass(false);
      __syncthreads();
    }

    // y sums: a round of R through LDS, the owner of a cell adds the 2m + 1 rows of its column
    float Y[NS][VEC];
#pragma unroll
    for (int rd = 0; rd < NR; ++rd) {
      constexpr int RS = FT_RY * TZ;                               // floats of one sum's image
#pragma unroll
      for (int i = 0; i < FT_ITEMS; ++i) {
        const int r = ly + i * FT_TY;
        if (r < ry) {
#pragma unroll
          for (int s = rd * FT_ROUND; s < NS && s < (rd + 1) * FT_ROUND; ++s)
            ft_store<VEC>(&lds[(s - rd * FT_ROUND) * RS + r * TZ + lz * VEC], R[i][s]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int s = rd * FT_ROUND; s < NS && s < (rd + 1) * FT_ROUND; ++s) {
        const float* col = &lds[(s - rd * FT_ROUND) * RS + ly * TZ + lz * VEC];
        ft_load<VEC>(col, Y[s]);
        for (int d = 1; d < w2; ++d) {
          float t[VEC];
          ft_load<VEC>(col + d * TZ, t);
#pragma unroll
          for (int v = 0; v < VEC; ++v) Y[s][v] += t[v];
        }
      }
      __syncthreads();
    }

    if (own) {
      constexpr int NCH = vps_quantity_channels(QUANT);
      float o[NCH][VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float M = Y[0][v];
        const bool has = Y[NS - 1][v] != 0.f && M != 0.f;           // the exact count of cells with mass (and a sum to divide by)
        if constexpr (QUANT == VPS_FILTERED_VM) {
#pragma unroll
          for (int a = 0; a < 3; ++a) o[a][v] = has ? Y[1 + a][v] / M : 0.f;
          o[3][v] = has ? M * c : 0.f;
        } else {
          constexpr int I[6] = {0, 1, 2, 0, 0, 1}, J[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            float t = Y[4 + k][v] - (Y[1 + I[k]][v] * Y[1 + J[k]][v]) / M;
            if (k < 3) t = t < 0.f ? 0.f : t;
            o[k][v] = has ? t * c : 0.f;
          }
        }
      }
      float* dst = out + (size_t)x * plane + own_off;
#pragma unroll
      for (int k = 0; k < NCH; ++k) ft_store<VEC>(dst + k * ncell, o[k]);
    }
  }
}

template <int QUANT>
void filter_launch_q(vps_ctx* ctx, int N, int m, float c, const float* chans, float* out) {
  // 16-byte stores where every row starts 16-byte aligned; else (N % 4 == 2) 8-byte stores throughout
  const int vec = (N & 3) == 0 ? 4 : 2, tz = FT_LZ * vec;
  const int ntz = (N + tz - 1) / tz, nty = (N + FT_TY - 1) / FT_TY;
  // x chunks: never longer than 64 planes (the rounding chain), as many as give four workgroups per CU several times over, but
  // not shorter than 32 planes where N allows (a chunk sums 2m planes before its first output)
  const long long tiles = (long long)ntz * nty, want = 16LL * ctx->num_cu;
  const long long lo = (N + FT_XCHUNK_MAX - 1) / FT_XCHUNK_MAX, hi = std::max(lo, (long long)(N / FT_XCHUNK_MIN));
  const int nxc = (int)std::max(lo, std::min((want + tiles - 1) / tiles, hi));
  const int xchunk = (N + nxc - 1) / nxc;
  const dim3 grid(ntz, nty, (N + xchunk - 1) / xchunk);
  if (vec == 4)
    hipLaunchKernelGGL((filter_kernel<QUANT, 4>), grid, dim3(FT_THREADS), 0, ctx->stream, chans, out, N, m, xchunk, c);
  else
    hipLaunchKernelGGL((filter_kernel<QUANT, 2>), grid, dim3(FT_THREADS), 0, ctx->stream, chans, out, N, m, xchunk, c);
}

}  // namespace

void vps_filter_launch(vps_ctx* ctx, int quantity, int N, int m, float c, const float* chans, float* out) {
  if (quantity == VPS_FILTERED_VM) filter_launch_q<VPS_FILTERED_VM>(ctx, N, m, c, chans, out);
  else filter_launch_q<VPS_FILTERED_STRESS>(ctx, N, m, c, chans, out);
}
