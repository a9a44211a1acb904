// Velocity-gradient fields of a whole periodic grid (include/vps_hip.h, "Velocity-gradient fields"): VPS_DIVERGENCE,
// VPS_VORTICITY and VPS_STRAIN_RATE from second-order central differences of the three velocity channels.  The one stencil
// kernel of the library: every other grid kernel is per-cell algebra or an FFT line.
//
// HBM-bound by design.  The floor is one read of each velocity channel and one write of each output channel, 4 bytes each per
// cell: 16 B (divergence), 24 B (vorticity), 36 B (strain rate).  To stay near it
//   - a workgroup of 256 threads owns a tile of GR_TY = 16 rows (y) by 16 lanes x VEC cells (z: 64 cells with 16-byte accesses,
//     32 cells with 8-byte accesses where N % 4 == 2 and odd rows are only 8-byte aligned) and MARCHES ALONG X over a chunk of
//     planes.  A thread keeps its VEC cells of the planes x - 1, x, x + 1 of the three components in registers, so d/dx costs no
//     second fetch: every plane of the chunk is loaded once per tile, plus the two planes outside the chunk's ends;
//   - plane x of the tile goes through LDS with a one-row halo in y and a one-cell halo in z (fetched by the first lanes of waves
//     0 and 1: 2 rows and 2 columns per component that needs them), double buffered: ONE barrier per plane.  d/dy reads rows
//     ly and ly + 2 of the LDS tile with the access width of the global loads, d/dz takes its inner neighbours from the thread's
//     own registers and the two outer ones from LDS;
//   - the loads of plane x + 2 are issued before the arithmetic of plane x and consumed one iteration later;
//   - a template over the quantity forms only the derivatives it needs (3 of 9 for the divergence, 6 for the vorticity, all 9 for
//     the strain rate), and with them only the halos and register planes those need: the divergence keeps no x-neighbours of
//     uy and uz, no y-halo of ux and uz, no z-halo of ux and uy.
// LDS: 2 buffers x 3 components x 18 rows x (16 VEC + 8) floats = 31,104 B (VEC 4) / 17,280 B (VEC 2).  Workgroups per CU, VEC 4:
// five for the divergence and the vorticity (72 / 96 VGPRs; the LDS sets the limit), four for the strain rate (116 VGPRs: four
// waves per SIMD); VEC 2: eight (46 / 58 / 64 VGPRs).  Every output element has exactly one writer; there are no atomics.
// The halo fetch is lopsided: the 2 x 16 cells of the z columns are single 4-byte loads at stride N, 32 cache lines per
// component and plane, issued by half of wave 1 alone, and the row halos by half of wave 0 alone.
//
// Arithmetic: float32, no contraction, in the fixed order of the header -- d = (u(+1) - u(-1)) * h with h = (float)(1 / (2 Lcell))
// from the host; exact for integer velocities and a power-of-two Lcell (tests/test_gpu_gradient.py compares bits).
#pragma clang fp contract(off)

#include "vps_internal.h"
#include "quantity.h"

namespace {

constexpr int GR_TY = 16;          // rows of a tile = rows of threads
constexpr int GR_LZ = 16;          // lanes along z; a lane holds VEC consecutive cells
constexpr int GR_THREADS = GR_TY * GR_LZ;
constexpr int GR_PAD = 4;          // LDS row: [3 unused][z - 1 halo][16 VEC cells][z + 1 halo][3 unused]: the cells start 16-byte aligned

// is d u_c / d x_a part of QUANT?
template <int QUANT>
constexpr bool gr_need(int c, int a) {
  return QUANT == VPS_DIVERGENCE ? c == a : QUANT == VPS_VORTICITY ? c != a : true;
}

template <int VEC>
__device__ __forceinline__ void gr_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  }
}
template <int VEC>
__device__ __forceinline__ void gr_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
}

// One plane of the tile as a thread holds it: its own VEC cells of each component, and -- in the lanes that fetch one -- a piece
// of the halo (a row piece of VEC cells, or one cell of a z column in h[c][0]).
template <int VEC>
struct GrPlane {
  float u[3][VEC];
  float h[3][VEC];
};

template <int QUANT, int VEC>
__global__ void __launch_bounds__(GR_THREADS)
    gradient_kernel(const float* __restrict__ chans, float* __restrict__ out, int N, int xchunk, float h) {
  constexpr int TZ = GR_LZ * VEC, RS = TZ + 2 * GR_PAD, NCH = vps_quantity_channels(QUANT);
  __shared__ __attribute__((aligned(16))) float tile[2][3][GR_TY + 2][RS];

  const int tid = threadIdx.x, lz = tid % GR_LZ, ly = tid / GR_LZ;
  const int z0 = blockIdx.x * TZ, y0 = blockIdx.y * GR_TY;
  const int w = min(TZ, N - z0), hgt = min(GR_TY, N - y0);       // the tile's cells: N is a multiple of VEC, so is w
  const int xs = blockIdx.z * xchunk, len = min(xchunk, N - xs);
  const size_t plane = (size_t)N * N, ncell = plane * N;

  // what this thread fetches of a plane: its own cells ...
  const bool own = lz * VEC < w && ly < hgt;
  const size_t own_off = (size_t)(y0 + ly) * N + z0 + lz * VEC;
  // ... and, in the first 32 lanes of waves 0 and 1, a piece of the halo: wave 0 the rows y0 - 1 and y0 + hgt (VEC cells per
  // lane), wave 1 the columns z0 - 1 and z0 + w (one cell per lane), all wrapped
  static_assert(2 * GR_LZ <= 64 && 2 * GR_TY <= 64 && GR_THREADS >= 128, "the halo lanes of waves 0 and 1");
  const int hk = tid & 63, hper = tid < 64 ? GR_LZ : GR_TY, hwhich = hk / hper, hidx = hk % hper;
  const bool hrow = tid < 2 * GR_LZ && hidx * VEC < w;
  const bool hcol = tid >= 64 && tid < 64 + 2 * GR_TY && hidx < hgt;
  size_t halo_off = 0;
  int halo_lds = 0;                                              // offset in a component's [GR_TY + 2][RS] image
  if (hrow) {
    const int y = hwhich ? (y0 + hgt == N ? 0 : y0 + hgt) : (y0 == 0 ? N - 1 : y0 - 1);
    halo_off = (size_t)y * N + z0 + hidx * VEC;
    halo_lds = (hwhich ? hgt + 1 : 0) * RS + GR_PAD + hidx * VEC;
  } else if (hcol) {
    const int z = hwhich ? (z0 + w == N ? 0 : z0 + w) : (z0 == 0 ? N - 1 : z0 - 1);
    halo_off = (size_t)(y0 + hidx) * N + z;
    halo_lds = (hidx + 1) * RS + (hwhich ? GR_PAD + w : GR_PAD - 1);
  }
  const int own_lds = (ly + 1) * RS + GR_PAD + lz * VEC;

  auto fetch = [&](int x, GrPlane<VEC>& p) {                     // x in [-1, N]: wrapped
    const size_t base = (size_t)(x < 0 ? N - 1 : x >= N ? 0 : x) * plane;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* src = chans + c * ncell + base;
      if (own) gr_load<VEC>(src + own_off, p.u[c]);
      if (gr_need<QUANT>(c, 1) && hrow) gr_load<VEC>(src + halo_off, p.h[c]);
      if (gr_need<QUANT>(c, 2) && hcol) p.h[c][0] = src[halo_off];
    }
  };
  auto stage = [&](int buf, const GrPlane<VEC>& p) {             // a fetched plane -> LDS: only what d/dy and d/dz will read
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* img = &tile[buf][c][0][0];
      if ((gr_need<QUANT>(c, 1) || gr_need<QUANT>(c, 2)) && own) gr_store<VEC>(img + own_lds, p.u[c]);
      if (gr_need<QUANT>(c, 1) && hrow) gr_store<VEC>(img + halo_lds, p.h[c]);
      if (gr_need<QUANT>(c, 2) && hcol) img[halo_lds] = p.h[c][0];
    }
  };

  GrPlane<VEC> prev = {}, cur = {}, next = {}, far = {};
  fetch(xs - 1, prev);
  fetch(xs, cur);
  fetch(xs + 1, next);
  stage(0, cur);
  __syncthreads();

  for (int it = 0; it < len; ++it) {
    const int x = xs + it, buf = it & 1;
    const bool more = it + 1 < len;                              // uniform
    if (more) fetch(x + 2, far);
    if (own) {
      // d[c][a][v] = d u_c / d x_a in cell v of the thread
      float d[3][3][VEC];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* img = &tile[buf][c][0][0];
        if (gr_need<QUANT>(c, 0)) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) d[c][0][v] = (next.u[c][v] - prev.u[c][v]) * h;
        }
        if (gr_need<QUANT>(c, 1)) {
          float ym[VEC], yp[VEC];
          gr_load<VEC>(img + own_lds - RS, ym);
          gr_load<VEC>(img + own_lds + RS, yp);
#pragma unroll
          for (int v = 0; v < VEC; ++v) d[c][1][v] = (yp[v] - ym[v]) * h;
        }
        if (gr_need<QUANT>(c, 2)) {
          const float zm = img[own_lds - 1], zp = img[own_lds + VEC];
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            d[c][2][v] = ((v + 1 < VEC ? cur.u[c][v + 1] : zp) - (v > 0 ? cur.u[c][v - 1] : zm)) * h;
        }
      }
      float o[NCH][VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if constexpr (QUANT == VPS_DIVERGENCE) {
          o[0][v] = (d[0][0][v] + d[1][1][v]) + d[2][2][v];
        } else if constexpr (QUANT == VPS_VORTICITY) {
          o[0][v] = d[2][1][v] - d[1][2][v];
          o[1][v] = d[0][2][v] - d[2][0][v];
          o[2][v] = d[1][0][v] - d[0][1][v];
        } else {
          o[0][v] = d[0][0][v];
          o[1][v] = d[1][1][v];
          o[2][v] = d[2][2][v];
          o[3][v] = 0.5f * (d[0][1][v] + d[1][0][v]);
          o[4][v] = 0.5f * (d[0][2][v] + d[2][0][v]);
          o[5][v] = 0.5f * (d[1][2][v] + d[2][1][v]);
        }
      }
      float* dst = out + (size_t)x * plane + own_off;
#pragma unroll
      for (int k = 0; k < NCH; ++k) gr_store<VEC>(dst + k * ncell, o[k]);
    }
    if (more) {
      stage(buf ^ 1, next);           // plane x + 1, fetched one iteration ago; the reads of this buffer ended before the last barrier
      __syncthreads();
      prev = cur;
      cur = next;
      next = far;
    }
  }
}

template <int QUANT>
void gradient_launch_q(vps_ctx* ctx, int N, float h, const float* chans, float* out) {
  // 16-byte accesses where every row starts 16-byte aligned; else (N % 4 == 2) 8-byte accesses throughout
  const int vec = (N & 3) == 0 ? 4 : 2, tz = GR_LZ * vec;
  const int ntz = (N + tz - 1) / tz, nty = (N + GR_TY - 1) / GR_TY;
  // x chunks: enough workgroups for four per CU several times over, but chunks of 64 planes or more where N allows (a chunk
  // fetches two planes beyond its own)
  const long long tiles = (long long)ntz * nty, want = 16LL * ctx->num_cu;
  const int nxc = (int)std::max(1LL, std::min((want + tiles - 1) / tiles, (long long)(N / 64)));
  const int xchunk = (N + nxc - 1) / nxc;
  const dim3 grid(ntz, nty, (N + xchunk - 1) / xchunk);
  if (vec == 4)
    hipLaunchKernelGGL((gradient_kernel<QUANT, 4>), grid, dim3(GR_THREADS), 0, ctx->stream, chans, out, N, xchunk, h);
  else
    hipLaunchKernelGGL((gradient_kernel<QUANT, 2>), grid, dim3(GR_THREADS), 0, ctx->stream, chans, out, N, xchunk, h);
}

}  // namespace

void vps_gradient_launch(vps_ctx* ctx, int quantity, int N, float h, const float* chans, float* out) {
  switch (quantity) {
    case VPS_DIVERGENCE: return gradient_launch_q<VPS_DIVERGENCE>(ctx, N, h, chans, out);
    case VPS_VORTICITY: return gradient_launch_q<VPS_VORTICITY>(ctx, N, h, chans, out);
    default: return gradient_launch_q<VPS_STRAIN_RATE>(ctx, N, h, chans, out);
  }
}
