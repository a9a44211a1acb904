// z and y passes: the two transposing kernels and their launcher.  Kernel unit only (fft_parts.hip).
#pragma once
#include "fft_line.h"

namespace {

// ------------------------------------------------------------------------------
// Transposing pass (z pass: REAL=true, y pass: REAL=false).
// One workgroup transforms T lines a0..a0+T-1 of batch b and writes, for every
// output index k, the T results to T contiguous complex slots out[b][k][a0..].
// ------------------------------------------------------------------------------
// NTEMP: non-temporal loads and stores (y pass of images up to ~0.75 GB: -4..-9 % there; on larger ones +2..+5 % with
// 64-byte segments, -6 % with full 128-byte lines)
// KG: the Nyquist-plane launch of the chunked exchange (output rows shifted per destination rank, PassParams::kg) -- its own
// instantiation, so that the main passes carry no per-element division
template <int NC, int T, bool REAL, bool NTEMP = false, bool KG = false>
__global__ void __launch_bounds__(T* PlanInfo<NC>::L)
    fft_transpose_pass(const PassParams p) {
  typedef PlanInfo<NC> PI;
  constexpr int L = PI::L, RL = PI::RL, NT = T * L;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  cf* tw_lds = reinterpret_cast<cf*>(smem_raw);
  cf* buf = tw_lds + PI::TWL;
  const cf* tw = PI::TWLDS ? tw_lds : p.tw_stage;

  const int tid = threadIdx.x;
  const int t = tid / L, l = tid % L;
  const int tiles = (p.A + T - 1) / T;
  // Tiles narrower than a 128-byte cache line (T < 16): run the 16/T tiles that share output
  // lines on ONE XCD, close in time, so that its L2 merges their partial-line writes before
  // write-back.  Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8, observed,
  // speed only): hardware block h = 8 s + x handles logical tile G*(8*(s/G) + x) + s%G.
  unsigned bid = blockIdx.x;
  constexpr unsigned G = (T < 16) ? 16 / T : 1;
  if constexpr (G > 1) {
    const unsigned span = 8 * G;
    if (bid / span < gridDim.x / span) {   // whole groups only; the tail keeps the identity map
      const unsigned base = (bid / span) * span, h = bid % span;
      bid = base + G * (h % 8) + (h / 8);
    }
  }
  const int bo = bid / tiles;                 // batch as the output sees it
  const int a0 = (bid % tiles) * T;
  const long long b = p.bg ? (long long)(bo / p.bg) * p.bg_in + p.b_off + (long long)(bo % p.bg) * p.bg_step : bo;   // batch as the input sees it
  const long long ogap = p.bg ? (long long)(bo / p.bg) * p.bg_gap : 0;

  if constexpr (PI::TWLDS)
    for (int i = tid; i < PI::TW; i += NT) tw_lds[i] = p.tw_stage[i];

  cf v[RL];
  {
    const bool live = (a0 + t) < p.A;
    constexpr int R = PI::R0, NB = RL / R;
    if constexpr (REAL) {
      // line of 2*NC floats read as NC packed complex z[j] = x[2j] + i x[2j+1]
      const cf* src = reinterpret_cast<const cf*>(reinterpret_cast<const float*>(p.in) +
                                                   (long long)b * p.in_sb +
                                                   (long long)(a0 + t) * p.in_sa);
#pragma unroll
      for (int m = 0; m < NB; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r)
          v[m * R + r] = live ? load_stream(&src[l + L * m + r * (NC / R)]) : make_float2(0.f, 0.f);
      if (p.in_w) {
        const cf* srcw = reinterpret_cast<const cf*>(reinterpret_cast<const float*>(p.in_w) +
                                                      (long long)b * p.in_sb + (long long)(a0 + t) * p.in_sa);
#pragma unroll
        for (int m = 0; m < NB; ++m)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const cf w = live ? srcw[l + L * m + r * (NC / R)] : make_float2(0.f, 0.f);
            v[m * R + r] = make_float2(v[m * R + r].x * w.x, v[m * R + r].y * w.y);
          }
      }
    } else {
      const cf* src = reinterpret_cast<const cf*>(p.in) + (long long)b * p.in_sb +
                      (long long)(a0 + t) * p.in_sa;
#pragma unroll
      for (int m = 0; m < NB; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if constexpr (NTEMP) {
            v[m * R + r] = live ? load_stream(&src[l + L * m + r * (NC / R)]) : make_float2(0.f, 0.f);
          } else {
            v[m * R + r] = live ? src[l + L * m + r * (NC / R)] : make_float2(0.f, 0.f);
          }
        }
    }
  }
  __syncthreads();  // twiddle image visible
  // a line's lanes sit in one wave when L divides 64: stage exchanges then need no workgroup barrier
  constexpr bool WSYNC = (L <= 64) && (64 % L == 0);
  fft_from_regs<NC, WSYNC>(v, buf + t * PI::PITCH, tw, l);
  __syncthreads();  // every lane done with the per-line buffers
  // transposed image [k][t]
#pragma unroll
  for (int i = 0; i < RL; ++i) buf[tridx<T>(out_index<NC>(l, i), t)] = v[i];
  __syncthreads();

  cf* out = reinterpret_cast<cf*>(p.out) + (long long)bo * p.out_ob + ogap + a0;
  if constexpr (!REAL) {
    const int kc = p.kcut ? p.kcut[p.kz_fixed >= 0 ? p.kz_fixed : (int)b] : NC;
    const int2 pt = p.ptab ? p.ptab[bo % p.bg] : make_int2(0, -1);   // (uniform over the workgroup)
    out += (long long)pt.x * p.out_ok;
#pragma unroll 4
    for (int i = 0; i < RL; ++i) {
      const int idx = tid + i * NT;
      const int tt = idx % T, k = idx / T;
      if (a0 + tt < p.A && min(k, NC - k) <= kc) {
        const cf val = buf[tridx<T>(k, tt)];
        long long o = (long long)packed_row(k, NC, pt.y) * p.out_ok + tt;
        if constexpr (KG) o += (long long)(k / p.kg) * p.kg_gap;
        if constexpr (NTEMP)
          store_stream(&out[o], val);
        else
          out[o] = val;
      }
    }
  } else {
    cf* nyq = reinterpret_cast<cf*>(p.out_nyq) + (long long)b * p.nyq_ob + a0;
    r2c_store_tile<NC, T, NT, true>(buf, tid, p.tw_r2c, out, p.out_ok, nyq, p.A - a0);
  }
}


// ------------------------------------------------------------------------------
// Wide transposing y pass for lines whose 16-line tile does not fit LDS (NC > 1024) or fills it (NC = 1024).
// What bounds the transposing pass of long lines is the WRITE pattern, not the transform: a plain
// transposing copy of a 2048^3 half spectrum (tools/micro/transpose_bw.hip) moves 3.9 TB/s with the
// 64-byte segments of 8-line tiles and 5.5 TB/s with full 128-byte lines -- and fft_transpose_pass<2048, 8>
// ran at exactly the former.  This kernel writes 128-byte segments with the LDS of an 8-line tile:
// a workgroup loads 2 x TG lines, transforms them one TG-line group after the other through the same
// exchange buffers (the first group's spectrum waits in registers), and then stages the transposed
// image in two k-halves [NC/2][2 TG] -- after the last radix-R stage register slot (m, r) holds
// k = l + L m + r NC/R, so r < R/2 is exactly the lower half.
// ------------------------------------------------------------------------------
// (1024-point lines: two 512-thread workgroups fit a CU's LDS, so the kernel is held to the 128 VGPRs of four waves per SIMD)
template <int NC, int TG, int L, bool NTEMP>
__global__ void __launch_bounds__(TG* L, (NC == 1024 ? 4 : 1))
    fft_transpose_pass_wide(const PassParams p) {
  typedef PlanInfo<NC> PI;
  constexpr int RL = NC / L, NT = TG * L, T = 2 * TG;
  constexpr int R = LastRadix<NC>::R;
  static_assert((R & 1) == 0 && (NC & 1) == 0, "the image is staged in two k-halves");
  static_assert(((NC / 2) * T) % NT == 0, "whole store rounds");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  cf* tw_lds = reinterpret_cast<cf*>(smem_raw);
  cf* buf = tw_lds + PI::TWL;
  const cf* tw = PI::TWLDS ? tw_lds : p.tw_stage;

  const int tid = threadIdx.x;
  const unsigned tiles = (unsigned)((p.A + T - 1) / T);
  const unsigned ntiles = tiles * (unsigned)p.B;   // (the launcher checks that this fits)

  if constexpr (PI::TWLDS)
    for (int i = tid; i < PI::TW; i += NT) tw_lds[i] = p.tw_stage[i];

  // Register budget: 1024 threads leave 128 VGPRs, and two groups' values are 64 of them.  Left to itself the compiler
  // forms the LDS / global addresses of BOTH transforms and of the store loops once, ahead of the first transform, and
  // keeps ~40 of them live throughout (84 bytes per lane spilled, +4 % run time).  A thread index passed through an
  // empty asm is a new value to it: addresses derived from it are formed where they are used.
  auto fresh = [](int x) {
    asm volatile("" : "+v"(x));
    return x;
  };
  // stage-0 inputs of line `first` + (line of thread `who`) of tile `tile` (who: the thread index, possibly laundered)
  auto load_line = [&](cf (&v)[RL], unsigned tile, int who, int first) {
    constexpr int R0 = PI::R0, NB = RL / R0;
    const int bo_ = (int)(tile / tiles), a0_ = (int)(tile % tiles) * T;
    const long long b_ = p.bg ? (long long)(bo_ / p.bg) * p.bg_in + p.b_off + (long long)(bo_ % p.bg) * p.bg_step : bo_;
    const int tl = who / L, ll = who % L;
    const bool live = (a0_ + first + tl) < p.A;
    const cf* src = reinterpret_cast<const cf*>(p.in) + b_ * p.in_sb + (long long)(a0_ + first + tl) * p.in_sa;
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int r = 0; r < R0; ++r) {
        const int j = ll + L * m + r * (NC / R0);
        if constexpr (NTEMP) {   // (streaming loads: 13.7 against 14.4 ms per 2048^3 launch with plain ones)
          v[m * R0 + r] = live ? load_stream(&src[j]) : make_float2(0.f, 0.f);
        } else {
          v[m * R0 + r] = live ? src[j] : make_float2(0.f, 0.f);
        }
      }
  };
  constexpr bool WSYNC = (L <= 64) && (64 % L == 0);
  // Persistent: a workgroup walks tiles blockIdx.x, + gridDim.x, ...  ONE 1024-thread workgroup fits a CU, so nothing else
  // would overlap a tile's first loads or its last stores: the next tile's first group is requested as soon as the registers
  // of the current tile's lower half are free -- it flies behind the second half's image and stores.
  // (Placement measured and not kept: each XCD taking gridDim.x / 8 CONSECUTIVE tiles of every group of gridDim.x, so that its L2
  // owns contiguous 4 KB runs of an output row instead of every 8th 128-byte piece: 12.59 against 12.59 ms per 2048^3 launch.)
  cf v0[RL], v1[RL];
  unsigned tile = blockIdx.x;
  if (tile < ntiles) load_line(v0, tile, tid, 0);
  __syncthreads();  // twiddle image visible
  for (; tile < ntiles; tile = (ntiles - tile > gridDim.x) ? tile + gridDim.x : ntiles) {
    const int bo = (int)(tile / tiles);                 // batch as the output sees it
    const int a0 = (int)(tile % tiles) * T;
    const long long b = p.bg ? (long long)(bo / p.bg) * p.bg_in + p.b_off + (long long)(bo % p.bg) * p.bg_step : bo;   // batch as the input sees it
    const long long ogap = p.bg ? (long long)(bo / p.bg) * p.bg_gap : 0;
    {
      const int tida = fresh(tid);
      fft_from_regs_l<NC, L, WSYNC>(v0, buf + (tida / L) * PI::PITCH, tw, tida % L);
    }
    // (requesting the second group ahead of the first transform: 14.1 against 12.4 ms per 2048^3 launch)
    load_line(v1, tile, fresh(tid), TG);
    __syncthreads();  // every lane done with the per-line buffers
    {
      const int tidb = fresh(tid);
      fft_from_regs_l<NC, L, WSYNC>(v1, buf + (tidb / L) * PI::PITCH, tw, tidb % L);
    }

    const int2 pt = p.ptab ? p.ptab[bo % p.bg] : make_int2(0, -1);   // (uniform over the workgroup)
    cf* out = reinterpret_cast<cf*>(p.out) + (long long)bo * p.out_ob + ogap + (long long)pt.x * p.out_ok + a0;
    const int kc = p.kcut ? p.kcut[p.kz_fixed >= 0 ? p.kz_fixed : (int)b] : NC;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      __syncthreads();  // exchange buffers / the previous half image are free
      const int tid2 = fresh(tid);
#pragma unroll
      for (int i = 0; i < RL; ++i) {
        if (((i % R) >= R / 2) == (h == 1)) {
          const int k = out_index_l<NC, L>(tid2 % L, i) - h * (NC / 2);
          buf[tridx<T>(k, tid2 / L)] = v0[i];
          buf[tridx<T>(k, tid2 / L + TG)] = v1[i];
        }
      }
      // the lower halves are in the image, the upper halves just went: v0 takes the next tile's first group
      // (requested after the barrier instead: 12.96 against 12.43 ms)
      if (h == 1 && ntiles - tile > gridDim.x) load_line(v0, tile + gridDim.x, fresh(tid), 0);
      __syncthreads();
      constexpr int IT = (NC / 2) * T / NT;
      // 16-byte stores: a lane owns the lines (tt, tt + 1) of a row, a 128-byte segment leaves as eight dwordx4 stores instead of
      // sixteen dwordx2 (the pencil kernel's epilogue gained 7 % from the same change: these epilogues are bound by store ISSUE)
      if (((p.out_ok | p.A) & 1) == 0 && (reinterpret_cast<size_t>(out) & 15) == 0) {   // (uniform)
        static_assert(IT % 2 == 0, "whole rounds of line pairs");
#pragma unroll 4
        for (int i = 0; i < IT / 2; ++i) {
          const int idx = tid2 + i * NT;
          const int tt = (idx % (T / 2)) * 2, kk = idx / (T / 2), k = kk + h * (NC / 2);
          if (a0 + tt < p.A && min(k, NC - k) <= kc) {
            const cf va = buf[tridx<T>(kk, tt)], vb = buf[tridx<T>(kk, tt + 1)];
            const long long o = (long long)packed_row(k, NC, pt.y) * p.out_ok + tt;
            const vps_f4 val = {va.x, va.y, vb.x, vb.y};
            if constexpr (NTEMP)
              __builtin_nontemporal_store(val, reinterpret_cast<vps_f4*>(&out[o]));
            else
              *reinterpret_cast<vps_f4*>(&out[o]) = val;
          }
        }
        continue;
      }
#pragma unroll 4
      for (int i = 0; i < IT; ++i) {
        const int idx = tid2 + i * NT;
        const int tt = idx % T, kk = idx / T, k = kk + h * (NC / 2);
        if (a0 + tt < p.A && min(k, NC - k) <= kc) {
          const cf val = buf[tridx<T>(kk, tt)];
          const long long o = (long long)packed_row(k, NC, pt.y) * p.out_ok + tt;
          if constexpr (NTEMP)
            store_stream(&out[o], val);
          else
            out[o] = val;
        }
      }
    }
    __syncthreads();  // the image is consumed before the next tile's exchanges overwrite it
  }
}

// lines whose y pass runs the wide kernel (two 8-line groups per workgroup)
template <int NC>
constexpr bool wide_transpose() {
  // 1024: the 16-line tile fits LDS as ONE 1024-thread workgroup per CU (1.80 ms per 1024^3 launch); as two groups of 8 it is
  // two persistent 512-thread workgroups per CU: 1.58 ms.  512 (32 lines, 256-byte segments): 0.20 -> 0.21 ms, not taken.
  // 2000: 800 threads x 2 x 20 points do not fit 128 VGPRs.
  return NC == 1024 || NC == 1536 || NC == 2048 || NC == 4096;
}

template <int NC, int T>
size_t transpose_lds_bytes() {
  typedef PlanInfo<NC> PI;
  size_t lines = (size_t)T * PI::PITCH;
  size_t tr = (size_t)NC * T;
  return (PI::TWL + (lines > tr ? lines : tr)) * sizeof(cf);
}

template <int NC, bool REAL>
int launch_transpose(vps_ctx* ctx, const PassParams& p, int kind) {
  // 1024-point complex lines: 16-line tiles (128-byte segments, one 1024-thread workgroup per
  // CU) measured 13 % faster than 8-line tiles; for the packed-real 1024-point z pass the
  // 8-line tiles with XCD-paired placement are faster.
  // (4-line tiles with four-way XCD grouping were slower at 2048: 2.59 vs 2.25 ms.)
  // (Persistent workgroups that request the next tile's lines before transforming the current one -- to overlap load,
  // transform and store where only ONE workgroup fits a CU -- measured at 2048^3: at the plan's 1024 threads the 32
  // prefetch registers spill (128-VGPR cap); on half the lanes per line (512 threads, 256 VGPRs, wave-level exchanges)
  // still 124 bytes per lane of scratch and 164 ms per step of y passes against 113 ms for this kernel.  This kernel itself
  // on half the lanes (512 threads, 197 VGPRs, no spill, wave-level exchanges): 121.5 against 115.6 ms.  The persistent
  // form at the plan's 1024 threads with the lane indices re-materialised per tile (117 VGPRs, no spill): 137.9 ms.  Not kept.)
  typedef PlanInfo<NC> PI;
  constexpr int T = (NC == 1024 && !REAL) ? 16 : transpose_T<NC>();
  // (single planes -- the Nyquist plane's own launch -- stay with the narrow kernel: nothing to gain there, and the
  // profiler's per-kernel averages then describe the main launches only)
  if constexpr (!REAL && wide_transpose<NC>()) if (p.B > 1) {
    // 2 x T lines per workgroup, 128-byte output segments (fft_transpose_pass_wide)
    constexpr int TGW = transpose_T<NC>();   // lines per group
    const size_t lds = transpose_lds_bytes<NC, TGW>();
    // full 128-byte lines written once: non-temporal stores (2048^3: 3.93 against 4.56 ms per 512-row slab; with the 64-byte
    // segments of the 8-line kernel they were a loss on images this large).  On half the plan's lanes per line (512 threads)
    // the kernel spills 47 registers.
    constexpr int LW = PI::L;
    auto kern = fft_transpose_pass_wide<NC, TGW, LW, true>;
    if (lds > 64 * 1024)
      VPS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const long long tiles = (p.A + 2 * TGW - 1) / (2 * TGW);
    long long grid = tiles * p.B;
    if (grid <= 0 || grid > 0x7fffffffLL) return vps_fail(ctx, VPS_ERR_ARG, "fft grid out of range");
    // as many workgroups as fit the chip at once (one per CU at 2048), each walking its share of the tiles: 2048^3 launch
    // 13.4 -> 12.4 ms, a 256-row slab 1.80 -> 1.63 ms against one workgroup per tile
    const long long per_cu = (long long)(ctx->lds_per_cu / lds) > 0 ? (long long)(ctx->lds_per_cu / lds) : 1;
    if (grid > (long long)ctx->num_cu * per_cu) grid = (long long)ctx->num_cu * per_cu;
    {
      vps_launch_timer tm(ctx, kind);
      hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(TGW * LW), lds, ctx->stream, p);
    }
    VPS_HIP_CHECK(ctx, hipGetLastError());
    return VPS_OK;
  }
  const size_t lds = transpose_lds_bytes<NC, T>();
  auto kern = fft_transpose_pass<NC, T, REAL>;
  if constexpr (!REAL) {
    const double image_bytes = 8.0 * (double)p.A * (double)p.B * (double)NC;
    // non-temporal loads and stores: always with full 128-byte segments (T >= 16: 1024^3 y pass 1.79 against 1.90 ms);
    // with narrower tiles only while the image is small (partial lines have to meet in L2 first)
    if (image_bytes <= 768.0 * 1048576.0 || T >= 16) kern = fft_transpose_pass<NC, T, REAL, true>;
    if (p.kg) kern = fft_transpose_pass<NC, T, REAL, true, true>;   // Nyquist plane of a chunked exchange (one small image)
  }
  if (lds > 64 * 1024)
    VPS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const long long tiles = (p.A + T - 1) / T;
  const long long grid = tiles * p.B;
  if (grid <= 0 || grid > 0x7fffffffLL) return vps_fail(ctx, VPS_ERR_ARG, "fft grid out of range");
  {
    vps_launch_timer tm(ctx, kind);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(T * PI::L), lds, ctx->stream, p);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

}  // namespace
