// Fused deposit + z pass: the two pencil kernels and their launcher.  Kernel unit only (fft_parts.hip).
#pragma once
#include "fft_line.h"
#include "quantity.h"

namespace {

// ------------------------------------------------------------------------------
// Fused deposit + field algebra + z pass ("pencil" kernel).  A pencil is the TP z-lines
// (x, y0..y0+TP-1, all z) that one z-pass tile transforms.  The deposit stage has sorted
// the particle records {cell-in-pencil, rho vx, rho vy, rho vz, rho} by pencil
// (deposit.hip), so one workgroup accumulates rho of its pencil in LDS (vps_lds_add), keeps
// 1/rho of its own stage-0 cells in registers, then per component accumulates rho*v in the same
// LDS region, forms v = rho v / rho (or p = rho v Lcell^3) as it loads the FFT's stage-0 inputs,
// transforms and writes B[x][kz][y] -- the real-space grid is never written to or read from
// HBM, and the accumulator, exchange buffers and transposed image all share one LDS region.
// ------------------------------------------------------------------------------

// The per-record factor of the dividing launches: 1 / rho (v_rcp_f32), or for the density-weighted velocity rho^(alpha - 1) as
// exp2((alpha - 1) log2 rho) on the transcendental units (v_log_f32, one multiply, v_exp_f32: once per record and launch, outside
// every round).  Empty cells give 0 for every alpha (the NaN -> 0 rule of interp.py:329-331).  rho is a sum of positive
// densities; float32 denormals and powers beyond the float32 range are outside the contract (include/vps_hip.h).
template <bool WEIGHTED>
__device__ __forceinline__ float pencil_rho_factor(float r, float wexp) {
  if constexpr (WEIGHTED)
    return vps_rho_weight(r, wexp);
  else
    return r != 0.f ? __builtin_amdgcn_rcpf(r) : 0.f;
}

// The per-cell value of the scalar density launches (DENSITY instantiation) from the cell's density total: rho^sexp as
// exp2(sexp log2 rho), or ln rho = log2 rho * ln 2 (quantity.h: vps_rho_scalar_nz), on the same units; 0 in empty cells for both.  (The plain density,
// PENCIL_SCALAR_RHO, never gets here: the accumulator goes into the transform as it is.)
__device__ __forceinline__ float pencil_rho_scalar(float r, int mode, float sexp) {
  const float s = vps_rho_scalar_nz(r, mode == PENCIL_SCALAR_LOG, sexp);
  return r != 0.f ? s : 0.f;
}

// One workgroup per pencil, on the plan's lanes per line; four waves per SIMD (measured at 512^3 / 1024^3 / 2048^3) need <= 128 VGPRs.
// DENSITY: ONE field from ONE round -- the accumulated rho, turned per cell into rho^alpha or ln rho by its records (nothing
// at all for the plain density) -- and one transform, stored as a workgroup's last field.
template <int NC, int TP, bool ENERGY = false, bool WEIGHTED = false, bool DENSITY = false>
__global__ void __launch_bounds__(TP* PlanInfo<NC>::L, 4) pencil_fft_z_kernel(const PencilParams p) {
  static_assert(!(DENSITY && (ENERGY || WEIGHTED)), "the scalar density launch is a form of its own");
  typedef PlanInfo<NC> PI;
  constexpr int L = PI::L, RL = PI::RL, NT = TP * L, N = 2 * NC;
  constexpr int ACC = TP * N;                       // floats of one accumulator
  constexpr int LINES = TP * PI::PITCH * 2;         // floats of the exchange buffers
  constexpr int SHARED = (ACC > LINES ? ACC : LINES);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  // ONE LDS region serves, in turn, as the rho accumulator, each rho*v accumulator and the FFT's
  // exchange / transposed-image buffer.
  float* acc = reinterpret_cast<float*>(smem_raw);
  cf* buf = reinterpret_cast<cf*>(acc);
  cf* tw_lds = reinterpret_cast<cf*>(acc + SHARED);
  const cf* tw = PI::TWLDS ? tw_lds : p.tw_stage;

  const int tid = threadIdx.x;
  const int t = tid / L, l = tid % L;
  // Pencils narrower than a 128-byte output line (TP < 16): the 16/TP pencils that share output lines are consecutive
  // pencil numbers; run them on ONE XCD, close in time, so that its L2 merges their partial-line writes (same map as
  // fft_transpose_pass: hardware block h = 8 s + x handles logical pencil G*(8*(s/G) + x) + s%G)
  constexpr unsigned GP = (TP < 16) ? 16 / TP : 1;
  unsigned pencil = blockIdx.x;
  if constexpr (GP > 1) {
    constexpr unsigned span = 8 * GP;
    if (pencil / span < p.npencils / span) {   // whole groups only; the tail keeps the identity map
      const unsigned h = pencil % span;
      pencil = (pencil / span) * span + GP * (h % 8) + (h / 8);
    }
  }
  const unsigned s = p.start[pencil], e = p.start[pencil + 1];
  if constexpr (PI::TWLDS)
    for (int i = tid; i < PI::TW; i += NT) tw_lds[i] = p.tw_stage[i];
  // What a CELL needs besides the sums -- 1/rho (velocity), the running sum of (rho v_c)^2 (energy) -- is kept per RECORD:
  // every record of a cell reads the cell's total from the accumulator and carries the same value.  A per-cell table would
  // be RL register pairs per lane next to the RL transform registers (it was: the kernel then fit four waves per SIMD only
  // up to 1024-cell lines, and not at all for energy); per record it is KR registers, whatever the line length.
  // The cells of the first KR*NT records of the bucket stay in registers; the value each round adds (rho, then rho v_c) is
  // fetched one round ahead, so the loads fly behind the previous round's FFT.  Only unusually full pencils read records
  // inside a round (tail loops below); their per-record value lives in p.side[record].
  // register-resident record groups: enough for a typical bucket (~1.2 x mean occupancy at the bench
  // densities) -- 3 x 256 threads at 512^3, 2 x 512 at 1024^3 (measured optimum each)
  constexpr int KR = NT >= 512 ? 2 : (NT >= 256 ? 3 : 4);
  unsigned rloc[KR];
  float rval[KR];
  float rrec[KR];   // 1/rho of the record's cell (velocity; WEIGHTED: rho^(alpha-1)) / sum over components of (rho v_c)^2 of its cell (ENERGY)
                    // / rho^alpha or ln rho of its cell (DENSITY)
  auto fetch = [&](int word) {   // record word 1..3: rho v_c, 4: rho
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const unsigned j = s + tid + k * NT;
      if (j < e) rval[k] = __uint_as_float(p.records[(size_t)j * 5 + word]);
    }
  };
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const unsigned j = s + tid + k * NT;
    rloc[k] = (j < e) ? p.records[(size_t)j * 5] : 0xffffffffu;
  }
  const bool divide = !ENERGY && !DENSITY && p.divide;
  fetch((DENSITY || divide) ? 4 : 1 + p.chan[0]);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int R0 = PI::R0, NB0 = RL / R0;
  const int x = pencil / p.nby, y0 = (pencil % p.nby) * TP;
  // more than two particles per cell on average: hot cells are likely, take the native atomics (vps_lds_add)
  const bool crowded = (e - s) > 2u * (unsigned)ACC;
#pragma unroll
  for (int k = 0; k < KR; ++k) rrec[k] = 1.f;
  const unsigned tail0 = s + tid + KR * NT;   // this thread's first record beyond the register-resident ones
  if (divide) {
    for (int i = tid; i < ACC / 4; i += NT) reinterpret_cast<float4*>(acc)[i] = zero4;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (rloc[k] != 0xffffffffu) vps_lds_add(&acc[rloc[k]], rval[k], crowded);
    fetch(1 + p.chan[0]);
    for (unsigned j = tail0; j < e; j += NT) {
      const unsigned* rec = p.records + (size_t)j * 5;
      vps_lds_add(&acc[rec[0]], __uint_as_float(rec[4]), crowded);
    }
    __syncthreads();
    // one reciprocal per record; empty-rho cells give 0 (the NaN->0 rule of interp.py:329-331)
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (rloc[k] != 0xffffffffu) {
        const float r = acc[rloc[k]];
        rrec[k] = pencil_rho_factor<WEIGHTED>(r, p.wexp);
      }
    for (unsigned j = tail0; j < e; j += NT) {
      const float r = acc[p.records[(size_t)j * 5]];
      p.side[j] = pencil_rho_factor<WEIGHTED>(r, p.wexp);
    }
  }

  // ENERGY: the three rho*v_c rounds add up q_c^2 per record, a FOURTH round accumulates rho and finishes
  // E = vol * sum / rho in the cells that hold records (all others stay 0)
  const bool we = !ENERGY && p.with_energy;     // (uniform) momentum launch that also produces the energy field
  const int nround = DENSITY ? 1 : ((ENERGY || we) ? p.ncomp + 1 : p.ncomp);
  for (int c = 0; c < nround; ++c) {
    // opaque copies: keeps the compiler from hoisting ~50 loop-invariant LDS addresses out of the
    // component loop (they cost more registers than they save instructions, and an occupancy step)
    int lc = l, tc = t, tidc = tid;
    asm volatile("" : "+v"(lc), "+v"(tc), "+v"(tidc));
    lc &= L - 1;   // give the value ranges back to the compiler (address folding needs them)
    tc &= TP - 1;
    tidc &= NT - 1;
    __syncthreads();   // rho / previous component's transposed image fully consumed
    // The accumulator still holds the previous round's totals -- rho ahead of the first velocity component, a component ahead
    // of the next one (ENERGY) -- and is zero in every cell without a record: the records clear their own cells (a few hundred
    // 4-byte writes) instead of a dense fill of the whole region (64 - 128 KB at the LDS write rate: 830 - 1500 clk per round).
    // After a transform the region is FFT scratch and needs the dense fill.
    const bool sparse_clear = ENERGY ? (c > 0) : (divide && c == 0);
    if (sparse_clear) {
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (rloc[k] != 0xffffffffu) acc[rloc[k]] = 0.f;
      for (unsigned j = tail0; j < e; j += NT) acc[p.records[(size_t)j * 5]] = 0.f;
    } else {
      for (int i = tid; i < ACC / 4; i += NT) reinterpret_cast<float4*>(acc)[i] = zero4;
    }
    __syncthreads();
    const bool rho_round = (ENERGY || we) && c == p.ncomp;
    const int word = (DENSITY || rho_round) ? 4 : 1 + p.chan[c < p.ncomp ? c : 0];
    // velocity: each term is divided by its cell's rho as it is added -- sum_k (q_k / rho) for the reference's
    // (sum_k q_k) / rho: a different rounding of the same value, within the float32 accumulation noise of the sums
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (rloc[k] != 0xffffffffu) vps_lds_add(&acc[rloc[k]], divide ? rval[k] * rrec[k] : rval[k], crowded);
    if (c + 1 < nround) fetch(((ENERGY || we) && c + 1 == p.ncomp) ? 4 : 1 + p.chan[c + 1 < p.ncomp ? c + 1 : 0]);
    for (unsigned j = tail0; j < e; j += NT) {
      const unsigned* rec = p.records + (size_t)j * 5;
      const float val = __uint_as_float(rec[word]);
      vps_lds_add(&acc[rec[0]], divide ? val * p.side[j] : val, crowded);
    }
    __syncthreads();
    if (ENERGY || we) {
      if (!rho_round) {
        // the cell totals of this component, squared, per record
#pragma unroll
        for (int k = 0; k < KR; ++k)
          if (rloc[k] != 0xffffffffu) {
            const float q = acc[rloc[k]];
            rrec[k] = (c == 0) ? q * q : rrec[k] + q * q;
          }
        for (unsigned j = tail0; j < e; j += NT) {
          const float q = acc[p.records[(size_t)j * 5]];
          p.side[j] = (c == 0) ? q * q : p.side[j] + q * q;
        }
        if constexpr (ENERGY) continue;   // (the barrier at the top of the loop protects the accumulator)
        // (with_energy: the accumulator goes on into this component's own transform)
      } else {
        // the accumulator holds rho: E = sum * (1 / rho) * vol where there is mass, 0 elsewhere -- every record writes its cell's
        // value (records of one cell write the same bits), after everybody has read rho
#pragma unroll
        for (int k = 0; k < KR; ++k)
          if (rloc[k] != 0xffffffffu) {
            const float r = acc[rloc[k]];
            rrec[k] = r != 0.f ? rrec[k] * __builtin_amdgcn_rcpf(r) * p.vol : 0.f;
          }
        for (unsigned j = tail0; j < e; j += NT) {
          const float r = acc[p.records[(size_t)j * 5]];
          p.side[j] = r != 0.f ? p.side[j] * __builtin_amdgcn_rcpf(r) * p.vol : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KR; ++k)
          if (rloc[k] != 0xffffffffu) acc[rloc[k]] = rrec[k];
        for (unsigned j = tail0; j < e; j += NT) acc[p.records[(size_t)j * 5]] = p.side[j];
        __syncthreads();
      }
    }
    if constexpr (DENSITY) {
      // the accumulator holds rho.  The plain density is done; else every record forms s(rho) of its cell, and once everybody
      // has read rho writes it back (records of one cell write the same bits; cells without a record stay 0) -- the way the
      // energy launch finishes its rho round
      if (p.scalar != PENCIL_SCALAR_RHO) {
#pragma unroll
        for (int k = 0; k < KR; ++k)
          if (rloc[k] != 0xffffffffu) rrec[k] = pencil_rho_scalar(acc[rloc[k]], p.scalar, p.sexp);
        for (unsigned j = tail0; j < e; j += NT) p.side[j] = pencil_rho_scalar(acc[p.records[(size_t)j * 5]], p.scalar, p.sexp);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KR; ++k)
          if (rloc[k] != 0xffffffffu) acc[rloc[k]] = rrec[k];
        for (unsigned j = tail0; j < e; j += NT) acc[p.records[(size_t)j * 5]] = p.side[j];
        __syncthreads();
      }
    }
    // stage-0 inputs straight from the accumulator: z[j] = f[2j] + i f[2j+1]
    cf v[RL];
    {
      const float* q = acc + tc * N;
      const float sc = (ENERGY || DENSITY || divide || rho_round) ? 1.f : p.vol;
#pragma unroll
      for (int m = 0; m < NB0; ++m)
#pragma unroll
        for (int rr = 0; rr < R0; ++rr) {
          const int j = lc + L * m + rr * (NC / R0);
          const float2 qq = *reinterpret_cast<const float2*>(q + 2 * j);
          v[m * R0 + rr] = make_float2(qq.x * sc, qq.y * sc);
        }
    }
    __syncthreads();   // accumulator of this component consumed: its memory becomes FFT scratch
    constexpr bool WSYNC = (L <= 64) && (64 % L == 0);
    fft_from_regs_l<NC, L, WSYNC>(v, buf + tc * PI::PITCH, tw, lc);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RL; ++i) buf[tridx<TP>(out_index_l<NC, L>(lc, i), tc)] = v[i];
    __syncthreads();
    const int oc = (ENERGY || DENSITY) ? 0 : c;
    cf* out = p.out[oc] + (long long)x * NC * N + y0;
    cf* nyq = p.nyq[oc] + (long long)x * N + y0;
    // 8-line pencils (64-byte output segments) leave in 16-byte stores: the epilogue is bound by store ISSUE (half the
    // instructions with dwordx4).  Plain stores for the energy launch and for the energy field of a with_energy launch -- a
    // workgroup's LAST field: its half lines merge in L2 with the partner pencil's when they are not marked streaming (PMC: 44.9 ->
    // 35.1 GB written for 34.4 GB of output); streaming stores otherwise.  Measured at C4: DESIGN.md section 7.
    constexpr bool ST16 = TP == 8 && (NC & 1) == 0 && ((NC / 2) * (TP / 2)) % NT == 0;
    if constexpr (ST16) {
      if (ENERGY || DENSITY || rho_round)
        r2c_store_tile16<NC, TP, NT, true>(buf, tidc, p.tw_r2c, out, N, nyq);
      else
        r2c_store_tile16<NC, TP, NT, false>(buf, tidc, p.tw_r2c, out, N, nyq);
    } else
      r2c_store_tile<NC, TP, NT, false, (ENERGY || DENSITY) && TP < 16>(buf, tidc, p.tw_r2c, out, N, nyq, TP);
  }
}

// ------------------------------------------------------------------------------
// Epilogue of the kernel that transforms a pencil of TP lines in two halves of TP/2 lines (split pencil): thread
// (t, l) holds the spectrum of line t in `vpark` and of line t + TP/2 in `v`.  The transposed image of all TP lines does not
// fit next to nothing else: it is staged in two halves of the mode PAIRS -- the real-to-complex step needs Z[k] with Z[NC - k]:
// after the last radix-R stage register slot (m, r) holds k = l + L m + r NC/R, so r < R/4 and r >= 3R/4 are exactly the modes
// k < NC/4 and k >= 3 NC/4 (the pairs of the first half), the middle slots the second.  Z[3 NC/4] pairs with Z[NC/4] of the
// OTHER half image: the first phase leaves it in `edge` (TP values).  Row kk of a half image: k < NC/4 -> kk = k;
// k >= 3NC/4 -> kk = k - NC/2 (first half); NC/4 <= k < 3NC/4 -> kk = k - NC/4 (second half).  16-byte stores: two lines per lane.
// ------------------------------------------------------------------------------
template <int NC, int TP, int L, bool STREAM>
__device__ __forceinline__ void two_half_image_store(cf* buf, cf* edge, const cf (&vpark)[NC / L], const cf (&v)[NC / L], int l, int t,
                                                     int tid, cf* out, cf* nyq, const cf* __restrict__ tw_r2c) {
  constexpr int RL = NC / L, TH = TP / 2, NT = TH * L, N = 2 * NC;
  constexpr int R = LastRadix<NC>::R;
  static_assert((R % 4) == 0 && (NC % 4) == 0, "image in two halves of the mode pairs");
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    int lc = l, tc = t, tidc = tid;
    asm volatile("" : "+v"(lc), "+v"(tc), "+v"(tidc));
    lc &= L - 1;
    tc &= TH - 1;
    tidc &= NT - 1;
    __syncthreads();   // exchange buffers / the previous half image are free
#pragma unroll
    for (int i = 0; i < RL; ++i) {
      const int r = i % R;
      const bool outer = (r < R / 4) || (r >= 3 * R / 4);
      if (outer == (g == 0)) {
        const int k = out_index_l<NC, L>(lc, i);
        const int kk = (g == 0) ? ((r < R / 4) ? k : k - NC / 2) : k - NC / 4;
        buf[tridx<TP>(kk, tc)] = vpark[i];
        buf[tridx<TP>(kk, tc + TH)] = v[i];
        if (g == 0 && i == 3 * R / 4 && lc == 0) {   // slot (m = 0, r = 3R/4) of lane 0: mode 3 NC/4
          edge[tc] = vpark[i];
          edge[tc + TH] = v[i];
        }
      }
    }
    __syncthreads();
    // pairs of this half: k = 0 .. NC/4 - 1 with NC - k (g = 0; k = 0: the self-paired modes 0 and NC/2 -- NC/2 sits in
    // the OTHER half image, so g = 0 writes X[0] and the Nyquist plane, g = 1 writes X[NC/2] from its own row);
    // k = NC/4 .. NC/2 - 1 with NC - k, and the self-paired NC/2 (g = 1)
    constexpr int H2 = TP / 2, ITEMS = (NC / 4) * H2;
    static_assert(ITEMS % NT == 0, "whole rounds");
#pragma unroll 4
    for (int i = 0; i < ITEMS / NT; ++i) {
      const int idx = tidc + i * NT;
      const int tt = (idx % H2) * 2, kq = idx / H2;           // kq = 0 .. NC/4 - 1
      const int k = (g == 0) ? kq : kq + NC / 4;              // the smaller mode of the pair
      const int rowk = (g == 0) ? k : k - NC / 4;             // its row in this half image
      const int rown = (g == 0) ? (NC - k) - NC / 2 : (NC - k) - NC / 4;   // row of NC - k (k > 0)
      const cf a0 = buf[tridx<TP>(rowk, tt)], a1 = buf[tridx<TP>(rowk, tt + 1)];
      if (g == 0 && k == 0) {
        *reinterpret_cast<vps_f4*>(&out[tt]) = vps_f4{a0.x + a0.y, 0.f, a1.x + a1.y, 0.f};
        *reinterpret_cast<vps_f4*>(&nyq[tt]) = vps_f4{a0.x - a0.y, 0.f, a1.x - a1.y, 0.f};
      } else {
        if (g == 1 && k == NC / 4) {
          // (row NC/2 - NC/4 of this half image holds mode NC/2, which pairs with itself)
          const cf h0 = buf[tridx<TP>(NC / 2 - NC / 4, tt)], h1 = buf[tridx<TP>(NC / 2 - NC / 4, tt + 1)];
          *reinterpret_cast<vps_f4*>(&out[(long long)(NC / 2) * N + tt]) = vps_f4{h0.x, -h0.y, h1.x, -h1.y};
        }
        const bool at_edge = (g == 1 && k == NC / 4);      // partner 3 NC/4 was left in `edge` by the first phase
        const cf n0 = at_edge ? edge[tt] : buf[tridx<TP>(rown, tt)], n1 = at_edge ? edge[tt + 1] : buf[tridx<TP>(rown, tt + 1)];
        const cf w = tw_r2c[k];
        const cf s0 = make_float2(a0.x + n0.x, a0.y - n0.y), d0 = make_float2(a0.x - n0.x, a0.y + n0.y);
        const cf s1 = make_float2(a1.x + n1.x, a1.y - n1.y), d1 = make_float2(a1.x - n1.x, a1.y + n1.y);
        const cf w0 = cmul(w, d0), w1 = cmul(w, d1);
        const vps_f4 lo = {0.5f * (s0.x + w0.y), 0.5f * (s0.y - w0.x), 0.5f * (s1.x + w1.y), 0.5f * (s1.y - w1.x)};
        const vps_f4 hi = {0.5f * (s0.x - w0.y), 0.5f * (-s0.y - w0.x), 0.5f * (s1.x - w1.y), 0.5f * (-s1.y - w1.x)};
        if constexpr (!STREAM) {
          *reinterpret_cast<vps_f4*>(&out[(long long)k * N + tt]) = lo;
          *reinterpret_cast<vps_f4*>(&out[(long long)(NC - k) * N + tt]) = hi;
        } else {
          __builtin_nontemporal_store(lo, reinterpret_cast<vps_f4*>(&out[(long long)k * N + tt]));
          __builtin_nontemporal_store(hi, reinterpret_cast<vps_f4*>(&out[(long long)(NC - k) * N + tt]));
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------
// Split pencil: the same pencil (TP = 8 y-lines) on HALF the threads -- a workgroup runs the deposit rounds and the transform of
// lines 0..3, parks their spectrum in registers (RL values per lane), does the same for lines 4..7, and only then stages the
// transposed image of all eight lines and stores it.  The LDS region is that of FOUR lines: at 4096-cell lines 67.6 KB instead
// of 135 KB (+ 16 KB of twiddles, now read through L2 as the 4096-point y pass does), so TWO workgroups of 512 threads share a
// CU where one of 1024 ran alone with every phase exposed (pencil kernel at 0.26 of peak at N = 4096).
// The image of eight lines no longer fits either: it is staged in two halves of the mode PAIRS -- the real-to-complex step needs
// Z[k] with Z[NC - k]: after the last radix-R stage register slot (m, r) holds k = l + L m + r NC/R, so r < R/4 and
// r >= 3R/4 are exactly the modes k < NC/4 and k >= 3 NC/4 (the pairs of the first half), the middle slots the second.
// Every record is looked at once per half (a record belongs to the half that holds its line); everything else -- per-record
// 1/rho and energy sums, sparse clears, CAS-first LDS adds, the 16-byte epilogue -- is the pencil kernel's.
// ------------------------------------------------------------------------------
template <int NC, int TP, bool ENERGY>
__global__ void __launch_bounds__((TP / 2) * PlanInfo<NC>::L, 4) pencil_split_fft_z_kernel(const PencilParams p) {
  typedef PlanInfo<NC> PI;
  constexpr int L = PI::L, RL = PI::RL, TH = TP / 2, NT = TH * L, N = 2 * NC;
  constexpr int R = LastRadix<NC>::R;
  static_assert(TP == 8 && (R % 4) == 0 && (NC % 4) == 0, "eight lines in two halves, image in two halves of the mode pairs");
  constexpr int ACC = TH * N;                       // floats of one accumulator (four lines)
  constexpr int LINES = TH * PI::PITCH * 2;         // floats of the exchange buffers
  constexpr int IMG = (NC / 2) * TP * 2;            // floats of half an image: NC/2 modes x 8 lines
  constexpr int SHARED = (ACC > LINES ? (ACC > IMG ? ACC : IMG) : (LINES > IMG ? LINES : IMG));
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* acc = reinterpret_cast<float*>(smem_raw);
  cf* buf = reinterpret_cast<cf*>(acc);
  // Z[3 NC/4] of the eight lines: its partner Z[NC/4] sits in the OTHER half image (slot r = R/4 against r = 3R/4), so the first
  // image phase leaves it here for the second
  cf* edge = reinterpret_cast<cf*>(acc + SHARED);
  const cf* tw = p.tw_stage;                        // (through L2: the region is the whole of the workgroup's LDS)

  const int tid = threadIdx.x;
  const int t = tid / L, l = tid % L;
  unsigned pencil = blockIdx.x;
  {   // the two pencils that complete a 128-byte output line on ONE XCD, close in time (as in pencil_fft_z_kernel)
    constexpr unsigned GP = 16 / TP, span = 8 * GP;
    if (pencil / span < p.npencils / span) {
      const unsigned base = (pencil / span) * span, h = pencil % span;
      pencil = base + GP * (h % 8) + (h / 8);
    }
  }
  const int x = pencil / p.nby, y0 = (pencil % p.nby) * TP;
  const unsigned s = p.start[pencil], e = p.start[pencil + 1];
  const bool crowded = (e - s) > 4u * (unsigned)ACC;
  constexpr int KR = 2;      // register-resident record groups: 2 x 256 / 2 x 512 threads hold a typical bucket of EIGHT lines
  constexpr int NW_ = ENERGY ? 4 : 3;
  unsigned rloc[KR];         // cell inside the pencil: line * N + z
  float rw[KR][NW_];         // the record's values [rho v_x, rho v_y, rho v_z (, rho)]: every round of both halves reads them here
  float rrec[KR];
#pragma unroll
  for (int k = 0; k < KR; ++k) {
    const unsigned j = s + tid + k * NT;
    rloc[k] = 0xffffffffu;
    rrec[k] = 1.f;
    if (j < e) {
      const unsigned* rec = p.records + (size_t)j * 5;
      rloc[k] = rec[0];
#pragma unroll
      for (int w_ = 0; w_ < NW_; ++w_) rw[k][w_] = __uint_as_float(rec[1 + w_]);
    }
  }
  const bool divide = !ENERGY && p.divide;
  const unsigned tail0 = s + tid + KR * NT;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int R0 = PI::R0, NB0 = RL / R0;
  constexpr bool WSYNC = (L <= 64) && (64 % L == 0);
  // cell of a record inside the half that is being worked on, or 0xffffffff: not this half's
  auto local = [&](unsigned cell, int h) -> unsigned {
    const unsigned lo = (unsigned)h * (unsigned)ACC;
    return (cell - lo) < (unsigned)ACC ? cell - lo : 0xffffffffu;     // (0xffffffff - lo wraps far beyond ACC)
  };
  auto dense_clear = [&]() {
    for (int i = tid; i < ACC / 4; i += NT) reinterpret_cast<float4*>(acc)[i] = zero4;
  };
  // one accumulation round of half h: adds `word` of every record of the half (times its 1/rho when dividing)
  auto scatter = [&](int h, int word, bool times_rrec) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const unsigned c_ = local(rloc[k], h);
      if (c_ != 0xffffffffu) {
        float v_;
        if constexpr (ENERGY) {
          v_ = word == 1 ? rw[k][0] : (word == 2 ? rw[k][1] : (word == 3 ? rw[k][2] : rw[k][NW_ - 1]));
        } else {   // (vector launches keep three words; rho -- the dividing launches' first rounds -- is read where it is used)
          v_ = word == 1 ? rw[k][0] : (word == 2 ? rw[k][1] : (word == 3 ? rw[k][2]
                                                                          : __uint_as_float(p.records[(size_t)(s + tid + k * NT) * 5 + 4])));
        }
        vps_lds_add(&acc[c_], times_rrec ? v_ * rrec[k] : v_, crowded);
      }
    }
    for (unsigned j = tail0; j < e; j += NT) {
      const unsigned* rec = p.records + (size_t)j * 5;
      const unsigned c_ = local(rec[0], h);
      if (c_ != 0xffffffffu) {
        const float v_ = __uint_as_float(rec[word]);
        vps_lds_add(&acc[c_], times_rrec ? v_ * p.side[j] : v_, crowded);
      }
    }
  };
  auto sparse_clear = [&](int h) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const unsigned c_ = local(rloc[k], h);
      if (c_ != 0xffffffffu) acc[c_] = 0.f;
    }
    for (unsigned j = tail0; j < e; j += NT) {
      const unsigned c_ = local(p.records[(size_t)j * 5], h);
      if (c_ != 0xffffffffu) acc[c_] = 0.f;
    }
  };

  // ---- velocity: 1 / rho of every record's cell, half by half ----
  if (divide) {
    for (int h = 0; h < 2; ++h) {
      __syncthreads();
      dense_clear();
      __syncthreads();
      scatter(h, 4, false);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        const unsigned c_ = local(rloc[k], h);
        if (c_ != 0xffffffffu) {
          const float r = acc[c_];
          rrec[k] = r != 0.f ? __builtin_amdgcn_rcpf(r) : 0.f;
        }
      }
      for (unsigned j = tail0; j < e; j += NT) {
        const unsigned c_ = local(p.records[(size_t)j * 5], h);
        if (c_ != 0xffffffffu) {
          const float r = acc[c_];
          p.side[j] = r != 0.f ? __builtin_amdgcn_rcpf(r) : 0.f;
        }
      }
    }
  }
  // ---- ENERGY: per record the sum over components of (cell total of rho v_c)^2, half by half and component by component ----
  if constexpr (ENERGY) {
    for (int h = 0; h < 2; ++h)
      for (int c = 0; c < p.ncomp; ++c) {
        __syncthreads();
        if (c == 0) dense_clear(); else sparse_clear(h);
        __syncthreads();
        scatter(h, 1 + p.chan[c], false);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const unsigned c_ = local(rloc[k], h);
          if (c_ != 0xffffffffu) {
            const float q = acc[c_];
            rrec[k] = (c == 0) ? q * q : rrec[k] + q * q;
          }
        }
        for (unsigned j = tail0; j < e; j += NT) {
          const unsigned c_ = local(p.records[(size_t)j * 5], h);
          if (c_ != 0xffffffffu) {
            const float q = acc[c_];
            p.side[j] = (c == 0) ? q * q : p.side[j] + q * q;
          }
        }
      }
  }

  // ---- per output field: both halves accumulated and transformed, then the image of all eight lines in two halves ----
  const int nfields = ENERGY ? 1 : p.ncomp;
  for (int c = 0; c < nfields; ++c) {
    cf vpark[RL], v[RL];
    for (int h = 0; h < 2; ++h) {
      int lc = l, tc = t;
      asm volatile("" : "+v"(lc), "+v"(tc));   // (keeps the LDS addresses of the two halves from being formed up front)
      lc &= L - 1;
      tc &= TH - 1;
      __syncthreads();   // previous image / previous half's exchange buffers consumed
      dense_clear();
      __syncthreads();
      if constexpr (ENERGY) {
        scatter(h, 4, false);              // rho
        __syncthreads();
        // E = vol * sum / rho where there is mass: every record writes its cell's value once all have read rho
        float ev[KR];
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const unsigned c_ = local(rloc[k], h);
          ev[k] = 0.f;
          if (c_ != 0xffffffffu) {
            const float r = acc[c_];
            ev[k] = r != 0.f ? rrec[k] * __builtin_amdgcn_rcpf(r) * p.vol : 0.f;
          }
        }
        for (unsigned j = tail0; j < e; j += NT) {
          const unsigned c_ = local(p.records[(size_t)j * 5], h);
          if (c_ != 0xffffffffu) {
            const float r = acc[c_];
            p.side[j] = r != 0.f ? p.side[j] * __builtin_amdgcn_rcpf(r) * p.vol : 0.f;
          }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const unsigned c_ = local(rloc[k], h);
          if (c_ != 0xffffffffu) acc[c_] = ev[k];
        }
        for (unsigned j = tail0; j < e; j += NT) {
          const unsigned c_ = local(p.records[(size_t)j * 5], h);
          if (c_ != 0xffffffffu) acc[c_] = p.side[j];
        }
      } else {
        scatter(h, 1 + p.chan[c], divide);
      }
      __syncthreads();
      {
        const float* q = acc + tc * N;
        const float sc = (ENERGY || divide) ? 1.f : p.vol;
#pragma unroll
        for (int m = 0; m < NB0; ++m)
#pragma unroll
          for (int rr = 0; rr < R0; ++rr) {
            const int j = lc + L * m + rr * (NC / R0);
            const float2 qq = *reinterpret_cast<const float2*>(q + 2 * j);
            v[m * R0 + rr] = make_float2(qq.x * sc, qq.y * sc);
          }
      }
      __syncthreads();   // accumulator consumed: its memory becomes FFT scratch
      fft_from_regs_l<NC, L, WSYNC>(v, buf + tc * PI::PITCH, tw, lc);
      if (h == 0) {
#pragma unroll
        for (int i = 0; i < RL; ++i) vpark[i] = v[i];
      }
    }
    // ---- image halves: pairs (k, NC - k) with min(k, NC - k) < NC/4 first, the rest second ----
    cf* out = p.out[c] + (long long)x * NC * N + y0;
    cf* nyq = p.nyq[c] + (long long)x * N + y0;
    two_half_image_store<NC, TP, L, !ENERGY>(buf, edge, vpark, v, l, t, tid, out, nyq, p.tw_r2c);
  }
}

// (A wave-private form -- every wave scans all records of the pencil, keeps those of its own line(s) and runs zero-fill, LDS
// adds, read-back, stage-0 loads and the exchanges inside its own LDS region with wave-level ordering only, three workgroup
// barriers per component instead of seven -- measured at C4: 97 against 75 ms per step of pencil launches, bit-identical
// results.  The barriers are not what the kernel waits for; eight-fold record scans and 64-lane zero-fills cost more.)

template <int NC>
size_t pencil_lds_bytes() {
  typedef PlanInfo<NC> PI;
  constexpr int PENCIL_TP = pencil_tp<NC>();
  constexpr int ACC = PENCIL_TP * 2 * NC, LINES = PENCIL_TP * PI::PITCH * 2;
  return (size_t)(ACC > LINES ? ACC : LINES) * sizeof(float) + (size_t)PI::TWL * sizeof(cf);
}

template <int NC>
size_t pencil_split_lds_bytes() {
  typedef PlanInfo<NC> PI;
  constexpr int TH = pencil_tp<NC>() / 2;
  constexpr size_t ACC = (size_t)TH * 2 * NC, LINES = (size_t)TH * PI::PITCH * 2, IMG = (size_t)(NC / 2) * pencil_tp<NC>() * 2;
  const size_t shared = ACC > LINES ? (ACC > IMG ? ACC : IMG) : (LINES > IMG ? LINES : IMG);
  return shared * sizeof(float) + (size_t)pencil_tp<NC>() * sizeof(cf);
}

template <int NC>
int launch_pencil(vps_ctx* ctx, const PencilParams& p, long long npencils) {
  typedef PlanInfo<NC> PI;
  // 2048 packed points (4096-cell lines, where a whole pencil leaves one workgroup per CU), energy launch: the split kernel.
  // (Its vector form does not fit 128 VGPRs: whole pencils there, as for every other length.)
  if constexpr (NC == 2048) if (p.energy) {
    const size_t lds2 = pencil_split_lds_bytes<NC>();
    constexpr int TP2 = pencil_tp<NC>();
    auto kern2 = pencil_split_fft_z_kernel<NC, TP2, true>;
    if (lds2 > 64 * 1024)
      VPS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern2),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    PencilParams pp2 = p;
    pp2.npencils = (unsigned)npencils;
    {
      vps_launch_timer tm(ctx, VPS_K_FFT_Z);
      hipLaunchKernelGGL(kern2, dim3((unsigned)npencils), dim3((TP2 / 2) * PI::L), lds2, ctx->stream, pp2);
    }
    VPS_HIP_CHECK(ctx, hipGetLastError());
    return VPS_OK;
  }
  const size_t lds = pencil_lds_bytes<NC>();
  constexpr int PENCIL_TP = pencil_tp<NC>();
  if (lds > ctx->lds_per_cu) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "pencil kernel needs %zu B LDS", lds);
  auto kern = p.energy ? pencil_fft_z_kernel<NC, PENCIL_TP, true>
                       : (p.weighted ? pencil_fft_z_kernel<NC, PENCIL_TP, false, true>
                                     : (p.scalar ? pencil_fft_z_kernel<NC, PENCIL_TP, false, false, true>
                                                 : pencil_fft_z_kernel<NC, PENCIL_TP, false>));
  if (lds > 64 * 1024)
    VPS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  PencilParams pp = p;
  pp.npencils = (unsigned)npencils;
  {
    vps_launch_timer tm(ctx, VPS_K_FFT_Z);
    hipLaunchKernelGGL(kern, dim3((unsigned)npencils), dim3(PENCIL_TP * PI::L), lds, ctx->stream, pp);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

}  // namespace
