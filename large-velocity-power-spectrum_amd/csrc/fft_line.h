// One line of NC complex points: its plan (lanes, radices), the Stockham stages with their LDS exchanges and twiddles, the
// stores shared by the passes, and the constexpr rules that launchers and host API derive from a line length.
// The host API (fft.hip) includes this for those rules only; it instantiates nothing that runs on the device.
#pragma once
#include "fft_dft.h"

namespace {

// ---- per-length plans: L lanes per line, radices R0*R1*R2 = NC -----------------
template <int NC>
struct Plan;
#define VPS_PLAN(NC_, L_, A_, B_, C_)                          \
  template <>                                                  \
  struct Plan<NC_> {                                           \
    static constexpr int L = L_, R0 = A_, R1 = B_, R2 = C_;    \
  };
VPS_PLAN(8, 1, 8, 1, 1)
VPS_PLAN(16, 1, 16, 1, 1)
VPS_PLAN(32, 4, 8, 4, 1)
VPS_PLAN(64, 8, 8, 8, 1)
VPS_PLAN(128, 8, 16, 8, 1)
VPS_PLAN(256, 16, 16, 16, 1)
VPS_PLAN(512, 32, 8, 8, 8)
VPS_PLAN(1024, 64, 16, 8, 8)
VPS_PLAN(2048, 128, 16, 16, 8)
VPS_PLAN(4096, 256, 16, 16, 16)
// 2^a 5^b lengths: N = 250, 500, 1000 (lines of N/2 packed-real and N complex points)
// 3 * 2^a lengths: N = 96, 192, 384, 768
VPS_PLAN(48, 2, 8, 6, 1)
VPS_PLAN(96, 4, 8, 12, 1)
VPS_PLAN(192, 8, 8, 8, 3)
VPS_PLAN(384, 16, 8, 8, 6)
VPS_PLAN(768, 32, 8, 8, 12)
VPS_PLAN(1536, 64, 8, 8, 24)
VPS_PLAN(125, 25, 5, 5, 5)
VPS_PLAN(250, 25, 10, 5, 5)
VPS_PLAN(500, 25, 10, 10, 5)
VPS_PLAN(1000, 50, 10, 10, 10)
VPS_PLAN(2000, 100, 10, 10, 20)

template <int NC>
struct PlanInfo {
  typedef Plan<NC> P;
  static constexpr int L = P::L;
  static constexpr int RL = NC / L;
  static constexpr int R0 = P::R0, R1 = P::R1, R2 = P::R2;
  static constexpr int NS1 = R0, NS2 = R0 * R1;
  static constexpr int TW1 = (R1 > 1) ? (R1 - 1) * NS1 : 0;
  static constexpr int TW2 = (R2 > 1) ? (R2 - 1) * NS2 : 0;
  static constexpr int TW = TW1 + TW2;  // entries of the per-stage twiddle image
  // the image is staged in LDS except for the longest lines, where the tile itself needs
  // nearly all of the 160 KiB (the table then stays in L2)
  static constexpr bool TWLDS = NC <= 2048;
  static constexpr int TWL = TWLDS ? ((TW + 1) & ~1) : 0;  // LDS entries reserved for it
  // LDS line pitch (complex elements): one pad slot per 32 elements
  static constexpr int PITCH = NC + (NC >> 5) + 1;
  static_assert(R0 * R1 * R2 == NC, "bad plan");
  static_assert(RL % R0 == 0 && RL % R1 == 0 && RL % R2 == 0, "radix must divide RL");
};

// Position of element p inside a line's LDS exchange buffer: one pad slot per 32 elements.
// (Measured alternative: the XOR swizzle p ^ ((p >> A) & 15) makes every exchange access of the
// 512..4096-point plans bank-conflict free on paper, but its per-access address arithmetic
// costs ~30 VGPRs, drops the x pass from 3 to 2 waves/SIMD and ran 20-60 % slower at
// N = 1024/2048, with no measurable gain in the z/y passes: the exchanges are not the limiter.)
template <int NC>
__device__ __forceinline__ int padidx(int p) {
  return p + (p >> 5);
}

// Transposed tile image [k][t] with pitch T and an XOR swizzle of t, so that both the
// column-wise writes (16 consecutive k, one t) and the row-wise reads (one k, all t)
// of ds_write_b64 / ds_read_b64 touch distinct LDS slots.
template <int T>
__device__ __forceinline__ int tridx(int k, int t) {
  constexpr int SH = (T >= 16) ? 0 : ((T == 8) ? 1 : ((T == 4) ? 2 : ((T == 2) ? 3 : 4)));
  return k * T + (t ^ ((k >> SH) & (T - 1)));
}

// Stage s input for lane l: v[m*R + r] = src(l + L*m + r*NC/R)
template <int NC, int L, int RL, int R>
__device__ __forceinline__ void lds_load_stage(cf (&v)[RL], const cf* line, int l) {
  constexpr int NB = RL / R;
  // Where every stride is a multiple of the 32 elements between pad slots, padidx(l + c) = padidx(l) + c + c / 32 exactly: ONE
  // lane-dependent address and immediate offsets.  (Left to the compiler each of the RL addresses cost four VALU operations --
  // or, shift, and, add3 -- a fifth of the instructions of a 2048-point transform.)
  if constexpr ((L % 32 == 0) && ((NC / R) % 32 == 0)) {
    const cf* base = line + padidx<NC>(l);
#pragma unroll
    for (int m = 0; m < NB; ++m) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int c = L * m + r * (NC / R);
        v[m * R + r] = base[c + (c >> 5)];
      }
    }
  } else {
#pragma unroll
    for (int m = 0; m < NB; ++m) {
#pragma unroll
      for (int r = 0; r < R; ++r) v[m * R + r] = line[padidx<NC>(l + L * m + r * (NC / R))];
    }
  }
}

template <int NC, int L, int RL, int R, int NS>
__device__ __forceinline__ void twiddle_butterfly(cf (&v)[RL], const cf* tw, int l) {
  constexpr int NB = RL / R;
#pragma unroll
  for (int m = 0; m < NB; ++m) {
    if constexpr (NS > 1) {
      const int k = (l + L * m) % NS;   // (NS is a compile-time constant: a mask for powers of two)
#pragma unroll
      for (int r = 1; r < R; ++r) v[m * R + r] = cmul(v[m * R + r], tw[(r - 1) * NS + k]);
    }
    Dft<R>::run(&v[m * R]);
  }
}

// The same with the stage's twiddles in registers, loaded once per kernel (load_stage_twiddles): they depend on the lane alone.
// twr[r - 1] = tw[(r - 1) * NS + l] is the twiddle of the lane's FIRST butterfly (m = 0); for m > 0 the index moves by L m and
// the twiddle by the constant factor exp(-2 pi i r L m / (NS R)) -- a 16th root of unity for the last stage of the 2048-point
// plan (L = 128, NS = 256, R = 8), applied to the value first (rot16: two packed operations, none for r = 4).  Seven values in
// 14 VGPRs instead of 14 KB of LDS that the x pass no longer needs.
template <int Q>   // v * exp(-2 pi i Q / 16)
__device__ __forceinline__ cf rot16(cf v) {
  constexpr int q = ((Q % 16) + 16) % 16;
  if constexpr (q == 0) return v;
  else if constexpr (q == 4) return cmul_mi(v);
  else if constexpr (q == 8) return make_float2(-v.x, -v.y);
  else if constexpr (q == 12) return make_float2(-v.y, v.x);
  else if constexpr (q == 2) return make_float2((v.x + v.y) * VPS_SQRT1_2, (v.y - v.x) * VPS_SQRT1_2);
  else if constexpr (q == 6) return make_float2((v.y - v.x) * VPS_SQRT1_2, -(v.x + v.y) * VPS_SQRT1_2);
  else if constexpr (q == 10) return make_float2(-(v.x + v.y) * VPS_SQRT1_2, (v.x - v.y) * VPS_SQRT1_2);
  else if constexpr (q == 14) return make_float2((v.x - v.y) * VPS_SQRT1_2, (v.x + v.y) * VPS_SQRT1_2);
  else {
    // odd q: cos / sin of q pi / 8 from the pi / 8 pair
    constexpr float c = (q == 1 || q == 15) ? VPS_COS_PI_8 : (q == 3 || q == 13) ? VPS_SIN_PI_8 : (q == 5 || q == 11) ? -VPS_SIN_PI_8 : -VPS_COS_PI_8;
    constexpr float sn = (q == 1 || q == 7) ? VPS_SIN_PI_8 : (q == 3 || q == 5) ? VPS_COS_PI_8 : (q == 9 || q == 15) ? -VPS_SIN_PI_8 : -VPS_COS_PI_8;
    return cmul(v, make_float2(c, -sn));   // exp(-i q pi / 8) = cos - i sin
  }
}
template <int NC, int L, int RL, int R, int NS>
struct RegTwiddles {
  static constexpr int NB = RL / R;
  // SAME: L is a multiple of NS, every butterfly of a lane has the same twiddle index l % NS.  Otherwise the index moves by L
  // per butterfly without wrapping, and the angle by STEP16 sixteenths of a turn per unit of r.
  static constexpr bool SAME = (L % NS == 0);
  static constexpr bool OK = SAME || ((L * (NB - 1) < NS) && ((16 * L) % (NS * R) == 0));
  static constexpr int STEP16 = (OK && !SAME) ? (16 * L) / (NS * R) : 0;
};
template <int NC, int L, int RL, int R, int NS, int M, int RR>
__device__ __forceinline__ void twiddle_reg_apply(cf (&v)[RL], const cf* twr) {
  if constexpr (RR < R) {
    v[M * R + RR] = cmul(rot16<RegTwiddles<NC, L, RL, R, NS>::STEP16 * M * RR>(v[M * R + RR]), twr[RR - 1]);
    twiddle_reg_apply<NC, L, RL, R, NS, M, RR + 1>(v, twr);
  }
}
template <int NC, int L, int RL, int R, int NS, int M = 0>
__device__ __forceinline__ void twiddle_butterfly_reg(cf (&v)[RL], const cf* twr) {
  static_assert(RegTwiddles<NC, L, RL, R, NS>::OK, "register twiddles: constant 16th-root steps between a lane's butterflies");
  if constexpr (M < RL / R) {
    twiddle_reg_apply<NC, L, RL, R, NS, M, 1>(v, twr);
    Dft<R>::run(&v[M * R]);
    twiddle_butterfly_reg<NC, L, RL, R, NS, M + 1>(v, twr);
  }
}
template <int NC, int L, int RL, int R, int NS>
__device__ __forceinline__ void load_stage_twiddles(cf (&twr)[R - 1], const cf* __restrict__ tw_global, int l) {
#pragma unroll
  for (int r = 1; r < R; ++r) twr[r - 1] = tw_global[(r - 1) * NS + l % NS];
}

// Can padidx(j0 + r NS) be formed as padidx(j0) + (r NS + r NS / 32) for every butterfly of a radix-R stage?  j0 = A + k with A a
// multiple of NS R and k < NS; the split is exact iff (j0 mod 32) + (r NS mod 32) < 32 -- checked here for every residue.
template <int R, int NS>
constexpr bool pad_split_ok() {
  int g = NS * R;
  while (32 % g != 0 && g > 1) {   // gcd(NS R, 32) for the power-of-two cases; anything else: no split
    if (g % 2) return false;
    g /= 2;
  }
  if (32 % g != 0) return false;
  for (int a = 0; a < 32; a += g)
    for (int k = 0; k < NS && k < 32; ++k)
      for (int r = 0; r < R; ++r)
        if ((a + k) % 32 + (r * NS) % 32 >= 32) return false;
  return (NS & (NS - 1)) == 0 && (R & (R - 1)) == 0;
}
template <int NC, int L, int RL, int R, int NS>
__device__ __forceinline__ void lds_store_stage(const cf (&v)[RL], cf* line, int l) {
  constexpr int NB = RL / R;
#pragma unroll
  for (int m = 0; m < NB; ++m) {
    const int j = l + L * m;
    const int k = j % NS;
    const int j0 = (j - k) * R + k;
    if constexpr (pad_split_ok<R, NS>()) {   // one lane-dependent address per butterfly, immediate offsets (see lds_load_stage)
      cf* base = line + padidx<NC>(j0);
#pragma unroll
      for (int r = 0; r < R; ++r) base[r * NS + ((r * NS) >> 5)] = v[m * R + r];
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) line[padidx<NC>(j0 + r * NS)] = v[m * R + r];
    }
  }
}

// Exchange synchronisation.  When a line's L lanes live inside one wave (L <= 64, lines never
// straddle waves) the stage exchanges only need wave-level ordering: a wave's LDS operations
// execute in issue order, so a compiler fence is enough and the waves of a workgroup run
// decoupled.  Otherwise a workgroup barrier.
template <bool WAVE>
__device__ __forceinline__ void exchange_sync() {
  if constexpr (WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// Second exchange of the 1024-point plan (64 lanes x 16 points, radices 16 x 8 x 8) WITHOUT LDS.  Between the two radix-8 stages
// element (lane 16 g + c, slot m*8 + 4a + b) of the next stage is element (lane 16 b + c, slot a*8 + 4m + g) of the previous one:
// the column c inside a row of 16 lanes stays, and for every (a, m) the four registers q = 0..3 at slots a*8 + 4m + q are
// transposed against the four lane ROWS.  gfx950's v_permlane32_swap (upper half of vdst <-> lower half of vsrc) and
// v_permlane16_swap (odd rows of vdst <-> even rows of vsrc) do a 4 x 4 row transpose of four registers in four instructions:
// 32 VALU swaps replace 16 ds_write_b64 + 16 ds_read_b64 and a wave-level sync in a kernel whose LDS pipe is the busiest unit
// (pencil kernel at C4: SQ_ACTIVE_INST_LDS x 16 waves ~ 90 % of the CU's cycles).  tools/micro/permlane_swap.hip pins the semantics.
template <int NC, int L, bool WAVE>
constexpr bool swap_exchange2() {
  return WAVE && NC == 1024 && L == 64 && PlanInfo<NC>::R0 == 16 && PlanInfo<NC>::R1 == 8 && PlanInfo<NC>::R2 == 8;
}
typedef unsigned vps_u2 __attribute__((ext_vector_type(2)));
// y_b at lane row g = x_g at lane row b (rows of 16 lanes), in place
__device__ __forceinline__ void rows_transpose4(float& x0, float& x1, float& x2, float& x3) {
  vps_u2 r;
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x0), __float_as_uint(x2), false, false);
  x0 = __uint_as_float(r.x); x2 = __uint_as_float(r.y);
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x1), __float_as_uint(x3), false, false);
  x1 = __uint_as_float(r.x); x3 = __uint_as_float(r.y);
  r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x0), __float_as_uint(x1), false, false);
  x0 = __uint_as_float(r.x); x1 = __uint_as_float(r.y);
  r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x2), __float_as_uint(x3), false, false);
  x2 = __uint_as_float(r.x); x3 = __uint_as_float(r.y);
}

// Runs stages 1.. (stage 0 inputs already in v).  On return v holds the spectrum:
// v[m*RLAST + r] = F[l + L*m + r*NC/RLAST].  L lanes per line (default: the plan's; the persistent transposing pass
// of the longest lines runs a line on half as many lanes with twice the points each).
// TWREG: the twiddles of stage 2 come from registers (twr); see twiddle_butterfly_reg
template <int NC, int L, bool WAVE, bool TWREG = false>
__device__ __forceinline__ void fft_from_regs_l(cf (&v)[NC / L], cf* line, const cf* tw, int l, const cf* twr = nullptr) {
  typedef PlanInfo<NC> PI;
  constexpr int RL = NC / L;
  static_assert(RL % PI::R0 == 0 && RL % PI::R1 == 0 && RL % PI::R2 == 0, "radix must divide RL");
  twiddle_butterfly<NC, L, RL, PI::R0, 1>(v, tw, l);
  if constexpr (PI::R1 > 1) {
    lds_store_stage<NC, L, RL, PI::R0, 1>(v, line, l);
    exchange_sync<WAVE>();
    lds_load_stage<NC, L, RL, PI::R1>(v, line, l);
    twiddle_butterfly<NC, L, RL, PI::R1, PI::NS1>(v, tw, l);
    if constexpr (PI::R2 > 1) {
      if constexpr (swap_exchange2<NC, L, WAVE>()) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {   // the four (a, m) groups: slots 4 g4 .. 4 g4 + 3
          rows_transpose4(v[4 * g4].x, v[4 * g4 + 1].x, v[4 * g4 + 2].x, v[4 * g4 + 3].x);
          rows_transpose4(v[4 * g4].y, v[4 * g4 + 1].y, v[4 * g4 + 2].y, v[4 * g4 + 3].y);
        }
        // slot m*8 + 4a + b of the next stage <- transposed slot a*8 + 4m + b: (a, m) = (0, 1) and (1, 0) trade places
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const cf tmp = v[4 + b];
          v[4 + b] = v[8 + b];
          v[8 + b] = tmp;
        }
      } else {
        exchange_sync<WAVE>();
        lds_store_stage<NC, L, RL, PI::R1, PI::NS1>(v, line, l);
        exchange_sync<WAVE>();
        lds_load_stage<NC, L, RL, PI::R2>(v, line, l);
      }
      if constexpr (TWREG)
        twiddle_butterfly_reg<NC, L, RL, PI::R2, PI::NS2>(v, twr);
      else
        twiddle_butterfly<NC, L, RL, PI::R2, PI::NS2>(v, tw + PI::TW1, l);
    }
  }
}
template <int NC, bool WAVE = false, bool TWREG = false>
__device__ __forceinline__ void fft_from_regs(cf (&v)[PlanInfo<NC>::RL], cf* line, const cf* tw, int l, const cf* twr = nullptr) {
  fft_from_regs_l<NC, PlanInfo<NC>::L, WAVE, TWREG>(v, line, tw, l, twr);
}

template <int NC>
struct LastRadix {
  typedef PlanInfo<NC> PI;
  static constexpr int R = (PI::R2 > 1) ? PI::R2 : ((PI::R1 > 1) ? PI::R1 : PI::R0);
};

// output index of register slot i = m*R + r after the last stage
template <int NC, int L>
__device__ __forceinline__ int out_index_l(int l, int i) {
  constexpr int R = LastRadix<NC>::R;
  const int m = i / R, r = i % R;
  return l + L * m + r * (NC / R);
}
template <int NC>
__device__ __forceinline__ int out_index(int l, int i) {
  return out_index_l<NC, PlanInfo<NC>::L>(l, i);
}

// host-side twiddle image for complex length NC (double precision, rounded once)
template <int NC>
void build_stage_tw(std::vector<cf>& out) {
  typedef PlanInfo<NC> PI;
  out.assign(PI::TW > 0 ? PI::TW : 1, make_float2(1.f, 0.f));
  const double tp = -2.0 * 3.14159265358979323846;
  if (PI::R1 > 1)
    for (int r = 1; r < PI::R1; ++r)
      for (int k = 0; k < PI::NS1; ++k) {
        double a = tp * (double)r * (double)k / (double)(PI::NS1 * PI::R1);
        out[(r - 1) * PI::NS1 + k] = make_float2((float)cos(a), (float)sin(a));
      }
  if (PI::R2 > 1)
    for (int r = 1; r < PI::R2; ++r)
      for (int k = 0; k < PI::NS2; ++k) {
        double a = tp * (double)r * (double)k / (double)(PI::NS2 * PI::R2);
        out[PI::TW1 + (r - 1) * PI::NS2 + k] = make_float2((float)cos(a), (float)sin(a));
      }
}

// ---- loads, stores and the real-input epilogue that more than one pass uses ----
__device__ __forceinline__ int packed_row(int k, int NC, int kc_pack) {
  return (kc_pack < 0 || k <= kc_pack) ? k : k - (NC - 2 * kc_pack - 1);
}

// Non-temporal (streaming) access to one complex value: data that is written once for the next pass
// or read once from the previous one should not displace what the caches hold.
// Measured (512^3 / 1024^3): x-pass loads -12 / -14 %, z-side stores -6 %.
__device__ __forceinline__ cf load_stream(const cf* ptr) {
  const double raw = __builtin_nontemporal_load(reinterpret_cast<const double*>(ptr));
  return *reinterpret_cast<const cf*>(&raw);
}
__device__ __forceinline__ void store_stream(cf* ptr, cf v) {
  __builtin_nontemporal_store(*reinterpret_cast<const double*>(&v), reinterpret_cast<double*>(ptr));
}

// Real-input post-processing of a transposed tile image buf[k][t] (NC packed-complex outputs Z per line):
//   X[k] = 0.5*((Z[k]+conj(Z[NC-k])) - i w^k (Z[k]-conj(Z[NC-k]))),  w = exp(-2 pi i/(2 NC)),
// X[0] and X[NC] (Nyquist, stored apart) real.  Modes k and NC-k share Z[k], Z[NC-k] and, because
// w^(NC-k) = -conj(w^k), the product w^k (Z[k]-conj(Z[NC-k])): one thread writes both.
template <int NC, int T, int NT, bool BOUNDS, bool PLAIN = false>
__device__ __forceinline__ void r2c_store_tile(const cf* buf, int tid, const cf* __restrict__ tw_r2c, cf* out,
                                               long long out_ok, cf* nyq, int nlive) {
  // pair index kp = 0 .. NC/2 (the last one only for odd NC: for even NC the self-paired mode NC/2 rides with kp = 0)
  constexpr int PAIRS = (NC / 2 + (NC & 1)) * T;
  constexpr int IT = (PAIRS + NT - 1) / NT;
#pragma unroll 4
  for (int i = 0; i < IT; ++i) {
    const int idx = tid + i * NT;
    if ((PAIRS % NT) != 0 && idx >= PAIRS) break;
    const int tt = idx % T, k = idx / T;
    const bool ok = !BOUNDS || tt < nlive;
    const cf zk = buf[tridx<T>(k, tt)];
    if (k == 0) {
      if (ok) {
        out[tt] = make_float2(zk.x + zk.y, 0.f);
        nyq[tt] = make_float2(zk.x - zk.y, 0.f);
      }
      if constexpr ((NC & 1) == 0) {
        const cf zh = buf[tridx<T>(NC / 2, tt)];
        if (ok) out[(long long)(NC / 2) * out_ok + tt] = make_float2(zh.x, -zh.y);
      }
    } else {
      const cf zn = buf[tridx<T>(NC - k, tt)];
      const cf w = tw_r2c[k];
      const cf sm = make_float2(zk.x + zn.x, zk.y - zn.y);   // Z[k] + conj(Z[NC-k])
      const cf d = make_float2(zk.x - zn.x, zk.y + zn.y);    // Z[k] - conj(Z[NC-k])
      const cf wd = cmul(w, d);
      if (ok) {
        // -i * wd = (wd.y, -wd.x);  for NC-k: conj(sm) and -i * conj(wd) = (-wd.y, -wd.x)
        if constexpr (PLAIN) {
          out[(long long)k * out_ok + tt] = make_float2(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));
          out[(long long)(NC - k) * out_ok + tt] = make_float2(0.5f * (sm.x - wd.y), 0.5f * (-sm.y - wd.x));
        } else {
        store_stream(&out[(long long)k * out_ok + tt], make_float2(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x)));
        store_stream(&out[(long long)(NC - k) * out_ok + tt], make_float2(0.5f * (sm.x - wd.y), 0.5f * (-sm.y - wd.x)));
        }
      }
    }
  }
}

// The same for 8-line tiles with 16-byte stores: a thread owns the lines (tt, tt + 1) of a mode pair, so a 64-byte output
// segment leaves as four dwordx4 stores instead of eight dwordx2 (half the store instructions of the pencil kernel's epilogue).
// wpre: a thread's ITEMS / NT real-to-complex twiddles where a caller has loaded them ahead; none does (measured slower, DESIGN.md
// section 7).  The parameter stays because without the select the compiler schedules the epilogue of the 8-line pencil kernels
// differently, and the commit that retired that trial was held to byte-identical device code.
template <int NC, int T, int NT, bool PLAIN = false>
__device__ __forceinline__ void r2c_store_tile16(const cf* buf, int tid, const cf* __restrict__ tw_r2c, cf* out,
                                                 long long out_ok, cf* nyq, const cf* wpre = nullptr) {
  static_assert((NC & 1) == 0 && (T & 1) == 0, "pairs of lines");
  constexpr int H = T / 2;
  constexpr int ITEMS = (NC / 2) * H;
  static_assert(ITEMS % NT == 0, "whole rounds");
#pragma unroll 4
  for (int i = 0; i < ITEMS / NT; ++i) {
    const int idx = tid + i * NT;
    const int tt = (idx % H) * 2, k = idx / H;
    const cf a0 = buf[tridx<T>(k, tt)], a1 = buf[tridx<T>(k, tt + 1)];
    if (k == 0) {
      *reinterpret_cast<vps_f4*>(&out[tt]) = vps_f4{a0.x + a0.y, 0.f, a1.x + a1.y, 0.f};
      *reinterpret_cast<vps_f4*>(&nyq[tt]) = vps_f4{a0.x - a0.y, 0.f, a1.x - a1.y, 0.f};
      const cf h0 = buf[tridx<T>(NC / 2, tt)], h1 = buf[tridx<T>(NC / 2, tt + 1)];
      *reinterpret_cast<vps_f4*>(&out[(long long)(NC / 2) * out_ok + tt]) = vps_f4{h0.x, -h0.y, h1.x, -h1.y};
    } else {
      const cf n0 = buf[tridx<T>(NC - k, tt)], n1 = buf[tridx<T>(NC - k, tt + 1)];
      const cf w = wpre ? wpre[i] : tw_r2c[k];
      const cf s0 = make_float2(a0.x + n0.x, a0.y - n0.y), d0 = make_float2(a0.x - n0.x, a0.y + n0.y);
      const cf s1 = make_float2(a1.x + n1.x, a1.y - n1.y), d1 = make_float2(a1.x - n1.x, a1.y + n1.y);
      const cf w0 = cmul(w, d0), w1 = cmul(w, d1);
      const vps_f4 lo = {0.5f * (s0.x + w0.y), 0.5f * (s0.y - w0.x), 0.5f * (s1.x + w1.y), 0.5f * (s1.y - w1.x)};
      const vps_f4 hi = {0.5f * (s0.x - w0.y), 0.5f * (-s0.y - w0.x), 0.5f * (s1.x - w1.y), 0.5f * (-s1.y - w1.x)};
      if constexpr (PLAIN) {
        *reinterpret_cast<vps_f4*>(&out[(long long)k * out_ok + tt]) = lo;
        *reinterpret_cast<vps_f4*>(&out[(long long)(NC - k) * out_ok + tt]) = hi;
      } else {
        __builtin_nontemporal_store(lo, reinterpret_cast<vps_f4*>(&out[(long long)k * out_ok + tt]));
        __builtin_nontemporal_store(hi, reinterpret_cast<vps_f4*>(&out[(long long)(NC - k) * out_ok + tt]));
      }
    }
  }
}

// ---- what the launchers and the host API derive from a line length ----
template <int NC>
constexpr int transpose_T() {
  // tile width: 16 lines (128-byte output segments) while the LDS image fits,
  // at least one full wave of threads for short lines
  if (NC <= 16) return 64;
  if (NC <= 512) return 16;
  if (NC <= 2048) return 8;
  return 4;
}
// lines per x-pass workgroup: 256 threads' worth (4096-point lines, L = 256: ONE line)
template <int NC>
constexpr int xpass_T() {
  constexpr int L = Plan<NC>::L;
  constexpr int t = (256 / L) > 1 ? (256 / L) : 1;
  return (t > 1 && (t & 1)) ? t - 1 : t;   // even, so that a tile holds whole (ky, N-ky) pairs (L = 50 -> 4)
}

// y-lines per pencil: 16 (128-byte output segments); 8 from 2048-cell lines on: at 2048 cells 512
// threads and 76 KB of LDS per workgroup, so TWO workgroups share a CU and one's stores overlap the other's LDS work.  The two
// pencils that complete a 128-byte output line are placed on one XCD (remap in the kernel); 38 % of the lines still
// reach HBM as two halves (PMC WRITE_SIZE 142 GB for 103 GB of output), which costs less than the lost overlap.
// Measured at C4 (2048^3, ms per step of 7 fields): 16 lines x 64 lanes, spilling 111; 8 x 64 spilling 118, not spilling
// (two waves per SIMD) 106; 16 x 32 (one workgroup per CU, full-line writes) 88; 8 x 32 83; 4 x 64 (32-byte segments) 228.
constexpr int pencil_tp(int NC) { return NC >= 1024 ? 8 : 16; }   // (the host's callers: vps_pencil_tp())
template <int NC>
constexpr int pencil_tp() {
  return pencil_tp(NC);
}

// Shortest segment the SEG x pass loads: power-of-two lines whose plan has a multiple of 64 lanes (N = 1024, 2048, 4096) carry
// only the scalar-base load of load_line, which needs segments of at least L points; every other line takes any segment.
template <int NC>
constexpr int x_seg_min_len() {
  return ((NC & (NC - 1)) == 0 && PlanInfo<NC>::L % 64 == 0) ? PlanInfo<NC>::L : 1;
}
// most segments a line of N points may come in (vps_x_max_ranks); x_seg_min_len is 1 for every line that is no power of two
template <int NC = 16>
constexpr int x_max_segments(int N) {
  if (N == NC) return NC / x_seg_min_len<NC>();
  if constexpr (NC < 4096) return x_max_segments<2 * NC>(N);
  return N;
}

}  // namespace
