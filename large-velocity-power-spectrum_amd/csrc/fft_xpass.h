// x pass: the binning / writing kernel, the reduction of its per-workgroup partials and their launcher.  Kernel unit only
// (fft_parts.hip).
#pragma once
#include "fft_line.h"

namespace {

// ------------------------------------------------------------------------------
// x pass: lines are contiguous (or made of nseg contiguous segments); the result is
// binned straight from registers (MODE 0) or written in place order (MODE 1).
// Persistent workgroups loop over tiles of T lines.
// ------------------------------------------------------------------------------

// FAST (MODE 0 only): the k^2 table is symmetric (k2[N-i] == k2[i]) and non-decreasing on
// [0, N/2] -- true for 2 pi fftfreq -- so kx and -kx share one s and one shell: a lane
// then walks RL/2 values of |kx|, adds the two mirrored |F|^2 and issues one LDS atomic
// per |kx|, with no per-element branches (the host checks the table, vps_set_binning).
// FASTMODE 2 = FAST with INTEGER shells: in units of (2 pi / L)^2 the reference's s = (kx^2 + ky^2) + kz^2 is the integer
// n = ix^2 + iy^2 + iz^2 up to float64 rounding, and where no shell threshold lies within 1e-9 (relative) of an integer --
// both reference flavours: their edges are half-integer multiples of 2 pi / L -- the float64 comparison thr[b] <= s < thr[b+1]
// and the integer comparison nthr[b] <= n < nthr[b+1] (nthr[b] = ceil(thr[b] / k2[1])) decide every mode alike.  The kernel
// then needs no k^2 table at all: no float64 registers or adds per mode, 4-byte thresholds, and nothing to load per tile or
// per line (tile_beyond_shells / locate_line are arithmetic on the tile index).  vps_set_binning checks the condition and
// falls back to FASTMODE 1 where it fails (custom k ranges with edges on integer multiples).
// With integer shells the 2048-point plan also keeps its last stage's twiddles in registers (x_twreg): thresholds 4 KB + sums
// 8 KB + counts 4 KB + stage-1 twiddles 2 KB + two lines 34 KB = 52 KB, so THREE workgroups share a CU instead of two
// (70.6 KB before).  Measured at C4: persistent workgroups per CU 1 -> 2: 35.7 -> 22.7 ms per vector launch.
// (Lines made of segments -- the received blocks of a slab exchange -- take the same form: their loads are a scalar base and
//  one lane offset, load_line.  While the kernel also carried the general segment addressing, a 64-bit offset per element for
//  segments shorter than a line's lanes, that path alone cost 60 VGPRs and the register-twiddle variant spilled 97.)
template <int NC, int FASTMODE, bool SEG>
constexpr bool x_twreg() {
  return FASTMODE == 2 && NC == 2048 && PlanInfo<NC>::R2 > 1;
}
// HELM (MODE 0, ncomp = 3): Helmholtz decomposition.  While the three components of a line are transformed one after the other,
// D = k'x Fx + k'y Fy + k'z Fz (k' = integer mode numbers, the Nyquist entry N/2 of every axis set to 0) is accumulated in
// registers; |D|^2 / |k'|^2 (0 where k' = 0) -- the compressive part of sum_c |F_c|^2 -- goes through a second LDS image next
// to the |F|^2 image and is binned with the same shell decision into a second set of shell sums (p.psumc).
// k' is odd under k -> -k, so a mode and its Hermitian partner have the same |D|^2: the half spectrum's multiplicities hold.
template <int NC>
constexpr int x_cimg_pitch(bool fast) {   // floats per line of the HELM image: index k + k / CH, k < NC
  return NC + NC / (fast ? PlanInfo<NC>::RL / 2 : PlanInfo<NC>::RL) + 1;
}
// REALB (MODE 0, one component): the signed binning of vps_fft_x modes 6 / 7 -- Re F(kx) goes into the line's image where
// |F|^2 goes otherwise (the imaginary part is dropped); tables, multiplicities, shell decision, pairing, row cut and the
// float64 LDS atomics are the ones below, untouched.  A sum of values is binned, so +-kx and +-ky still share one atomic.
// MODE 5: |F|^2 ADDED into a full Hermitian [N][N][N] float32 grid, the line (ky, kz) at [kz][ky][:] and, for 0 < kz < N/2,
// once more at its partner [N-kz][(N-ky)%N][(N-kx)%N]; the planes kz = 0 and N/2 hold their partners as lines of their own.
template <int NC, int T, int MODE, bool SEG, bool COUNT, int FASTMODE, bool HELM = false, bool REALB = false>
__global__ void __launch_bounds__(T* PlanInfo<NC>::L, (x_twreg<NC, FASTMODE, SEG>() ? (HELM ? 2 : 3) : 1)) fft_x_pass(const XParams p) {
  typedef PlanInfo<NC> PI;
  constexpr bool FAST = FASTMODE != 0, INTB = FASTMODE == 2, TWREG = x_twreg<NC, FASTMODE, SEG>();
  constexpr int L = PI::L, RL = PI::RL, NT = T * L;
  constexpr int H = RL / 2;   // |kx| values per lane on the FAST path
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  // carve: thr (double, nbins+2 with a +inf sentinel; INTB: unsigned, 0xffffffff sentinel) | hsum (double) | [HELM: hsumc (double)]
  //        | tw | line buffers | hcnt | [window factors] | [HELM: T images of |D|^2 / |k'|^2]
  double* thr = reinterpret_cast<double*>(smem_raw);
  unsigned* nthr = reinterpret_cast<unsigned*>(smem_raw);
  double* hsum = INTB ? reinterpret_cast<double*>(nthr + ((p.nbins + 3) & ~1)) : thr + (MODE == 0 ? (p.nbins + 2) : 0);
  double* hsumc = hsum + p.nbins;   // (HELM only)
  cf* tw_lds = reinterpret_cast<cf*>(hsum + (MODE == 0 ? p.nbins : 0) + (HELM ? p.nbins : 0));
  constexpr int TWCOPY = TWREG ? PI::TW1 : PI::TW;                      // twiddle entries staged in LDS
  constexpr int TWRES = TWREG ? ((PI::TW1 + 1) & ~1) : PI::TWL;         // ... and reserved for them
  cf* buf = tw_lds + TWRES;
  const cf* tw = PI::TWLDS ? tw_lds : p.tw_stage;
  unsigned* hcnt = reinterpret_cast<unsigned*>(buf + T * PI::PITCH);
  float* wl = reinterpret_cast<float*>(hcnt + ((MODE == 0 && COUNT) ? p.nbins : 0));   // [NC] window factors (MODE 0 with p.win)
  constexpr int CIMG = x_cimg_pitch<NC>(FAST);

  const int tid = threadIdx.x;
  const int t = tid / L, l = tid % L;
  float* cimg = wl + (p.win ? NC : 0) + (HELM ? t * CIMG : 0);   // HELM: this line's |D|^2 / |k'|^2 image
  if constexpr (PI::TWLDS)
    for (int i = tid; i < TWCOPY; i += NT) tw_lds[i] = p.tw_stage[i];
  cf twr[TWREG ? (PI::R2 - 1) : 1];
  if constexpr (TWREG) load_stage_twiddles<NC, L, RL, PI::R2, PI::NS2>(twr, p.tw_stage + PI::TW1, l);
  // fl(kx*kx) of this lane's contiguous chunk of RL kx values, ordered by non-decreasing
  // |kx|: the chunks of the negative-frequency half (index >= NC/2) are walked backwards
  double k2x[(MODE == 0 && !INTB) ? (FAST ? H : RL) : 1];
  const bool rev = (l * RL) >= NC / 2;
  if constexpr (MODE == 0) {
    if constexpr (INTB) {
      for (int i = tid; i <= p.nbins + 1; i += NT) nthr[i] = (i <= p.nbins) ? p.nthr[i] : 0xffffffffu;
    } else {
      for (int i = tid; i <= p.nbins + 1; i += NT) thr[i] = (i <= p.nbins) ? p.thr[i] : INFINITY;
    }
    for (int i = tid; i < p.nbins; i += NT) {
      hsum[i] = 0.0;
      if constexpr (HELM) hsumc[i] = 0.0;
      if constexpr (COUNT) hcnt[i] = 0u;
    }
    if (p.win)
      for (int i = tid; i < NC; i += NT) wl[i] = p.win[i];
    if constexpr (INTB) {
    } else if constexpr (FAST) {
#pragma unroll
      for (int i = 0; i < H; ++i) k2x[i] = p.k2[l * H + i];
    } else {
#pragma unroll
      for (int i = 0; i < RL; ++i) k2x[i] = p.k2[l * RL + (rev ? RL - 1 - i : i)];
    }
  }
  __syncthreads();

  cf* line = buf + t * PI::PITCH;
  const int segmask = p.seglen - 1;
  const long long ntiles = (p.nlines + T - 1) / T;
  // PAIR (FAST path on whole ky ranges): a tile holds T/2 lines ky and their mirrors N-ky,
  // which share every s with them, so one lane bins four modes (+-kx, +-ky) per step.
  // wave-level synchronisation of everything line-local (exchanges, |F|^2 image)
  constexpr bool WSYNC = (L <= 64) && (64 % L == 0);
  // pairs are adjacent lines (t, t^1): with at least two lines per wave a pair never leaves its wave
  constexpr bool CANPAIR = FAST && (T >= 2) && (NC >= T) && (NC % T == 0) && (!WSYNC || L <= 32);
  const bool pair = CANPAIR && p.pair;
  constexpr int TH = (T >= 2) ? T / 2 : 1;
  // A PAIR tile holds TH consecutive |ky|, aligned to TH.  The y passes of a binning-only scope store the rows |ky| <= kcut[kz],
  // kcut = the exact cut rounded UP to 16 k + 15 (vps_set_binning, api.hip).  Where TH divides 16 (every power-of-two grid from
  // 128 on) a tile that is transformed lies entirely inside the stored rows.  Elsewhere (TH = 32 on the small grids, TH = 6 on
  // 3 2^a) a transformed tile may read rows the y pass left unwritten: every mode of such a row has fl(ky^2 + kz^2) >=
  // thr[nbins], the shell search below puts it at bin == nbins, and the `bin < nbins` guard keeps whatever the row held
  // (NaN included) out of every sum and count -- tests/test_gpu_configs.py runs the exchange buffers NaN-prefilled for this.
  // tile -> this lane's line, and the loads of its stage-0 inputs
  long long li = 0, lrow = 0;   // line index inside the launch's range, and the row of the input it is read from
  bool live = false, mirrored = false, has_partner = false;
  double k2y = 0.0, k2z = 0.0;   // fl(ky*ky), fl(kz*kz) of the line (MODE 0)
  unsigned nyz = 0u;             // INTB: iy^2 + iz^2 of the line
  float wyz = 1.f;               // window factor of the line's (ky, kz)
  float kyp = 0.f, kzp = 0.f;    // HELM: k'y, k'z of the line
  unsigned wz = 1u;              // Hermitian multiplicity of its kz plane
  double k2half = 0.0;
  if constexpr (MODE == 0 && !INTB) k2half = p.k2[NC / 2];
  cf v[RL];
  // PAIR tiles whose smallest |ky| already puts every mode of the tile beyond the last shell edge -- fl(ky^2 + kz^2) >=
  // thr[nbins], and s = (kx^2 + ky^2) + kz^2 can only be larger -- are neither loaded nor transformed: with the default
  // k range (kmax = Nyquist) that is the quarter of each kz plane outside the inscribed circle (1 - pi/4 = 21 %).
  // (The |ky| order of a plane's tiles is rotated from plane to plane: a persistent workgroup takes every gridDim-th
  // tile, and without the rotation the same workgroups would always draw the skipped outer |ky| and the others never.)
  constexpr long long tiles_per_plane = (NC / T) > 0 ? (NC / T) : 1;
  auto tile_q = [&](long long tile) -> int {   // which group of TH |ky| values PAIR tile `tile` holds
    const long long plane = tile / tiles_per_plane;
    return (int)((tile % tiles_per_plane + plane * 619) % tiles_per_plane);
  };
  auto tile_beyond_shells = [&](long long tile) -> bool {
    if constexpr (MODE == 0 && FAST) {
      if (pair) {
        const int kz = p.kz0 + ((int)(p.line0 / NC) + (int)(tile / tiles_per_plane)) * p.kz_step;
        if constexpr (INTB) {
          const unsigned ka = (unsigned)(tile_q(tile) * TH);
          return ka * ka + (unsigned)kz * (unsigned)kz >= p.nmax;
        } else {
          return (p.k2[tile_q(tile) * TH] + p.k2[kz]) >= p.thr[p.nbins];
        }
      }
    }
    return false;
  };
  auto locate_line = [&](long long tile) {
    li = tile * T + t;       // local line index
    mirrored = false;        // this line is the N-ky partner of line t - 1
    has_partner = false;     // line t + 1 holds this line's N-ky partner
    if (pair) {
      const long long plane = tile / tiles_per_plane;
      const int q = tile_q(tile);
      const int ky_a = q * TH + (t >> 1);
      const int ky = ((t & 1) == 0) ? ky_a : (ky_a == 0 ? NC / 2 : NC - ky_a);
      li = plane * NC + ky;
      mirrored = ((t & 1) == 1) && (ky_a != 0);
      has_partner = ((t & 1) == 0) && (ky_a != 0);
    }
    live = li < p.nlines && !tile_beyond_shells(tile);
    lrow = li;
    if (p.ptab) {   // chunked exchange (line0 = 0): every mode of a row that was not sent lies beyond the last shell edge
      const int ky = (int)(li % NC);
      const int2 pt = p.ptab[li / NC];
      live = live && (pt.y < 0 || ky <= pt.y || ky >= NC - pt.y);
      lrow = pt.x + packed_row(ky, NC, pt.y);
    }
    if constexpr (MODE == 0) {
      if (live) {
        const long long g = p.line0 + li;
        // (lines of the x pass have N = NC points: a compile-time divisor instead of a 64-bit division per tile and thread)
        const int kz = p.kz0 + (int)(g / NC) * p.kz_step;
        if constexpr (INTB) {
          const int kyi = (int)(g % NC);
          const unsigned iy = (unsigned)(2 * kyi <= NC ? kyi : NC - kyi);
          nyz = iy * iy + (unsigned)kz * (unsigned)kz;
        } else {
          k2y = p.k2[(int)(g % NC)];
          k2z = p.k2[kz];
        }
        wz = (kz == 0 || 2 * kz == NC) ? 1u : 2u;
        if (p.win) wyz = p.win[(int)(g % NC)] * p.win[kz];
        if constexpr (HELM) {
          const int kyi = (int)(g % NC);
          kyp = (2 * kyi < NC) ? (float)kyi : (2 * kyi == NC ? 0.f : (float)(kyi - NC));
          kzp = (2 * kz == NC) ? 0.f : (float)kz;
        }
      }
    }
  };
  auto load_line = [&](cf (&v)[RL], int c, int l) {   // l: the lane index (callers inside loops pass an opaque copy)
    constexpr int R = PI::R0, NB = RL / R;
    const cf* base = (c == 0 ? p.in : (c == 1 ? p.in1 : p.in2)) + lrow * p.seglen;
    if constexpr (!SEG && (L % 64 == 0)) {
      // A wave holds lanes of ONE line: whether the line is read at all is wave-uniform -- one scalar branch around the RL loads
      // instead of an exec-mask branch around every pair of them (which is what `live ? load : 0` per element compiles to).
      if (__builtin_amdgcn_readfirstlane((int)live)) {
#pragma unroll
        for (int m = 0; m < NB; ++m)
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const double raw = __builtin_nontemporal_load(reinterpret_cast<const double*>(&base[l + L * m + r * (NC / R)]));
            v[m * R + r] = *reinterpret_cast<const cf*>(&raw);
          }
      } else {
#pragma unroll
        for (int i = 0; i < RL; ++i) v[i] = make_float2(0.f, 0.f);
      }
      return;
    }
    if constexpr (SEG && (L % 64 == 0)) {
      // A wave holds lanes of ONE line here, so the line's base is wave-uniform; and with power-of-two segments of at least L
      // elements, element x = l + xr (xr = L m + r NC/R, a multiple of L) sits in segment xr >> seg_shift at offset
      // (xr & segmask) + l with no carry.  Everything but l is then scalar: the loads take an SGPR base and one 32-bit lane
      // offset instead of a 64-bit multiply-add per element (x pass of a received 2048^3 chunk, 8 segments: 4.22 -> see DESIGN).
      // (power-of-two lines: launch_x refuses segments shorter than L -- more than NC / L ranks -- so this is the only path the
      //  kernel carries for them; the general form below, with a 64-bit offset per element, costs it ~60 VGPRs)
      constexpr bool ONLY_SCALAR = (NC & (NC - 1)) == 0;
      if (ONLY_SCALAR || (p.seg_shift >= 0 && p.seglen >= L)) {
        const unsigned long long ub = reinterpret_cast<unsigned long long>(base);
        const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)ub), bhi = __builtin_amdgcn_readfirstlane((unsigned)(ub >> 32));
        const cf* sbase = reinterpret_cast<const cf*>(((unsigned long long)bhi << 32) | blo);
        // (the shift through an empty asm: the RL segment offsets are loop-invariant, and hoisted out of the tile loop they
        //  sit in ~2 RL VGPRs for the whole kernel -- the scalar file is full -- which spills the register-twiddle variant;
        //  formed where they are used they are a handful of scalar operations per load)
        int sh = p.seg_shift;
        asm volatile("" : "+s"(sh));
        const int smask = (1 << sh) - 1;
        if (__builtin_amdgcn_readfirstlane((int)live)) {   // (wave-uniform: one scalar branch around all the loads)
#pragma unroll
          for (int m = 0; m < NB; ++m)
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const int xr = L * m + r * (NC / R);
              const long long off = (long long)(xr >> sh) * p.seg_stride + (xr & smask);
              // (uniform 64-bit base + zero-extended 32-bit lane offset: the saddr + voffset form of global_load, one VGPR of
              //  address for all loads instead of a 64-bit VGPR pair each)
              const char* sb = reinterpret_cast<const char*>(sbase + off);
              const double raw = __builtin_nontemporal_load(reinterpret_cast<const double*>(sb + (unsigned)l * 8u));
              v[m * R + r] = *reinterpret_cast<const cf*>(&raw);
            }
        } else {
#pragma unroll
          for (int i = 0; i < RL; ++i) v[i] = make_float2(0.f, 0.f);
        }
        return;
      }
    }
#pragma unroll
    for (int m = 0; m < NB; ++m)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int x = l + L * m + r * (NC / R);
        if constexpr (SEG) {
          // element x of the line sits in segment x >> seg_shift at offset x & segmask
          // (this exact form -- a conditional double load, reinterpreted -- keeps every load a streaming one
          // with one base register and immediate offsets; going through load_stream() did not)
          // (seg_shift < 0: segment length not a power of two -- the 2^a 5^b grids on several ranks)
          // (a power-of-two line divides into power-of-two segments only: no division path to compile, or to keep registers for)
          constexpr bool POW2 = (NC & (NC - 1)) == 0;
          const int sg = (POW2 || p.seg_shift >= 0) ? (x >> p.seg_shift) : x / p.seglen;
          const int so = (POW2 || p.seg_shift >= 0) ? (x & segmask) : x - sg * p.seglen;
          const double raw = live ? __builtin_nontemporal_load(reinterpret_cast<const double*>(
                                        &base[(long long)sg * p.seg_stride + so]))
                                  : 0.0;
          v[m * R + r] = *reinterpret_cast<const cf*>(&raw);
        } else {
          const double raw = live ? __builtin_nontemporal_load(reinterpret_cast<const double*>(&base[x])) : 0.0;
          v[m * R + r] = *reinterpret_cast<const cf*>(&raw);
        }
      }
  };
  if ((long long)blockIdx.x < ntiles) {
    locate_line(blockIdx.x);
    load_line(v, 0, l);
  }
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // (carrying the flag over from the prefetch's locate_line instead of testing again: -2 % at 2048, +30 % at 512 -- not kept)
    if (tile_beyond_shells(tile)) {   // (uniform over the workgroup) nothing to bin here: only keep the prefetch chain going
      if (tile + gridDim.x < ntiles) {
        locate_line(tile + gridDim.x);
        load_line(v, 0, l);
      }
      continue;
    }
    // line bookkeeping of THIS tile (v already holds, or is receiving, its inputs)
    const long long li_cur = li;
    const bool live_cur = live, mirrored_cur = mirrored, partner_cur = has_partner;
    const double k2y_cur = k2y, k2z_cur = k2z;
    const unsigned nyz_cur = nyz;
    const unsigned wz_cur = wz;
    const float wyz_cur = wyz;
    const float kyp_cur = kyp, kzp_cur = kzp;
    if constexpr (MODE != 0) {
      exchange_sync<WSYNC>();  // previous tile's readers are done with the line buffers
      fft_from_regs<NC, WSYNC, TWREG>(v, line, tw, l, twr);
    }
    if constexpr (MODE == 1) {
      if (live_cur) {
        cf* o = p.out + li_cur * (long long)NC;
#pragma unroll
        for (int i = 0; i < RL; ++i) o[out_index<NC>(l, i)] = v[i];
      }
    } else if constexpr (MODE == 4) {
      // transform only (timing aid): keep the results alive without storing them
#pragma unroll
      for (int i = 0; i < RL; ++i) asm volatile("" ::"v"(v[i].x), "v"(v[i].y));
    } else if constexpr (MODE == 2) {
      if (live_cur) {
        float* o = reinterpret_cast<float*>(p.out) + li_cur * (long long)NC;
#pragma unroll
        for (int i = 0; i < RL; ++i) o[out_index<NC>(l, i)] += v[i].x * v[i].x + v[i].y * v[i].y;
      }
    } else if constexpr (MODE == 5) {
      // p.out is the BASE of the full grid, whatever line0 / kz0 (fft_x_impl has checked 0 <= kz <= N/2).  For a register slot
      // i the lanes of a line hold consecutive kx (out_index = l + const): the direct store is one ascending run of 4 L bytes
      // per line, the mirrored one the same run of the partner line walked downwards -- the same cache lines, fully covered
      // by one wave instruction either way.  Every element has one writer: a plain read-modify-write.
      if (live_cur) {
        const long long g = p.line0 + li_cur;
        const int ky = (int)(g % NC), kz = p.kz0 + (int)(g / NC);
        float* base = reinterpret_cast<float*>(p.out);
        float* o = base + ((long long)kz * NC + ky) * NC;
        const bool mir = kz > 0 && 2 * kz < NC;
        float* m = mir ? base + ((long long)(NC - kz) * NC + (ky ? NC - ky : 0)) * NC : o;
#pragma unroll
        for (int i = 0; i < RL; ++i) {
          const int kx = out_index<NC>(l, i);
          const float a = v[i].x * v[i].x + v[i].y * v[i].y;
          o[kx] += a;
          if (mir) m[kx ? NC - kx : 0] += a;
        }
      }
    } else {
      // Shell sums.  |F|^2 goes through LDS once so that every lane gets a CONTIGUOUS chunk
      // of RL kx values: along kx the shell index moves monotonically (per half line), so a
      // lane accumulates each run of equal bins in registers and issues one LDS float64
      // atomic per run, and the lanes of a wave-instruction hit different bins.
      // The components of a vector field are transformed one after the other and their |F|^2 summed in
      // registers (the reference bins the SUM, interp.py:1372-1421), so the shell search and the LDS
      // atomics below run once per line, not once per component.  As soon as a transform has been
      // squared its registers take the next loads: the next component of this tile, or the first of
      // the next tile, which then fly while this tile is binned.
      float pacc[RL];
      float dre[HELM ? RL : 1], dim[HELM ? RL : 1];   // HELM: D = sum_c k'_c F_c of this lane's elements
      for (int c = 0; c < p.ncomp; ++c) {
        // opaque copy of the lane index: keeps the LDS / global addresses of this loop from being
        // hoisted out of it as ~50 extra live registers (an occupancy step)
        int lc = l;
        asm volatile("" : "+v"(lc));
        lc = (L & (L - 1)) == 0 ? (lc & (L - 1)) : lc % L;   // give the value range back to the compiler (address folding needs it)
        exchange_sync<WSYNC>();  // previous readers are done with the line buffers
        fft_from_regs<NC, WSYNC, TWREG>(v, line, tw, lc, twr);
#pragma unroll
        for (int i = 0; i < RL; ++i) {
          float a;
          if constexpr (REALB) a = v[i].x;
          else a = v[i].x * v[i].x + v[i].y * v[i].y;
          pacc[i] = (c == 0) ? a : pacc[i] + a;
        }
        if constexpr (HELM) {
#pragma unroll
          for (int i = 0; i < RL; ++i) {
            float kc;
            if (c == 0) {
              const int kx = out_index<NC>(lc, i);
              kc = (2 * kx < NC) ? (float)kx : (2 * kx == NC ? 0.f : (float)(kx - NC));
            } else {
              kc = (c == 1) ? kyp_cur : kzp_cur;
            }
            dre[i] = (c == 0) ? kc * v[i].x : fmaf(kc, v[i].x, dre[i]);
            dim[i] = (c == 0) ? kc * v[i].y : fmaf(kc, v[i].y, dim[i]);
          }
        }
        if (c + 1 < p.ncomp) {
          load_line(v, c + 1, lc);
        } else if (tile + gridDim.x < ntiles) {
          locate_line(tile + gridDim.x);
          load_line(v, 0, lc);
        }
      }
      float* pw = reinterpret_cast<float*>(line);
      if constexpr (PI::R1 > 1) exchange_sync<WSYNC>();  // last exchange fully consumed
      constexpr int CH = FAST ? H : RL;              // chunk length; one pad word per chunk
      {
        int lw = l;   // opaque again: 16 store addresses recomputed per tile instead of kept live
        asm volatile("" : "+v"(lw));
        lw = (L & (L - 1)) == 0 ? (lw & (L - 1)) : lw % L;
#pragma unroll
        for (int i = 0; i < RL; ++i) {
          // k = lw + c with c a multiple of CH wherever the plan's lanes are (power-of-two plans): k / CH = lw / CH + c / CH
          constexpr int RLAST = LastRadix<NC>::R;
          const int c = L * (i / RLAST) + (i % RLAST) * (NC / RLAST);
          if constexpr ((L % CH == 0) && ((NC / RLAST) % CH == 0)) {
            pw[(lw + lw / CH) + c + c / CH] = pacc[i];
          } else {
            const int k = out_index<NC>(lw, i);
            pw[k + k / CH] = pacc[i];
          }
          if constexpr (HELM) {
            // |D|^2 / |k'|^2 into the line's second image, same index (every k' component an integer < 2^12: exact in float)
            const int k = out_index<NC>(lw, i);
            const float kx = (2 * k < NC) ? (float)k : (2 * k == NC ? 0.f : (float)(k - NC));
            const float k2 = fmaf(kx, kx, fmaf(kyp_cur, kyp_cur, kzp_cur * kzp_cur));
            const float d2 = fmaf(dre[i], dre[i], dim[i] * dim[i]);
            cimg[k + k / CH] = (k2 > 0.f) ? d2 / k2 : 0.f;
          }
        }
      }
      exchange_sync<WSYNC>();
      if constexpr (FAST) {
        if (live_cur && !mirrored_cur) {
          const unsigned w = wz_cur * (partner_cur ? 2u : 1u);
          const float wf = (float)wz_cur * wyz_cur;   // Hermitian multiplicity x window factor of (ky, kz)
          // the partner line's |F|^2 image is the next line buffer
          constexpr int POFF = PI::PITCH * 2;
          const float* mine = pw + l * (H + 1);                        // kx = l*H + i
          const float* mirr = pw + (NC + NC / H - 1) - l * (H + 1);    // NC-kx for i >= 1 at mirr[-i]
          // Every |kx| is binned independently (no chain between the LDS reads): the edges
          // are uniform (checked by vps_set_binning), so the float guess is off by at most
          // one shell and is corrected against the exact float64 thresholds.
          auto bin_one = [&](int i, double k2xi) {
            int bin;
            if constexpr (INTB) {
              // n = ix^2 + iy^2 + iz^2: the float guess is within one shell, the integer thresholds decide
              const unsigned ix = (unsigned)(l * H + i);
              const unsigned n = ix * ix + nyz_cur;
              int g = (int)((sqrtf((float)n) * p.kf - p.edge0) * p.inv_spacing);
              g = min(max(g, 0), p.nbins - 1);
              const unsigned lo = nthr[g], hi = nthr[g + 1];
              bin = g - ((n < lo) ? 1 : 0) + ((n >= hi) ? 1 : 0);
            } else {
            // s = (kx*kx + ky*ky) + kz*kz with numpy's rounding (the table holds fl(k*k))
            const double s = (k2xi + k2y_cur) + k2z_cur;
            int g = (int)((sqrtf((float)s) - p.edge0) * p.inv_spacing);
            g = min(max(g, 0), p.nbins - 1);
            const double lo = thr[g], hi = thr[g + 1];
            bin = g - ((s < lo) ? 1 : 0) + ((s >= hi) ? 1 : 0);
            }
            float pv = mine[i];
            if (partner_cur) pv += mine[i + POFF];
            unsigned c = 1u;
            if (i > 0) {
              pv += mirr[-i];
              if (partner_cur) pv += mirr[POFF - i];
              c = 2u;
            } else if (l > 0) {
              pv += mirr[1];
              if (partner_cur) pv += mirr[POFF + 1];
              c = 2u;
            }
            float pc = 0.f;   // HELM: the same modes of the |D|^2 / |k'|^2 images
            if constexpr (HELM) {
              const float* cm = cimg + l * (H + 1);
              const float* cr = cimg + (NC + NC / H - 1) - l * (H + 1);
              pc = cm[i];
              if (partner_cur) pc += cm[i + CIMG];
              if (i > 0) {
                pc += cr[-i];
                if (partner_cur) pc += cr[CIMG - i];
              } else if (l > 0) {
                pc += cr[1];
                if (partner_cur) pc += cr[CIMG + 1];
              }
            }
            if ((unsigned)bin < (unsigned)p.nbins) {
              if (p.win) pv *= wl[l * H + i];
              atomicAdd(&hsum[bin], (double)(pv * wf));
              if constexpr (HELM) {
                if (p.win) pc *= wl[l * H + i];
                atomicAdd(&hsumc[bin], (double)(pc * wf));
              }
              if constexpr (COUNT) atomicAdd(&hcnt[bin], c * w);
            }
          };
#pragma unroll
          for (int i = 0; i < H; ++i) bin_one(i, INTB ? 0.0 : k2x[INTB ? 0 : i]);
          if (l == L - 1) {   // the unpaired kx = NC/2 mode
            int bin;
            if constexpr (INTB) {
              const unsigned n = (unsigned)(NC / 2) * (unsigned)(NC / 2) + nyz_cur;
              int g = (int)((sqrtf((float)n) * p.kf - p.edge0) * p.inv_spacing);
              g = min(max(g, 0), p.nbins - 1);
              bin = g - ((n < nthr[g]) ? 1 : 0) + ((n >= nthr[g + 1]) ? 1 : 0);
            } else {
            const double s = (k2half + k2y_cur) + k2z_cur;
            int g = (int)((sqrtf((float)s) - p.edge0) * p.inv_spacing);
            g = min(max(g, 0), p.nbins - 1);
            bin = g - ((s < thr[g]) ? 1 : 0) + ((s >= thr[g + 1]) ? 1 : 0);
            }
            if ((unsigned)bin < (unsigned)p.nbins) {
              float pv = pw[NC / 2 + L];
              if (partner_cur) pv += pw[NC / 2 + L + POFF];
              if (p.win) pv *= wl[NC / 2];
              atomicAdd(&hsum[bin], (double)(pv * wf));
              if constexpr (HELM) {
                float pc = cimg[NC / 2 + L];
                if (partner_cur) pc += cimg[NC / 2 + L + CIMG];
                if (p.win) pc *= wl[NC / 2];
                atomicAdd(&hsumc[bin], (double)(pc * wf));
              }
              if constexpr (COUNT) atomicAdd(&hcnt[bin], w);
            }
          }
        }
      } else if (live_cur) {
        const double k2y = k2y_cur, k2z = k2z_cur;
        const unsigned w = wz_cur;
        const double wd = (double)w * (double)wyz_cur;
        const int kx0 = l * RL + (rev ? RL - 1 : 0);     // kx index of the chunk's first element in walking order
        // walk the chunk in the direction of non-decreasing |kx| (k2x was loaded that way)
        const float* mine = pw + l * (RL + 1) + (rev ? RL - 1 : 0);
        const int step = rev ? -1 : 1;
        // shell of the first element: thr[cur] <= s < thr[cur+1], cur = -1 / nbins outside
        double s = (k2x[0] + k2y) + k2z;
        int cur = (int)((sqrtf((float)s) - p.edge0) * p.inv_spacing);
        cur = min(max(cur, 0), p.nbins - 1);
        while (cur > 0 && s < thr[cur]) --cur;
        while (cur < p.nbins - 1 && s >= thr[cur + 1]) ++cur;
        if (s < thr[cur]) cur = -1;
        else if (s >= thr[cur + 1]) cur = p.nbins;
        double hi = (cur < p.nbins) ? thr[cur + 1] : INFINITY;
        double lo = (cur >= 0) ? thr[cur] : -INFINITY;
        double acc = 0.0, accc = 0.0;
        unsigned cnt = 0;
        const float* minec = cimg + l * (RL + 1) + (rev ? RL - 1 : 0);   // (HELM)
        auto flush = [&]() {   // one LDS atomic per (lane, shell) run
          if (cur >= 0 && cur < p.nbins) {
            atomicAdd(&hsum[cur], acc * wd);
            if constexpr (HELM) atomicAdd(&hsumc[cur], accc * wd);
            if constexpr (COUNT) atomicAdd(&hcnt[cur], cnt * w);
          }
          acc = 0.0;
          if constexpr (HELM) accc = 0.0;
          cnt = 0;
        };
#pragma unroll
        for (int i = 0; i < RL; ++i) {
          // s = (kx*kx + ky*ky) + kz*kz with numpy's rounding (the table holds fl(k*k))
          s = (k2x[i] + k2y) + k2z;
          while (s >= hi) {   // moved outwards to the next shell (the usual direction)
            flush();
            ++cur;
            lo = hi;
            hi = (cur < p.nbins) ? thr[cur + 1] : INFINITY;
          }
          while (s < lo) {    // only for chunks that are not monotone in |kx| (N = 16)
            flush();
            --cur;
            hi = lo;
            lo = (cur >= 0) ? thr[cur] : -INFINITY;
          }
          acc += (double)(p.win ? mine[i * step] * wl[kx0 + i * step] : mine[i * step]);
          if constexpr (HELM) accc += (double)(p.win ? minec[i * step] * wl[kx0 + i * step] : minec[i * step]);
          ++cnt;
        }
        flush();
      }
    }
    if constexpr (MODE != 0) {
      if (tile + gridDim.x < ntiles) {
        locate_line(tile + gridDim.x);
        load_line(v, 0, l);
      }
    }
  }
  if constexpr (MODE == 0) {
    // Per-workgroup partial shell sums go out with plain stores; reduce_partials adds them
    // up.  (Hundreds of workgroups doing float64 atomics on the same few cache lines of
    // psum serialise at the memory side and cost as much as the whole transform.)
    __syncthreads();
    double* ps = p.part_sum + (size_t)blockIdx.x * p.nbins;
    unsigned* pc = p.part_cnt + (size_t)blockIdx.x * p.nbins;
    for (int i = tid; i < p.nbins; i += NT) {
      ps[i] = hsum[i];
      if constexpr (HELM) p.part_sumc[(size_t)blockIdx.x * p.nbins + i] = hsumc[i];
      if constexpr (COUNT) pc[i] = hcnt[i];
    }
  }
}

__global__ void __launch_bounds__(256)
    reduce_partials(const double* __restrict__ part_sum, const unsigned* __restrict__ part_cnt, int nparts,
                    int nbins, double* __restrict__ psum, unsigned long long* __restrict__ nsample) {
  // grid = (bins / 256, groups): block (., g) sums a slice of the partials for 256 bins
  // and adds it with one atomic per bin (only gridDim.y adders per address)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nbins) return;
  const int per = (nparts + gridDim.y - 1) / gridDim.y;
  const int w0 = blockIdx.y * per, w1 = min(w0 + per, nparts);
  double s = 0.0;
  unsigned long long c = 0;
  for (int w = w0; w < w1; ++w) {
    s += part_sum[(size_t)w * nbins + i];
    if (part_cnt) c += part_cnt[(size_t)w * nbins + i];
  }
  if (s != 0.0) atomicAdd(&psum[i], s);
  if (part_cnt && c) atomicAdd(&nsample[i], c);
}

template <int NC, int MODE, bool COUNT = false, bool HELM = false, bool REALB = false>
int launch_x(vps_ctx* ctx, const XParams& p_in, int fast = 0) {   // fast: 0 general shell walk, 1 mirrored kx (float64), 2 integer shells
  static_assert(!HELM || MODE == 0, "the Helmholtz decomposition is a binning variant");
  static_assert(!REALB || (MODE == 0 && !HELM), "the signed binning is a one-component binning variant");
  constexpr bool NOSEG = REALB || MODE == 5;   // whole lines only: no segment variants are built for them (fft_x_impl refuses)
  XParams p = p_in;
  constexpr int T = xpass_T<NC>();
  typedef PlanInfo<NC> PI;
  if (!(MODE == 0 && NC >= 32)) fast = 0;
  const bool seg = p.seglen != NC;
  const bool twreg = fast == 2 && x_twreg<NC, 2, false>();
  size_t lds = ((twreg ? ((PI::TW1 + 1) & ~1) : PI::TWL) + (size_t)T * PI::PITCH) * sizeof(cf);
  if (MODE == 0) lds += (fast == 2 ? (size_t)((p.nbins + 3) & ~1) * sizeof(unsigned) : (size_t)(p.nbins + 2) * sizeof(double)) +
                        (size_t)p.nbins * sizeof(double) + (COUNT ? (size_t)p.nbins * sizeof(unsigned) : 0) +
                        (p.win ? (size_t)NC * sizeof(float) : 0);
  if (HELM) lds += (size_t)p.nbins * sizeof(double) + (size_t)T * x_cimg_pitch<NC>(fast != 0) * sizeof(float);
  if (lds > ctx->lds_per_cu) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "x pass needs %zu B LDS", lds);
  if (seg && x_seg_min_len<NC>() > 1 && (p.seg_shift < 0 || p.seglen < x_seg_min_len<NC>()))   // (callers check vps_x_max_ranks first)
    return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "x pass: lines of %d points in segments of %d (more than %d ranks)", NC, p.seglen,
                    NC / x_seg_min_len<NC>());
  if (NOSEG && seg) return vps_fail(ctx, VPS_ERR_ARG, "x pass: this mode takes whole lines (nseg = 1)");
  auto kern = fft_x_pass<NC, T, MODE, false, COUNT, 0, HELM, REALB>;
  if constexpr (!NOSEG) {
    if (seg) kern = fft_x_pass<NC, T, MODE, true, COUNT, 0, HELM>;
  }
  if constexpr (MODE == 0 && NC >= 32) {
    if (fast == 1) kern = fft_x_pass<NC, T, MODE, false, COUNT, 1, HELM, REALB>;
    if (fast == 2) kern = fft_x_pass<NC, T, MODE, false, COUNT, 2, HELM, REALB>;
    if constexpr (!NOSEG) {
      if (fast == 1 && seg) kern = fft_x_pass<NC, T, MODE, true, COUNT, 1, HELM>;
      if (fast == 2 && seg) kern = fft_x_pass<NC, T, MODE, true, COUNT, 2, HELM>;
    }
  }
  if (lds > 64 * 1024)
    VPS_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const long long ntiles = (p.nlines + T - 1) / T;
  long long per_cu = (long long)(ctx->lds_per_cu / (lds ? lds : 1));
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 8) per_cu = 8;
  {
    const long long want = (long long)vps_option("x_wg_per_cu", 0);
    if (want >= 1 && want < per_cu) per_cu = want;
  }
  long long grid = (long long)ctx->num_cu * per_cu;
  if (grid > ntiles) grid = ntiles;
  if (grid < 1) return VPS_OK;
  if (MODE == 0) {
    const size_t need = (size_t)grid * p.nbins * ((HELM ? 2 : 1) * sizeof(double) + sizeof(unsigned));
    if (need > ctx->xpart_cap) {
      VPS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
      if (ctx->d_xpart) VPS_HIP_CHECK(ctx, hipFree(ctx->d_xpart));
      ctx->d_xpart = nullptr;
      ctx->xpart_cap = 0;
      VPS_HIP_CHECK(ctx, hipMalloc(&ctx->d_xpart, need));
      ctx->xpart_cap = need;
    }
    p.part_sum = reinterpret_cast<double*>(ctx->d_xpart);
    p.part_sumc = HELM ? p.part_sum + (size_t)grid * p.nbins : nullptr;
    p.part_cnt = reinterpret_cast<unsigned*>(p.part_sum + (size_t)grid * p.nbins * (HELM ? 2 : 1));
  }
  {
    vps_launch_timer tm(ctx, VPS_K_FFT_X);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(T * PI::L), lds, ctx->stream, p);
    if (MODE == 0)
      hipLaunchKernelGGL(reduce_partials, dim3((unsigned)((p.nbins + 255) / 256), grid >= 64 ? 32u : 1u),
                         dim3(256), 0, ctx->stream,
                         p.part_sum, COUNT ? p.part_cnt : nullptr, (int)grid, p.nbins, p.psum, p.nsample);
    if (HELM)
      hipLaunchKernelGGL(reduce_partials, dim3((unsigned)((p.nbins + 255) / 256), grid >= 64 ? 32u : 1u),
                         dim3(256), 0, ctx->stream, p.part_sumc, nullptr, (int)grid, p.nbins, p.psumc, nullptr);
  }
  VPS_HIP_CHECK(ctx, hipGetLastError());
  return VPS_OK;
}

}  // namespace
