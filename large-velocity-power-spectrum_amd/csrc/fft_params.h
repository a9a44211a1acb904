// What crosses the boundary between the FFT's host API (fft.hip) and the units that hold its kernels (fft_parts.hip, compiled
// once per family of line lengths): the kernel arguments of the three passes and the entry points of a family unit.
// No kernel is defined here.
#pragma once
#include "vps_internal.h"

typedef float2 cf;

// ---- transposing passes (fft_transpose.h) ----
struct PassParams {
  const void* in;
  const void* in_w;          // REAL passes: optional second real field of the same layout; the line transformed is in * in_w
                             // (momentum p_c = v_c * mass of a gridded field without a separate algebra pass)
  void* out;
  void* out_nyq;
  long long in_sa, in_sb;  // input strides of the tile axis a and batch axis b (elements)
  long long out_ob, out_ok;  // output strides (complex elements): out[b*ob + k*ok + a]
  long long nyq_ob;          // out_nyq[b*nyq_ob + a]
  int A, B;                  // extent of tile axis / batch axis
  const cf* tw_stage;
  const cf* tw_r2c;
  // Chunked slab exchange (vps_fft_y): the B batches of a launch are `bg`-row groups, one per destination rank --
  // launch batch b reads input batch (b / bg) * bg_in + b_off + b % bg and its output starts bg_gap elements later per
  // group (room for the Nyquist rows that ride behind a destination's last chunk).  bg = 0: plain batches.
  int bg, b_off;
  long long bg_in, bg_gap;
  // the Nyquist-plane launch (B = 1): output row k moves by (k / kg) * kg_gap elements (kg = 0: none), so that each
  // destination's rows land behind that destination's block
  int kg;
  long long kg_gap;
  // binning-only consumers (vps_set_bin_only): rows ky with min(ky, NC - ky) > kcut[kz] are not stored -- every mode
  // there lies beyond the last shell edge and the binning x pass does not read them.  kz = kz_fixed, or the input batch
  const int* kcut;
  int kz_fixed;
  // chunked exchange (vps_fft_y): ptab[j] = {first row, kc} of the j-th plane of every destination's block (j = launch batch %
  // bg) -- the plane keeps the 2 kc + 1 rows |ky| <= kc (kc >= its kcut; -1: all NC rows): row ky at position ky, row NC - i at
  // position 2 kc + 1 - i behind the block's first row.  Launch batch b reads input batch
  // b_off + (b / bg) * bg_in + (b % bg) * bg_step.  NULL: plain planes of NC rows, out_ob apart.
  const int2* ptab = nullptr;
  int bg_step = 1;
};

// ---- fused deposit + z pass (fft_pencil.h) ----
struct PencilParams {
  const unsigned* records;   // (1 + 4) 32-bit words per particle, sorted by pencil
  const unsigned* start;     // [npencils + 1]
  int N, nx, nby;            // grid, slab rows, pencils per x row (N / TP)
  unsigned npencils;         // pencils of the launch
  int ncomp;
  int chan[3];               // record channel (0..2) feeding component c
  int divide;                // 1: v = q / rho (0 where rho == 0);  0: p = q * vol
                             // (divide = 1 with `weighted`: w = q * rho^wexp, the density-weighted velocity rho^alpha v)
  int energy;                // 1: ONE output field E = vol * sum_c q_c^2 / rho (= mass * |v|^2, interp.py:546)
  int with_energy;           // momentum launch (divide = 0, three components) that ALSO writes the energy field as out[3]: the
                             // cell totals of rho v_c its rounds accumulate are what E is made of -- one more round (rho) and
                             // one more transform instead of a launch of its own with four rounds and a start of its own
  float vol;
  float* side;               // [records] one float per record, for the records a workgroup cannot keep in registers
  cf* out[4];                // B_c[x][kz][y]
  cf* nyq[4];                // BN_c[x][y]
  const cf* tw_stage;
  const cf* tw_r2c;
  // density-weighted velocity (VPS_WEIGHTED_VELOCITY; last, so that no other member moves): the WEIGHTED instantiation keeps
  // rho^wexp, wexp = alpha - 1, per record where the velocity form keeps 1 / rho
  int weighted;
  float wexp;
  // scalar density quantities (VPS_DENSITY, VPS_LOG_DENSITY; the DENSITY instantiation): PENCIL_SCALAR_RHO the cell total as it
  // is, PENCIL_SCALAR_POW rho^sexp, PENCIL_SCALAR_LOG ln rho
  int scalar;
  float sexp;
};

// ---- x pass (fft_xpass.h) ----
struct XParams {
  const cf* in;            // component 0
  const cf* in1;           // components 1, 2 of a vector field (binning modes, ncomp > 1)
  const cf* in2;
  int ncomp;
  cf* out;
  long long nlines, line0;
  int N, kz0;
  int seglen, seg_shift;  // segment length and its log2 (-1: not a power of two)
  long long seg_stride;
  const cf* tw_stage;
  const double* k2;
  const double* thr;
  const float* win;        // 1 / W^2 per axis index (vps_set_window) or NULL
  int nbins;
  float edge0, inv_spacing;
  double* psum;
  unsigned long long* nsample;
  const int2* ptab;   // chunked exchange (vps_fft_x_bin_chunk; NULL otherwise): plane i of the launch starts at row ptab[i].x of a
                      // block and holds the rows |ky| <= ptab[i].y (-1: all N), see PassParams::ptab; its kz is kz0 + i * kz_step
  int kz_step;
  int pair;  // FAST path: tiles pair ky with N-ky (needs whole ky ranges: line0, nlines multiples of N)
  // integer shells (FAST == 2; vps_set_binning has checked that they reproduce the float64 comparison bit for bit): a mode
  // belongs to shell b iff nthr[b] <= ix^2 + iy^2 + iz^2 < nthr[b + 1] (signed mode indices); nmax = nthr[nbins]; kf = 2 pi / L
  const unsigned* nthr;
  unsigned nmax;
  float kf;
  double* part_sum;    // [grid][nbins] per-workgroup partial shell sums
  unsigned* part_cnt;  // [grid][nbins] per-workgroup partial shell counts
  // Helmholtz decomposition (HELM, ncomp = 3): shell sums of |k'.F|^2 / |k'|^2 (vps_fft_x_bin_helmholtz) and their partials
  double* psumc;
  double* part_sumc;
};

// ---- one family of line lengths (fft_parts.hip) ----
// The library holds FftPart<0> .. FftPart<3>, each defined by the unit compiled for that family.  NC is the complex line
// length; a family that does not hold it returns VPS_PART_NOT_MINE and the caller (fft.hip: try_parts) asks the next one.
#define VPS_PART_NOT_MINE (-12345)
template <int PART>
struct FftPart {
  static int tw(int NC, std::vector<cf>* st);   // host image of the stage twiddles
  static int transpose(vps_ctx* ctx, int NC, int real, const PassParams& p, int kind);
  static int x(vps_ctx* ctx, int NC, int mode, int count, const XParams& p, int fast, int helm);
  static long long pencil_lds(int NC);          // LDS bytes of the pencil kernel
  static int pencil(vps_ctx* ctx, int NC, const PencilParams& p, long long npencils);
};
