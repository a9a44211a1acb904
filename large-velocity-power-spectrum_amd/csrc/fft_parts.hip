// The FFT's kernels, one family of line lengths per object.
// Every line length instantiates ~20 kernels, and 21 lengths in one translation unit take minutes to compile.  The build
// therefore compiles this file once per length FAMILY (-DVPS_FFT_PART=0..3): each object defines FftPart<k> (fft_params.h),
// whose entry points instantiate the launchers of its own lengths and answer VPS_PART_NOT_MINE for every other.  Without
// the macro (tools/build_variant.sh fft, single-object builds) one object defines all four.
#include "fft_transpose.h"
#include "fft_pencil.h"
#include "fft_xpass.h"

namespace {

constexpr int family_of(int NC) {
  switch (NC) {
    case 8: case 16: case 32: case 64: case 128: case 256: return 0;
    case 512: case 1024: case 2048: case 4096: return 1;
    case 48: case 96: case 192: case 384: case 768: case 1536: return 2;
    case 125: case 250: case 500: case 1000: case 2000: return 3;
    default: return -1;
  }
}

}  // namespace

// (inside a member of FftPart<PART>: the call is instantiated for this family's lengths only)
#define VPS_CASE(N, CALL)                    \
  case N:                                    \
    if constexpr (family_of(N) == PART) {    \
      constexpr int NC_ = N;                 \
      CALL;                                  \
    } else {                                 \
      rc = VPS_PART_NOT_MINE;                \
    }                                        \
    break;
#define VPS_DISPATCH_NC(NCVAL, CALL)                                                                                          \
  switch (NCVAL) {                                                                                                            \
    VPS_CASE(8, CALL) VPS_CASE(16, CALL) VPS_CASE(32, CALL) VPS_CASE(64, CALL) VPS_CASE(128, CALL) VPS_CASE(256, CALL)        \
    VPS_CASE(512, CALL) VPS_CASE(1024, CALL) VPS_CASE(2048, CALL) VPS_CASE(4096, CALL)                                        \
    VPS_CASE(48, CALL) VPS_CASE(96, CALL) VPS_CASE(192, CALL) VPS_CASE(384, CALL) VPS_CASE(768, CALL) VPS_CASE(1536, CALL)    \
    VPS_CASE(125, CALL) VPS_CASE(250, CALL) VPS_CASE(500, CALL) VPS_CASE(1000, CALL) VPS_CASE(2000, CALL)                     \
    default: rc = VPS_PART_NOT_MINE;                                                                                          \
  }
// packed-real lines of the grids the pencil path takes (64 <= N <= 4096, no 2^a 5^b sizes)
#define VPS_DISPATCH_PENCIL(NCVAL, CALL)                                                              \
  switch (NCVAL) {                                                                                    \
    VPS_CASE(32, CALL) VPS_CASE(64, CALL) VPS_CASE(128, CALL) VPS_CASE(256, CALL)                     \
    VPS_CASE(512, CALL) VPS_CASE(1024, CALL) VPS_CASE(2048, CALL)                                     \
    VPS_CASE(96, CALL) VPS_CASE(192, CALL) VPS_CASE(384, CALL) VPS_CASE(768, CALL)                    \
    default: rc = VPS_PART_NOT_MINE;                                                                  \
  }

template <int PART>
int FftPart<PART>::tw(int NC, std::vector<cf>* st) {
  int rc = VPS_OK;
  VPS_DISPATCH_NC(NC, build_stage_tw<NC_>(*st));
  return rc;
}

template <int PART>
int FftPart<PART>::transpose(vps_ctx* ctx, int NC, int real, const PassParams& p, int kind) {
  int rc = VPS_OK;
  if (real) {
    VPS_DISPATCH_NC(NC, (rc = launch_transpose<NC_, true>(ctx, p, kind)));
  } else {
    VPS_DISPATCH_NC(NC, (rc = launch_transpose<NC_, false>(ctx, p, kind)));
  }
  return rc;
}

template <int PART>
int FftPart<PART>::x(vps_ctx* ctx, int NC, int mode, int count, const XParams& p, int fast, int helm) {
  int rc = VPS_OK;
  if (helm) {   // (binning only: fft_x_impl checks)
    if (count) {
      VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 0, true, true>(ctx, p, fast)));
    } else {
      VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 0, false, true>(ctx, p, fast)));
    }
  } else if (mode == 6) {   // the signed binning of Re F (vps_fft_x modes 6 / 7)
    if (count) {
      VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 0, true, false, true>(ctx, p, fast)));
    } else {
      VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 0, false, false, true>(ctx, p, fast)));
    }
  } else if (mode == 5) {
    VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 5>(ctx, p)));
  } else if (mode == 0 && count) {
    VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 0, true>(ctx, p, fast)));
  } else if (mode == 0) {
    VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 0, false>(ctx, p, fast)));
  } else if (mode == 1) {
    VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 1>(ctx, p)));
  } else if (mode == 2) {
    VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 2>(ctx, p)));
  } else {
    VPS_DISPATCH_NC(NC, (rc = launch_x<NC_, 4>(ctx, p)));
  }
  return rc;
}

template <int PART>
long long FftPart<PART>::pencil_lds(int NC) {
  long long rc = 0;
  long long lds = -1;
  VPS_DISPATCH_PENCIL(NC, (lds = (long long)pencil_lds_bytes<NC_>()));
  return rc == 0 ? lds : (long long)VPS_PART_NOT_MINE;
}

template <int PART>
int FftPart<PART>::pencil(vps_ctx* ctx, int NC, const PencilParams& p, long long npencils) {
  int rc = VPS_OK;
  VPS_DISPATCH_PENCIL(NC, (rc = launch_pencil<NC_>(ctx, p, npencils)));
  return rc;
}

#if defined(VPS_FFT_PART) && VPS_FFT_PART >= 0
template struct FftPart<VPS_FFT_PART>;
#else   // (no macro, or -1: every family in this object)
template struct FftPart<0>;
template struct FftPart<1>;
template struct FftPart<2>;
template struct FftPart<3>;
#endif
