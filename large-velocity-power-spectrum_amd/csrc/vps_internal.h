// Internal declarations shared by the translation units of libvps_hip.so.
// Not part of the ABI (that is include/vps_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/vps_hip.h"

struct vps_timed_launch {
  int kind;
  hipEvent_t start, stop;
};

struct vps_fft_tables {
  float2* tw_stage = nullptr;  // per-stage LDS twiddle image for complex length NC
  float2* tw_r2c = nullptr;    // exp(-2 pi i k / (2 NC)), k < NC  (real length 2 NC)
};

struct vps_comm;   // comm.hip: RCCL communicator, communication stream, events

struct vps_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_switch = nullptr;   // vps_set_stream: recorded on the stream that is left, waited for by the one that follows
  char err[512] = {0};
  int num_cu = 256;
  size_t lds_per_cu = 160 * 1024;
  size_t lds_per_block = 64 * 1024;   // hipDeviceAttributeMaxSharedMemoryPerBlock, queried once (vps_create)

  std::map<int, vps_fft_tables> fft_tables;  // keyed by complex length NC

  // binning tables (vps_set_binning)
  int bin_N = 0;
  int nbins = 0;
  double* d_k2 = nullptr;   // [N]
  double* d_thr = nullptr;  // [nbins+1]
  double edge0 = 0.0, inv_spacing = 0.0;
  bool bin_fast = false;    // k2 table symmetric and monotone: mirrored-kx binning is valid
  // integer shells (fft_xpass.h: FASTMODE 2): k2[i] = i^2 k2[1] to rounding and no threshold within 1e-9 of an integer multiple of
  // k2[1] -- then nthr[b] = ceil(thr[b] / k2[1]) decides every mode exactly like the float64 comparison
  bool bin_int = false;
  unsigned* d_nthr = nullptr;   // [nbins + 1]
  unsigned bin_nmax = 0;        // nthr[nbins]
  float bin_kf = 0.f;           // sqrt(k2[1])
  std::vector<double> h_k2, h_thr;  // host copies, to skip re-uploading identical tables

  // y-pass store cut for binning-only consumers (vps_set_bin_only): kcut[kz] = largest |ky| index whose modes can still reach
  // a shell, rounded up to the x pass's tile granularity; -1: none
  int* d_kcut = nullptr;
  std::vector<int> h_kcut;   // host copy (row packing of the chunked exchange)
  // plane tables of the chunked exchange for one (N, G, nchunks, packed): per chunk and plane slot j {first row, kc} (int2 on
  // the device) and the rows per destination block of every chunk; rebuilt on demand, dropped by vps_set_binning
  struct {
    int N = 0, G = 0, C = 0, packed = -1;
    void* d_tab = nullptr;
    std::vector<long long> rows;
  } ypack;
  bool bin_only = false;

  // 1 / W(k)^2 per axis index of the mass-assignment window (vps_set_window); NULL: no deconvolution
  float* d_win = nullptr;
  int win_N = 0;
  std::vector<float> h_win;

  // per-workgroup partial shell sums of the x pass
  void* d_xpart = nullptr;
  size_t xpart_cap = 0;

  // small device scratch for the NN lattice axes
  double* d_axes = nullptr;
  size_t axes_cap = 0;

  // exponent alpha of the density-weighted velocity rho^alpha v (vps_set_density_weight); NaN: never set
  double weight_alpha = __builtin_nan("");

  vps_comm* comm = nullptr;      // vps_comm_create

  unsigned nn_open_points = 0;   // diagnostics: lattice points the last NN scatter pass left to the exact fallback
  long long nn_last[4] = {-1, 0, 0, -1};   // vps_nn_last_search: kind, tiles, per-tile radii precomputed, open points (-1: not read)

  bool timing = false;
  std::vector<vps_timed_launch> launches;
  std::vector<hipEvent_t> event_pool;
};

int vps_fail(vps_ctx* ctx, int code, const char* fmt, ...);
// Tuning / test switches set by the host through vps_set_option (process-wide; the library never reads the environment).
double vps_option(const char* name, double dflt);

// VPS_WEIGHTED_VELOCITY needs an exponent on the context and takes neither VPS_FLAG_SHARE_ENERGY nor
// VPS_FLAG_REFERENCE_MOMENTUM_BUG: VPS_ERR_ARG, checked at the entry points before anything is enqueued (api.hip).
// The scalar density quantities go through the same check: VPS_DENSITY needs the exponent too, and VPS_DENSITY /
// VPS_LOG_DENSITY take none of VPS_FLAG_COMPONENTS, VPS_FLAG_SHARE_ENERGY, VPS_FLAG_REFERENCE_MOMENTUM_BUG.
int vps_check_weighted(vps_ctx* ctx, const char* who, int quantity, int flags);
// The second-moment quantities (VPS_TOTAL_ENERGY, VPS_SUBGRID_ENERGY, VPS_DISPERSION) are formed by vps_deposit_field alone.
// An entry point that cannot form them calls this first: VPS_ERR_ARG with the quantity's name, its number and `why`, before
// anything is enqueued; VPS_OK for every other code.
int vps_refuse_second_moment(vps_ctx* ctx, const char* who, int quantity, const char* why);
const char* vps_second_moment_name(int quantity);
// The velocity-gradient quantities (VPS_DIVERGENCE, VPS_VORTICITY, VPS_STRAIN_RATE) are formed by vps_field_algebra_out alone,
// from a whole grid; every other entry point that takes a quantity refuses them the same way.
int vps_refuse_grid_only(vps_ctx* ctx, const char* who, int quantity, const char* why);
const char* vps_gradient_name(int quantity);
// gradient.hip: the stencil launch behind vps_field_algebra_out for those codes.  chans: [>= 3][N^3] velocity channels, out:
// [vps_quantity_channels(quantity)][N^3], h = 1 / (2 Lcell) in float32; the caller has checked everything (N even, >= 4).
void vps_gradient_launch(vps_ctx* ctx, int quantity, int N, float h, const float* chans, float* out);
// The box-filter quantities (VPS_FILTERED_VM, VPS_FILTERED_STRESS) are formed by vps_field_algebra_out alone as well, and
// vps_refuse_grid_only refuses them with the gradient codes: a box of cells is as little a per-cell quantity as a difference.
const char* vps_filter_name(int quantity);
// filter.hip: the launch behind vps_field_algebra_out for those codes.  chans: [4][N^3] = [u, mass], out:
// [vps_quantity_channels(quantity)][N^3], half-width 1 <= m <= VPS_FILTER_MAX_HALF_WIDTH with 2m + 1 <= N,
// c = 1 / (2m+1)^3 in float32; the caller has checked everything (N even, >= 4).
#define VPS_FILTER_MAX_HALF_WIDTH 8   // what the kernel's LDS plan holds: a region of (16 + 2m) x (64 + 2m) cells, four channels
void vps_filter_launch(vps_ctx* ctx, int quantity, int N, int m, float c, const float* chans, float* out);

// Every entry point of the C ABI runs with the context's device current and restores the caller's
// on return: the library allocates (tables, partial sums, lattice axes) and launches on streams
// that belong to ctx->device, whatever device the calling thread had selected.
struct vps_device_guard {
  int prev = -1;
  explicit vps_device_guard(const vps_ctx* ctx) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != ctx->device && hipSetDevice(ctx->device) == hipSuccess) prev = cur;
  }
  ~vps_device_guard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define VPS_ENTER(ctx)                 \
  if (!(ctx)) return VPS_ERR_ARG;      \
  vps_device_guard vps_guard_(ctx)

#define VPS_HIP_CHECK(ctx, expr)                                                   \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess)                                                          \
      return vps_fail((ctx), VPS_ERR_HIP, "%s failed: %s (%s:%d)", #expr,          \
                      hipGetErrorString(_e), __FILE__, __LINE__);                  \
  } while (0)

// Brackets a kernel launch with events when ctx->timing is on.
struct vps_launch_timer {
  vps_ctx* ctx;
  int idx = -1;
  hipStream_t stream;
  vps_launch_timer(vps_ctx* c, int kind, hipStream_t on = nullptr);   // on: the stream the interval lives on (default: the context's)
  ~vps_launch_timer();
};

// The scalar density launches of the pencil kernel (VPS_DENSITY, VPS_LOG_DENSITY): one accumulation round of rho, then the
// per-cell function of it (quantity.h: vps_rho_scalar_nz) -- none (alpha = 1: the cell total as it is), rho^sexp, or ln rho.
enum { PENCIL_SCALAR_NONE = 0, PENCIL_SCALAR_RHO = 1, PENCIL_SCALAR_POW = 2, PENCIL_SCALAR_LOG = 3 };

// fft.hip
int vps_fft_get_tables(vps_ctx* ctx, int NC, vps_fft_tables* out);
// most slab ranks G whose segmented x pass (segments of N / G points) exists for lines of N points: 16 for N = 1024, 2048,
// 4096, else N (include/vps_hip.h: vps_fft_x_bin_chunk); an internal symbol, not part of the exported ABI
__attribute__((visibility("hidden"))) int vps_x_max_ranks(int N);
void vps_fft_free_tables(vps_ctx* ctx);
// fused deposit -> z pass ("pencil" path): records sorted by pencil -> ncomp half spectra
int vps_pencil_tp(int N);
bool vps_pencil_supported(vps_ctx* ctx, int N);
// What a pencil launch forms from the [rho v, rho] records: filled from (quantity, flags) in ONE place (deposit.hip:
// pencil_quantity), copied member by member into the kernel argument (fft_params.h: PencilParams, whose layout does not change).
struct PencilQuantity {
  int ncomp = 3;
  int chan[3] = {0, 1, 2};             // record channel (0..2) feeding component c
  int divide = 0, energy = 0;          // PencilParams
  int with_energy = 0;                 // VPS_FLAG_SHARE_ENERGY: 1 the momentum launch that also makes the energy field, 2 the energy call that uses it
  int weighted = 0;                    // q * rho^wexp
  float wexp = 0.f;
  int scalar = PENCIL_SCALAR_NONE;
  float sexp = 1.f;
};
// side: one float per record (scratch of the kernel: what it keeps per record when a bucket outgrows its registers)
int vps_fft_pencil_zy(vps_ctx* ctx, int N, int nx, const unsigned* records, const unsigned* start, float* side,
                      const PencilQuantity& q, float vol, void* spec_dev, void* nyq_dev, void* bwork_dev);

// ---- LDS floating-point accumulation ---------------------------------------------------------
// gfx950 executes ds_add_f32 far below the LDS rate (measured: about one lane every two clocks per
// CU), while its integer LDS atomics run at bank speed.  So a float add is first tried as ONE
// compare-and-swap on the bit pattern (plain read, add, ds_cmpst_rtn): it succeeds unless another
// lane or wave changed the word in between, which is rare when the lanes of a wave hit different
// words.  Only the losers fall back to the native atomic -- many particles in one cell therefore
// cost what they cost before, never a retry storm.  Same sums (in some order) either way.
// Pencil kernel 0.57 -> 0.49 ms at 512^3 / 1e7 particles.
#if defined(__HIPCC__)
// `crowded` (uniform over the caller's workgroup): expect many adds per word -- skip the attempt.
__device__ __forceinline__ void vps_lds_add(float* addr, float v, bool crowded = false) {
  if (crowded) {
    atomicAdd(addr, v);
    return;
  }
  unsigned* a = reinterpret_cast<unsigned*>(addr);
  const unsigned assumed = *a;
  if (atomicCAS(a, assumed, __float_as_uint(__uint_as_float(assumed) + v)) != assumed) atomicAdd(addr, v);
}
#endif
