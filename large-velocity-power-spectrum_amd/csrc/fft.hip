// 3-D real-to-complex FFT as three batched Stockham line passes, hand-written for
// gfx950 (wave64, 160 KiB LDS/CU), with |F|^2 + spherical-shell binning fused into
// the last pass.  No rocFFT/hipFFT.
//
// Replaces, on the device, the reference's pyFFTW calls and numpy histogram passes:
//   _vector_power / _scalar_power        vpower/interp.py:1372-1387, 1408-1421
//   FFTW_power / FFTW_vector_power       scripts/parallel_optimized.py:92-141
//   _pair_power + _hist_sample           vpower/interp.py:1440-1482
//   pair_power + hist_sample             scripts/parallel_optimized.py:145-190
//
// Data layout (all complex64 unless noted), N = cells per axis, nx = local x rows:
//   input      R[x][y][z]        float32, z contiguous
//   z pass  -> B[x][kz][y]       kz < N/2, y contiguous   (+ Nyquist plane BN[x][y])
//   y pass  -> C[kz][ky][x]      x contiguous             (+ CN[ky][x])
//   x pass  -> lines C[kz][ky][:] transformed in registers and binned (or written).
// Every pass reads whole contiguous lines and writes T-element (T*8 byte) contiguous
// segments of the next layout, so no pass ever does element-strided HBM access.
//
// One line of NC complex points is transformed by L lanes holding RL = NC/L points
// each; radix-8/16 butterflies run in registers and the stages exchange data through
// a padded per-line LDS buffer (Stockham autosort: stage inputs are always read at
// stride NC/R, outputs written at expand(j)+r*Ns).
//
// This unit is the host side: argument checks, tables, the layout of the chunked slab exchange and every FFT entry point
// of the C ABI.  It holds no kernel.  The kernels live in fft_transpose.h, fft_pencil.h and fft_xpass.h, built from
// fft_dft.h / fft_line.h and compiled by fft_parts.hip once per family of line lengths; fft_params.h is the interface.
#include <algorithm>
#include <cstdlib>

#include "fft_line.h"   // (constexpr rules of a line length only)

// The family unit that holds the length answers; the others return VPS_PART_NOT_MINE.
template <class F>
static long long try_parts(F call) {
  long long r = call(FftPart<0>());
  if (r == VPS_PART_NOT_MINE) r = call(FftPart<1>());
  if (r == VPS_PART_NOT_MINE) r = call(FftPart<2>());
  if (r == VPS_PART_NOT_MINE) r = call(FftPart<3>());
  return r;
}
static int routed(vps_ctx* ctx, int NC, long long r, const char* miss = "unsupported FFT length %d") {
  return r != VPS_PART_NOT_MINE ? (int)r : vps_fail(ctx, VPS_ERR_UNSUPPORTED, miss, NC);
}
static int route_tw(vps_ctx* ctx, int NC, std::vector<cf>* st) {
  return routed(ctx, NC, try_parts([&](auto part) { return part.tw(NC, st); }));
}
static int route_transpose(vps_ctx* ctx, int NC, int real, const PassParams& p, int kind) {
  return routed(ctx, NC, try_parts([&](auto part) { return part.transpose(ctx, NC, real, p, kind); }));
}
static int route_x(vps_ctx* ctx, int NC, int mode, int count, const XParams& p, int fast, int helm) {
  return routed(ctx, NC, try_parts([&](auto part) { return part.x(ctx, NC, mode, count, p, fast, helm); }));
}
static long long route_pencil_lds(int NC) {
  const long long r = try_parts([&](auto part) { return part.pencil_lds(NC); });
  return r != VPS_PART_NOT_MINE ? r : -1;
}
static int route_pencil(vps_ctx* ctx, int NC, const PencilParams& p, long long npencils) {
  return routed(ctx, NC, try_parts([&](auto part) { return part.pencil(ctx, NC, p, npencils); }),
                "pencil path: no kernel for lines of %d points");
}

int vps_fft_get_tables(vps_ctx* ctx, int NC, vps_fft_tables* out) {
  auto it = ctx->fft_tables.find(NC);
  if (it != ctx->fft_tables.end()) {
    *out = it->second;
    return VPS_OK;
  }
  std::vector<cf> st;
  int rc = route_tw(ctx, NC, &st);
  if (rc) return rc;
  std::vector<cf> r2c(NC);
  for (int k = 0; k < NC; ++k) {
    double a = -2.0 * 3.14159265358979323846 * (double)k / (double)(2 * NC);
    r2c[k] = make_float2((float)cos(a), (float)sin(a));
  }
  vps_fft_tables t;
  VPS_HIP_CHECK(ctx, hipMalloc(&t.tw_stage, st.size() * sizeof(cf)));
  VPS_HIP_CHECK(ctx, hipMalloc(&t.tw_r2c, r2c.size() * sizeof(cf)));
  VPS_HIP_CHECK(ctx, hipMemcpy(t.tw_stage, st.data(), st.size() * sizeof(cf), hipMemcpyHostToDevice));
  VPS_HIP_CHECK(ctx, hipMemcpy(t.tw_r2c, r2c.data(), r2c.size() * sizeof(cf), hipMemcpyHostToDevice));
  ctx->fft_tables[NC] = t;
  *out = t;
  return VPS_OK;
}

void vps_fft_free_tables(vps_ctx* ctx) {
  for (auto& kv : ctx->fft_tables) {
    (void)hipFree(kv.second.tw_stage);
    (void)hipFree(kv.second.tw_r2c);
  }
  ctx->fft_tables.clear();
}

int vps_x_max_ranks(int N) { return x_max_segments(N); }

// The one check of N and its message for every entry point that takes any supported grid.
static int check_fft_size(vps_ctx* ctx, int N) {
  if (vps_fft_supported(N)) return VPS_OK;
  return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "N=%d: need a power of two in [16,4096], 96, 192, 384, 768, 1536, 250, 500, 1000 or 2000", N);
}

static int fft_y_of(vps_ctx* ctx, int N, int nx, const cf* B, const cf* BN, void* spec_dev, void* nyq_dev);

extern "C" {

int vps_fft_supported(int N) {
  if (N == 250 || N == 500 || N == 1000 || N == 2000) return 1;   // 2^a 5^b plans (radix 5 / 10 / 20)
  if (N == 96 || N == 192 || N == 384 || N == 768 || N == 1536) return 1;   // 3 * 2^a plans (radix 3 / 6 / 12 / 24)
  return (N >= 16 && N <= 4096 && (N & (N - 1)) == 0) ? 1 : 0;
}

size_t vps_fft_workspace_bytes(int N, int nx) {
  // B[x][kz][y] (kz < N/2) + Nyquist plane BN[x][y]
  return ((size_t)nx * (size_t)(N / 2) * (size_t)N + (size_t)nx * (size_t)N) * sizeof(cf);
}

size_t vps_power_workspace_bytes(int N) {
  // z-pass image + y-pass image (each with its Nyquist plane)
  return 2 * vps_fft_workspace_bytes(N, N);
}

int vps_fft_zy_weighted(vps_ctx* ctx, int N, int nx, const float* field_dev, const float* weight_dev,
                        void* spec_dev, void* nyq_dev, void* work_dev);

int vps_fft_zy(vps_ctx* ctx, int N, int nx, const float* field_dev, void* spec_dev, void* nyq_dev,
               void* work_dev) {
  return vps_fft_zy_weighted(ctx, N, nx, field_dev, nullptr, spec_dev, nyq_dev, work_dev);
}

static int fft_z_of(vps_ctx* ctx, int N, int nx, const float* field_dev, const float* weight_dev, cf* B, cf* BN) {
  const int NH = N / 2;
  vps_fft_tables tz;
  int rc = vps_fft_get_tables(ctx, NH, &tz);
  if (rc) return rc;
  // z pass: lines (a = y, b = x) of R[x][y][:] -> B[x][kz][y], BN[x][y]
  PassParams pz{};
  pz.in = field_dev;
  pz.in_w = weight_dev;
  pz.out = B;
  pz.out_nyq = BN;
  pz.in_sa = N;
  pz.in_sb = (long long)N * N;
  pz.out_ob = (long long)NH * N;
  pz.out_ok = N;
  pz.nyq_ob = N;
  pz.A = N;
  pz.B = nx;
  pz.tw_stage = tz.tw_stage;
  pz.tw_r2c = tz.tw_r2c;
  return route_transpose(ctx, NH, 1, pz, VPS_K_FFT_Z);
}

int vps_fft_zy_weighted(vps_ctx* ctx, int N, int nx, const float* field_dev, const float* weight_dev,
                        void* spec_dev, void* nyq_dev, void* work_dev) {
  VPS_ENTER(ctx);
  if (int bad = check_fft_size(ctx, N)) return bad;
  if (nx < 1 || nx > N) return vps_fail(ctx, VPS_ERR_ARG, "nx=%d out of range", nx);
  if (!field_dev || !spec_dev || !nyq_dev || !work_dev) return vps_fail(ctx, VPS_ERR_ARG, "null buffer");
  cf* B = reinterpret_cast<cf*>(work_dev);
  cf* BN = B + (size_t)nx * (N / 2) * N;
  int rc = fft_z_of(ctx, N, nx, field_dev, weight_dev, B, BN);
  if (rc) return rc;
  // y pass: lines (a = x, b = kz) of B[x][kz][:] -> C[kz][ky][x]; Nyquist plane BN[x][:] -> CN[ky][x]
  return fft_y_of(ctx, N, nx, B, BN, spec_dev, nyq_dev);
}

// ---- the split form for the chunked slab exchange: z pass into an image, y pass one kz chunk at a time ----
size_t vps_fft_zimage_bytes(int N, int nx) { return vps_fft_workspace_bytes(N, nx); }

int vps_fft_z(vps_ctx* ctx, int N, int nx, const float* field_dev, const float* weight_dev, void* zimg_dev) {
  VPS_ENTER(ctx);
  if (!vps_fft_supported(N)) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_fft_z: unsupported N=%d", N);
  if (nx < 1 || nx > N) return vps_fail(ctx, VPS_ERR_ARG, "nx=%d out of range", nx);
  if (!field_dev || !zimg_dev) return vps_fail(ctx, VPS_ERR_ARG, "null buffer");
  cf* B = reinterpret_cast<cf*>(zimg_dev);
  return fft_z_of(ctx, N, nx, field_dev, weight_dev, B, B + (size_t)nx * (N / 2) * N);
}

int64_t vps_fft_y_chunk_elems(int N, int nx, int G, int nchunks, int chunk) {
  if (G < 1 || nchunks < 1 || chunk < 0 || chunk >= nchunks || N % G || (N / 2) % (G * nchunks)) return -1;
  const int64_t nkc = N / 2 / G / nchunks;
  return (int64_t)G * (nkc * N * nx + (chunk == nchunks - 1 ? (int64_t)(N / G) * nx : 0));
}

// ---- layout of the chunked slab exchange --------------------------------------------------------------------------------
// The kz < N/2 planes are cut into `nchunks` bands of G * nkc planes (nkc = N/2/G/nchunks); inside band c the planes are dealt
// out round-robin: slot j of rank h is plane c*G*nkc + j*G + h.  So (a) every rank holds planes of every |kz| -- the same
// share of rows its x passes can skip -- and (b) the j-th planes of all ranks are neighbours in kz and need the same rows to
// within one step of the cut: packed, every destination's block carries, for slot j, the 2 kc_j + 1 rows |ky| <= kc_j with
// kc_j = the largest kcut of the G planes of slot j.  Equal blocks for all destinations, a table of nkc entries per chunk.
static bool ypack_wanted(const vps_ctx* ctx, int N) {
  return ctx->bin_only && ctx->bin_N == N && (int)ctx->h_kcut.size() == N / 2 + 1;
}

// plane table of chunk `chunk` (device) and the rows of one destination's block; (re)built for (N, G, nchunks, packed)
static int ypack_get(vps_ctx* ctx, int N, int G, int nchunks, int chunk, bool packed, const int2** tab, long long* rows) {
  if (G < 1 || nchunks < 1 || N < 2 || (N / 2) % (G * nchunks) || chunk < 0 || chunk >= nchunks)
    return vps_fail(ctx, VPS_ERR_ARG, "chunked exchange: G=%d ranks x %d chunks must divide N/2=%d", G, nchunks, N / 2);
  if (packed && (int)ctx->h_kcut.size() != N / 2 + 1)
    return vps_fail(ctx, VPS_ERR_ARG, "chunked exchange: packed rows need the row cut of vps_set_binning(N=%d)", N);
  const int nkc = N / 2 / G / nchunks;
  auto& y = ctx->ypack;
  if (!(y.N == N && y.G == G && y.C == nchunks && y.packed == (int)packed && y.d_tab)) {
    std::vector<int2> t((size_t)nchunks * nkc);
    y.rows.assign(nchunks, 0);
    for (int c = 0; c < nchunks; ++c) {
      long long r = 0;
      for (int j = 0; j < nkc; ++j) {
        int kc = -1;
        if (packed) {
          kc = 0;
          for (int h = 0; h < G; ++h) kc = std::max(kc, ctx->h_kcut[c * G * nkc + j * G + h]);
          if (2 * kc + 1 >= N) kc = -1;
        }
        t[(size_t)c * nkc + j] = make_int2((int)r, kc);
        r += kc < 0 ? N : 2 * kc + 1;
      }
      y.rows[c] = r;
    }
    VPS_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // (a launch may still read the old table)
    if (y.d_tab) VPS_HIP_CHECK(ctx, hipFree(y.d_tab));
    y.d_tab = nullptr;
    y.N = 0;
    VPS_HIP_CHECK(ctx, hipMalloc(&y.d_tab, t.size() * sizeof(int2)));
    VPS_HIP_CHECK(ctx, hipMemcpy(y.d_tab, t.data(), t.size() * sizeof(int2), hipMemcpyHostToDevice));
    y.N = N; y.G = G; y.C = nchunks; y.packed = (int)packed;
  }
  if (tab) *tab = reinterpret_cast<const int2*>(y.d_tab) + (size_t)chunk * nkc;
  if (rows) *rows = y.rows[chunk];
  return VPS_OK;
}

int vps_fft_y_packed(vps_ctx* ctx, int N) { return ctx && ypack_wanted(ctx, N) ? 1 : 0; }

// A pure size query: the rows of a block follow from the host copy of the row cut; no device table is built or touched
// (ypack_get, which the y / x passes call, keeps its one-entry cache for the launch that follows).
// Returns -1: bad arguments, -2: G x nchunks does not divide N/2 (or G does not divide N), -3: packed without a row cut.
int64_t vps_fft_y_chunk_block(vps_ctx* ctx, int N, int nx, int G, int nchunks, int chunk, int packed) {
  if (!ctx || nx < 1 || N < 2) return -1;
  if (G < 1 || nchunks < 1 || chunk < 0 || chunk >= nchunks) return -1;
  if (N % G || (N / 2) % (G * nchunks)) {
    vps_fail(ctx, VPS_ERR_ARG, "chunked exchange: G=%d ranks x %d chunks must divide N/2=%d (and G divide N)", G, nchunks, N / 2);
    return -2;
  }
  if (packed && (int)ctx->h_kcut.size() != N / 2 + 1) {
    vps_fail(ctx, VPS_ERR_ARG, "chunked exchange: packed rows need the row cut of vps_set_binning(N=%d)", N);
    return -3;
  }
  const int nkc = N / 2 / G / nchunks;
  long long rows = 0;
  for (int j = 0; j < nkc; ++j) {
    int kc = -1;
    if (packed) {
      kc = 0;
      for (int h = 0; h < G; ++h) kc = std::max(kc, ctx->h_kcut[chunk * G * nkc + j * G + h]);
      if (2 * kc + 1 >= N) kc = -1;
    }
    rows += kc < 0 ? N : 2 * kc + 1;
  }
  return rows * nx + (chunk == nchunks - 1 ? (long long)(N / G) * nx : 0);
}

int vps_fft_y(vps_ctx* ctx, int N, int nx, const void* zimg_dev, int G, int nchunks, int chunk, void* out_dev) {
  VPS_ENTER(ctx);
  if (!vps_fft_supported(N)) return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_fft_y: unsupported N=%d", N);
  if (nx < 1 || nx > N || !zimg_dev || !out_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_y: bad nx / null buffer");
  if (vps_fft_y_chunk_elems(N, nx, G, nchunks, chunk) < 0)
    return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_y: G=%d ranks x %d chunks must divide N/2=%d (and G divide N)", G, nchunks, N / 2);
  const int NH = N / 2, nkz = NH / G, nkc = nkz / nchunks, nky = N / G;
  const bool last = chunk == nchunks - 1;
  vps_fft_tables ty;
  int rc = vps_fft_get_tables(ctx, N, &ty);
  if (rc) return rc;
  const cf* B = reinterpret_cast<const cf*>(zimg_dev);
  const cf* BN = B + (size_t)nx * NH * N;
  const int2* tab = nullptr;
  long long rows = 0;   // rows of one destination's block (N per plane when not packed)
  rc = ypack_get(ctx, N, G, nchunks, chunk, ypack_wanted(ctx, N), &tab, &rows);
  if (rc) return rc;
  const long long blk = rows * nx + (last ? (long long)nky * nx : 0);   // one destination's block
  (void)nkz;
  // launch batch b = h nkc + j (destination h, slot j) reads plane chunk G nkc + j G + h and writes the rows of slot j
  PassParams py{};
  py.in = B;
  py.out = out_dev;
  py.in_sa = (long long)NH * N;
  py.in_sb = N;
  py.out_ob = 0;
  py.out_ok = nx;
  py.A = nx;
  py.B = G * nkc;
  py.tw_stage = ty.tw_stage;
  py.bg = nkc;
  py.b_off = chunk * G * nkc;
  py.bg_in = 1;
  py.bg_step = G;
  py.bg_gap = blk;
  py.ptab = tab;
  py.kcut = (ctx->bin_only && ctx->bin_N == N) ? ctx->d_kcut : nullptr;
  py.kz_fixed = -1;
  rc = route_transpose(ctx, N, 0, py, VPS_K_FFT_Y);
  if (rc || !last) return rc;
  // Nyquist plane: ky rows of destination h go behind that destination's kz rows
  PassParams pn{};
  pn.in = BN;
  pn.out = reinterpret_cast<cf*>(out_dev) + rows * nx;
  pn.in_sa = N;
  pn.in_sb = 0;
  pn.out_ob = 0;
  pn.out_ok = nx;
  pn.A = nx;
  pn.B = 1;
  pn.tw_stage = ty.tw_stage;
  pn.kg = nky;
  pn.kg_gap = blk - (long long)nky * nx;
  pn.kcut = py.kcut;
  pn.kz_fixed = NH;
  return route_transpose(ctx, N, 0, pn, VPS_K_FFT_Y);
}

}  // extern "C"

// y pass of one field: B[x][kz][y] (+BN[x][y]) -> spec[kz][ky][x] (+nyq[ky][x])
static int fft_y_of(vps_ctx* ctx, int N, int nx, const cf* B, const cf* BN, void* spec_dev, void* nyq_dev) {
  const int NH = N / 2;
  vps_fft_tables ty;
  int rc = vps_fft_get_tables(ctx, N, &ty);
  if (rc) return rc;
  PassParams py{};
  py.in = B;
  py.out = spec_dev;
  py.in_sa = (long long)NH * N;
  py.in_sb = N;
  py.out_ob = (long long)N * nx;
  py.out_ok = nx;
  py.A = nx;
  py.B = NH;
  py.tw_stage = ty.tw_stage;
  py.kcut = (ctx->bin_only && ctx->bin_N == N) ? ctx->d_kcut : nullptr;
  py.kz_fixed = -1;
  rc = route_transpose(ctx, N, 0, py, VPS_K_FFT_Y);
  if (rc) return rc;
  PassParams pn = py;
  pn.kz_fixed = NH;
  pn.in = BN;
  pn.out = nyq_dev;
  pn.in_sa = N;
  pn.in_sb = 0;
  pn.out_ob = 0;
  pn.B = 1;
  rc = route_transpose(ctx, N, 0, pn, VPS_K_FFT_Y);
  return rc;
}

int vps_pencil_tp(int N) { return pencil_tp(N / 2); }

bool vps_pencil_supported(vps_ctx* ctx, int N) {
  if (!vps_fft_supported(N) || N < 64 || N > 4096) return false;   // (4096: 8-line pencils of 2048 packed points on 1024 threads, 148 KB of LDS)
  const long long lds = route_pencil_lds(N / 2);
  if (lds < 0) return false;
  return (size_t)lds <= ctx->lds_per_cu;
}

// records sorted by pencil -> ncomp half spectra after the z and y passes (spec_dev == NULL: z pass only, the
// z images [component][B | BN] stay in bwork_dev)
int vps_fft_pencil_zy(vps_ctx* ctx, int N, int nx, const unsigned* records, const unsigned* start, float* side,
                      const PencilQuantity& q, float vol, void* spec_dev, void* nyq_dev, void* bwork_dev) {
  const int ncomp = q.ncomp, divide = q.divide, energy = q.energy, with_energy = q.with_energy, weighted = q.weighted, scalar = q.scalar;
  if (scalar && (ncomp != 1 || divide || energy || with_energy || weighted))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_pencil_zy: a scalar density quantity is one undivided field of its own");
  if (weighted && (!divide || energy || with_energy))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_pencil_zy: the density-weighted velocity is a dividing vector launch of its own");
  // with_energy = 1: a momentum launch (three components) that leaves the energy field's z image as component 3 of bwork_dev;
  // with_energy = 2: no launch -- the y pass of that component 3 (the energy quantity of a step whose momentum launch made it)
  if (with_energy && (energy != (with_energy == 2) || divide != (with_energy == 2 ? 1 : 0) || (with_energy == 1 && ncomp != 3)))
    return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_pencil_zy: the shared energy field needs an undivided three-component momentum launch");
  const int NH = N / 2;
  vps_fft_tables tz;
  int rc = vps_fft_get_tables(ctx, NH, &tz);
  if (rc) return rc;
  const size_t bfield = (size_t)nx * NH * N, bnyq = (size_t)nx * N;
  cf* Bbase = reinterpret_cast<cf*>(bwork_dev);
  PencilParams p{};
  p.records = records;
  p.start = start;
  p.side = side;
  p.N = N;
  p.nx = nx;
  p.nby = N / vps_pencil_tp(N);
  p.ncomp = ncomp;
  for (int c = 0; c < 3; ++c) p.chan[c] = q.chan[c < ncomp ? c : 0];
  for (int c = 0; c < 4; ++c) {
    p.out[c] = Bbase + (size_t)c * (bfield + bnyq);
    p.nyq[c] = p.out[c] + bfield;
  }
  p.divide = divide;
  p.energy = energy;
  p.with_energy = with_energy == 1;
  p.weighted = weighted;
  p.wexp = q.wexp;
  p.scalar = scalar;
  p.sexp = q.sexp;
  p.vol = vol;
  p.tw_stage = tz.tw_stage;
  p.tw_r2c = tz.tw_r2c;
  const long long npencils = (long long)nx * p.nby;
  if (with_energy != 2) {
    rc = route_pencil(ctx, NH, p, npencils);
    if (rc) return rc;
  }
  if (!spec_dev) return VPS_OK;
  cf* spec = reinterpret_cast<cf*>(spec_dev);
  cf* nyq = reinterpret_cast<cf*>(nyq_dev);
  if (with_energy == 2)      // the z image the momentum launch left as component 3
    return fft_y_of(ctx, N, nx, p.out[3], p.nyq[3], spec, nyq);
  const int nout = energy ? 1 : ncomp;
  for (int c = 0; c < nout; ++c) {
    rc = fft_y_of(ctx, N, nx, p.out[c], p.nyq[c], spec + (size_t)c * NH * N * nx, nyq + (size_t)c * N * nx);
    if (rc) return rc;
  }
  return VPS_OK;
}

extern "C" {

static int fft_x_impl(vps_ctx* ctx, int N, int64_t nlines, int64_t line0, int kz0, const void* in_dev,
                      const void* in1_dev, const void* in2_dev, int ncomp, int nseg, int64_t seg_stride,
                      int mode, double* psum_dev, unsigned long long* nsample_dev, void* out_dev,
                      const int2* ptab = nullptr, int kz_step = 1, double* psumc_dev = nullptr) {
  VPS_ENTER(ctx);
  if (int bad = check_fft_size(ctx, N)) return bad;
  if (nlines < 0 || !in_dev) return vps_fail(ctx, VPS_ERR_ARG, "bad line count / null input");
  if (nseg < 1 || N % nseg) return vps_fail(ctx, VPS_ERR_ARG, "nseg=%d must divide N", nseg);
  // modes 5 (|F|^2 into the full Hermitian grid) and 6 / 7 (signed binning of Re F) take whole lines of whole grids
  const bool realbin = mode == 6 || mode == 7;
  if ((mode == 5 || realbin) && nseg != 1) return vps_fail(ctx, VPS_ERR_ARG, "mode %d: nseg must be 1", mode);
  if (nlines == 0) return VPS_OK;
  vps_fft_tables tx;
  int rc = vps_fft_get_tables(ctx, N, &tx);
  if (rc) return rc;
  XParams p{};
  p.in = reinterpret_cast<const cf*>(in_dev);
  p.in1 = reinterpret_cast<const cf*>(in1_dev);
  p.in2 = reinterpret_cast<const cf*>(in2_dev);
  p.ncomp = ncomp;
  p.out = reinterpret_cast<cf*>(out_dev);
  p.nlines = nlines;
  p.line0 = line0;
  p.N = N;
  p.kz0 = kz0;
  p.seglen = N / nseg;
  p.seg_shift = 0;
  while ((1 << p.seg_shift) < p.seglen) ++p.seg_shift;
  if ((1 << p.seg_shift) != p.seglen) p.seg_shift = -1;   // not a power of two: the kernel divides
  p.seg_stride = seg_stride;
  p.tw_stage = tx.tw_stage;
  p.ptab = ptab;
  p.kz_step = kz_step;
  if (ptab && (line0 != 0 || nlines % N || (mode != 0 && mode != 3)))
    return vps_fail(ctx, VPS_ERR_ARG, "chunk planes: whole planes from line 0, binning modes only");
  const bool binning = mode == 0 || mode == 3 || realbin;
  const bool counting = mode == 0 || mode == 6;
  int fastmode = 0;
  if (binning) {
    if (ctx->bin_N != N || !ctx->d_k2) return vps_fail(ctx, VPS_ERR_ARG, "vps_set_binning(N=%d) has not been called", N);
    if (!psum_dev || (counting && !nsample_dev)) return vps_fail(ctx, VPS_ERR_ARG, "null accumulator");
    if (realbin && ctx->d_win)
      return vps_fail(ctx, VPS_ERR_ARG, "mode %d bins a real-space lattice: a k-space window is set (vps_set_window(NULL) first)", mode);
    const long long maxline = line0 + nlines - 1;
    if (kz0 + (int)(maxline / N) * kz_step > N / 2) return vps_fail(ctx, VPS_ERR_ARG, "kz range exceeds N/2");
    p.k2 = ctx->d_k2;
    p.thr = ctx->d_thr;
    if (ctx->d_win && ctx->win_N != N) return vps_fail(ctx, VPS_ERR_ARG, "vps_set_window was called for N=%d, not %d", ctx->win_N, N);
    p.win = ctx->d_win;
    p.nbins = ctx->nbins;
    p.edge0 = (float)ctx->edge0;
    p.inv_spacing = (float)ctx->inv_spacing;
    p.psum = psum_dev;
    p.nsample = nsample_dev;
    p.pair = (ctx->bin_fast && line0 % N == 0 && nlines % N == 0 && vps_option("no_pair_binning", 0) == 0) ? 1 : 0;
    p.nthr = ctx->d_nthr;
    p.nmax = ctx->bin_nmax;
    p.kf = ctx->bin_kf;
    fastmode = !ctx->bin_fast ? 0 : (ctx->bin_int && ctx->d_nthr && vps_option("no_int_binning", 0) == 0) ? 2 : 1;
    p.psumc = psumc_dev;
    if (psumc_dev && ncomp != 3) return vps_fail(ctx, VPS_ERR_ARG, "Helmholtz decomposition: ncomp must be 3");
  } else if (mode == 1 || mode == 2 || mode == 5) {
    if (!out_dev) return vps_fail(ctx, VPS_ERR_ARG, "null output");
    // mode 5 addresses the full grid by (ky, kz): every plane of the call and its partner N - kz must lie inside it
    if (mode == 5 && (line0 < 0 || kz0 < 0 || kz0 + (line0 + nlines - 1) / N > N / 2))
      return vps_fail(ctx, VPS_ERR_ARG, "mode 5: kz range exceeds 0..N/2");
  } else if (mode != 4) {
    return vps_fail(ctx, VPS_ERR_ARG, "mode must be 0..7");
  }
  // (modes 0 and 3 are the kernel's binning MODE 0, with and without the shell counts; 6 and 7 its signed variant)
  return route_x(ctx, N, realbin ? 6 : (binning ? 0 : mode), counting, p, fastmode, binning && psumc_dev);
}

int vps_fft_x(vps_ctx* ctx, int N, int64_t nlines, int64_t line0, int kz0, const void* in_dev,
              int nseg, int64_t seg_stride, int mode, double* psum_dev,
              unsigned long long* nsample_dev, void* out_dev) {
  return fft_x_impl(ctx, N, nlines, line0, kz0, in_dev, in_dev, in_dev, 1, nseg, seg_stride, mode, psum_dev,
                    nsample_dev, out_dev);
}

// ncomp_min .. 3 components, each given; `who`: the entry point, for the message
static int check_components(vps_ctx* ctx, const char* who, const void* const* in_devs, int ncomp, int ncomp_min) {
  if (ncomp < ncomp_min || ncomp > 3 || !in_devs)
    return vps_fail(ctx, VPS_ERR_ARG, ncomp_min == 3 ? "%s: ncomp must be 3" : "%s: ncomp must be 1..3", who);
  for (int c = 0; c < ncomp; ++c)
    if (!in_devs[c]) return vps_fail(ctx, VPS_ERR_ARG, "%s: null component %d", who, c);
  return VPS_OK;
}

int vps_fft_x_bin(vps_ctx* ctx, int N, int64_t nlines, int64_t line0, int kz0, const void* const* in_devs,
                  int ncomp, int nseg, int64_t seg_stride, int count, double* psum_dev,
                  unsigned long long* nsample_dev) {
  VPS_ENTER(ctx);
  if (int bad = check_components(ctx, "vps_fft_x_bin", in_devs, ncomp, 1)) return bad;
  return fft_x_impl(ctx, N, nlines, line0, kz0, in_devs[0], in_devs[ncomp > 1 ? 1 : 0], in_devs[ncomp > 2 ? 2 : 0],
                    ncomp, nseg, seg_stride, count ? 0 : 3, psum_dev, nsample_dev, nullptr);
}

// Binning x pass of ONE received chunk of the slab exchange: in_devs[c] = the G blocks this rank received for component c
// (vps_fft_y's layout, x running over the senders' slabs), `packed` as the senders' vps_fft_y_packed said.  Planes of slot j
// are kz = chunk*G*nkc + j*G + rank; the last chunk's blocks end with this rank's Nyquist-plane rows, binned here too.
static int fft_x_bin_chunk_impl(vps_ctx* ctx, int N, int nx, int G, int nchunks, int chunk, int rank, int packed,
                                const void* const* in_devs, int ncomp, int count, double* psum_dev,
                                unsigned long long* nsample_dev, double* psumc_dev) {
  if (int bad = check_components(ctx, "vps_fft_x_bin_chunk", in_devs, ncomp, 1)) return bad;
  if (nx < 1 || nx * G != N || rank < 0 || rank >= G) return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_x_bin_chunk: nx * G must be N, 0 <= rank < G");
  if (G > vps_x_max_ranks(N))
    return vps_fail(ctx, VPS_ERR_UNSUPPORTED, "vps_fft_x_bin_chunk: N=%d takes at most %d ranks (G=%d): the x pass needs segments of at "
                    "least %d points", N, vps_x_max_ranks(N), G, N / vps_x_max_ranks(N));
  const int2* tab = nullptr;
  long long rows = 0;
  int rc = ypack_get(ctx, N, G, nchunks, chunk, packed != 0, &tab, &rows);
  if (rc) return rc;
  const int nkc = N / 2 / G / nchunks, nky = N / G;
  const bool last = chunk == nchunks - 1;
  const long long blk = rows * nx + (last ? (long long)nky * nx : 0);
  const int mode = count ? 0 : 3;
  rc = fft_x_impl(ctx, N, (int64_t)nkc * N, 0, chunk * G * nkc + rank, in_devs[0], in_devs[ncomp > 1 ? 1 : 0],
                  in_devs[ncomp > 2 ? 2 : 0], ncomp, G, blk, mode, psum_dev, nsample_dev, nullptr, tab, G, psumc_dev);
  if (rc || !last) return rc;
  const cf* nq[3];
  for (int c = 0; c < 3; ++c) nq[c] = reinterpret_cast<const cf*>(in_devs[c < ncomp ? c : 0]) + rows * nx;
  return fft_x_impl(ctx, N, nky, (int64_t)rank * nky, N / 2, nq[0], nq[1], nq[2], ncomp, G, blk, mode, psum_dev, nsample_dev,
                    nullptr, nullptr, 1, psumc_dev);
}

int vps_fft_x_bin_chunk(vps_ctx* ctx, int N, int nx, int G, int nchunks, int chunk, int rank, int packed,
                        const void* const* in_devs, int ncomp, int count, double* psum_dev,
                        unsigned long long* nsample_dev) {
  VPS_ENTER(ctx);
  return fft_x_bin_chunk_impl(ctx, N, nx, G, nchunks, chunk, rank, packed, in_devs, ncomp, count, psum_dev, nsample_dev, nullptr);
}

// Helmholtz decomposition (include/vps_hip.h): the binning x passes above with a second accumulator of the compressive part
int vps_fft_x_bin_helmholtz(vps_ctx* ctx, int N, int64_t nlines, int64_t line0, int kz0, const void* const* in_devs,
                            int ncomp, int nseg, int64_t seg_stride, int count, double* psum_dev,
                            unsigned long long* nsample_dev, double* psum_comp_dev) {
  VPS_ENTER(ctx);
  if (int bad = check_components(ctx, "vps_fft_x_bin_helmholtz", in_devs, ncomp, 3)) return bad;
  if (!psum_comp_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_x_bin_helmholtz: null compressive accumulator");
  return fft_x_impl(ctx, N, nlines, line0, kz0, in_devs[0], in_devs[1], in_devs[2], 3, nseg, seg_stride, count ? 0 : 3,
                    psum_dev, nsample_dev, nullptr, nullptr, 1, psum_comp_dev);
}

int vps_fft_x_bin_chunk_helmholtz(vps_ctx* ctx, int N, int nx, int G, int nchunks, int chunk, int rank, int packed,
                                  const void* const* in_devs, int ncomp, int count, double* psum_dev,
                                  unsigned long long* nsample_dev, double* psum_comp_dev) {
  VPS_ENTER(ctx);
  if (int bad = check_components(ctx, "vps_fft_x_bin_chunk_helmholtz", in_devs, ncomp, 3)) return bad;
  if (!psum_comp_dev) return vps_fail(ctx, VPS_ERR_ARG, "vps_fft_x_bin_chunk_helmholtz: null compressive accumulator");
  return fft_x_bin_chunk_impl(ctx, N, nx, G, nchunks, chunk, rank, packed, in_devs, 3, count, psum_dev, nsample_dev,
                              psum_comp_dev);
}

// All three passes of one whole N^3 field: z and y into the second half of the workspace, then the x pass in `mode` over the
// kz < N/2 planes and the Nyquist plane, whose output starts (N/2) N^2 elements of `out_elem` bytes behind out_dev.
// bin_only: the y pass may skip the rows beyond the last shell edge (vps_set_bin_only), for this call only.
static int fft3_whole(vps_ctx* ctx, int N, const float* field_dev, void* work_dev, bool bin_only, int mode, double* psum_dev,
                      unsigned long long* nsample_dev, void* out_dev, size_t out_elem) {
  VPS_ENTER(ctx);
  if (int bad = check_fft_size(ctx, N)) return bad;
  const size_t half = vps_fft_workspace_bytes(N, N);
  char* w = reinterpret_cast<char*>(work_dev);
  cf* spec = reinterpret_cast<cf*>(w + half);
  cf* nyq = spec + (size_t)(N / 2) * N * N;
  const bool keep = ctx->bin_only;
  ctx->bin_only = bin_only;
  int rc = vps_fft_zy(ctx, N, N, field_dev, spec, nyq, w);
  ctx->bin_only = keep;
  if (rc) return rc;
  rc = vps_fft_x(ctx, N, (int64_t)(N / 2) * N, 0, 0, spec, 1, 0, mode, psum_dev, nsample_dev, out_dev);
  if (rc) return rc;
  void* out_nyq = out_dev ? reinterpret_cast<char*>(out_dev) + (size_t)(N / 2) * N * N * out_elem : nullptr;
  return vps_fft_x(ctx, N, N, 0, N / 2, nyq, 1, 0, mode, psum_dev, nsample_dev, out_nyq);
}

int vps_power_bin(vps_ctx* ctx, int N, const float* field_dev, void* work_dev, double* psum_dev,
                  unsigned long long* nsample_dev) {
  // binned right away: modes beyond the last shell edge need not be stored
  return fft3_whole(ctx, N, field_dev, work_dev, true, 0, psum_dev, nsample_dev, nullptr, 0);
}

// (every mode is wanted by these two: no store cut in the y pass)
int vps_rfft3(vps_ctx* ctx, int N, const float* field_dev, void* work_dev, void* out_dev) {
  return fft3_whole(ctx, N, field_dev, work_dev, false, 1, nullptr, nullptr, out_dev, sizeof(cf));
}

int vps_power_grid(vps_ctx* ctx, int N, const float* field_dev, void* work_dev, float* power_dev) {
  return fft3_whole(ctx, N, field_dev, work_dev, false, 2, nullptr, nullptr, power_dev, sizeof(float));
}

}  // extern "C"
