/* vps_hip.h -- C ABI of libvps_hip.so: the MI355X (gfx950) hot path
 *   particles -> grid (NGP deposit | exact-NN resample) -> 3-D R2C FFT -> |f(k)|^2
 *   -> spherical-shell binning
 * that replaces the CPU path of YujieH3/large-velocity-power-spectrum behind the
 * reference's own Python function surface.
 *
 * The reference has NO FFI of its own for this path (it is pure numpy calling
 * pyFFTW / pyann / Annoy): every entry point below cites the
 * reference Python function (file:line under /root/reference) whose arithmetic it
 * replaces.  INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns 0 on success or a
 *     negative vps_status; nothing throws.  vps_last_error() gives the message.
 *   - "dev" pointers are device (HBM) addresses owned by the CALLER (e.g.
 *     torch.Tensor.data_ptr() or vps_malloc); "host" pointers are ordinary memory.
 *   - Streams.  All device work is enqueued on the context's stream (vps_set_stream;
 *     default: the null stream), the library's own memsets, copies and table uploads
 *     included; tests/stream_probe.py lists every entry point under one of three heads.
 *       PURE ENQUEUES return while the stream may still be busy: vps_memset,
 *         vps_cell_index, vps_density_velocity_vector, vps_deposit_ngp, vps_deposit_field,
 *         vps_deposit_fft_zy, vps_deposit_fft_z, vps_assign_expand, vps_deposit_assign,
 *         vps_field_algebra[_out], vps_fft_zy[_weighted], vps_fft_z, vps_fft_y, vps_fft_x,
 *         vps_fft_x_bin[_chunk][_helmholtz], vps_power_bin, vps_rfft3, vps_power_grid,
 *         vps_spectrum_zimages, vps_allreduce_shells, vps_set_stream.  One exception: a
 *         call that must regrow or rebuild a table the CONTEXT owns (the x pass's partial
 *         sums, the chunk tables of vps_fft_y after new binning tables or another chunk
 *         count, FFT twiddles of a new length) drains the stream first, that once.
 *       BLOCKING calls return only after the stream has drained, each because it brings a
 *         value to the host: vps_preprocess (minimum, bulk velocity), vps_totals,
 *         vps_count_in_slab, vps_deposit_fft_z_slab (the compaction counter of a slab-sized
 *         sort), vps_nn_resample* (bounding box; open-point count under timing),
 *         vps_hist_pairs, vps_memcpy_d2h, vps_timing_reset / _get / _list, vps_sync,
 *         vps_destroy, vps_comm_destroy; vps_set_binning and vps_set_window when the table
 *         CHANGES (a pending launch may still read the old one; unchanged tables: nothing
 *         happens); vps_pair_k and vps_memcpy_h2d take host data in stream order and
 *         complete the copy before returning.
 *       Everything else is host-only: nothing is enqueued.
 *     HOST POINTERS ARE FREE ON RETURN of every call, and the library enforces it: tables
 *     and edges go up by a synchronous copy, pointer lists are read on the host, and every
 *     call that copies host axes in stream order drains the stream behind the copy; no
 *     call relies on how the runtime treats pageable memory.
 *     vps_set_stream with ANOTHER stream than the current one records an event on the old
 *     stream and makes the new one wait for it: what earlier calls left for later ones --
 *     the context's tables and partial sums, the caller's sort workspace under
 *     VPS_FLAG_REUSE_SORT / VPS_FLAG_SHARE_ENERGY -- is complete before the first call on
 *     the new stream reads it.  The old stream must still exist at that moment: if it was
 *     destroyed first the call reports VPS_ERR_HIP once, nothing is ordered behind it, and
 *     the context is on the new stream all the same.  The event is recorded on the old
 *     stream, which ends a stream capture in progress there (the library captures none).
 *     With the same stream it does nothing (one pointer compare).  Buffers the CALLER hands from
 *     one stream to another are the caller's to order, as with any stream-ordered library.
 *   - Grids are float32, C order.  A multi-channel grid is channel-major (SoA):
 *     grid[c][x][y][z].  Slab decomposition is along x: a rank owns
 *     x in [x0, x0+nx).  N is the global cells-per-axis.
 *   - Calls on one context are not re-entrant.
 */
#ifndef VPS_HIP_H
#define VPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vps_ctx vps_ctx;

enum vps_status {
  VPS_OK = 0,
  VPS_ERR_ARG = -1,        /* bad argument (message says which)                 */
  VPS_ERR_HIP = -2,        /* a HIP runtime call failed                          */
  VPS_ERR_UNSUPPORTED = -3,/* e.g. N not a supported FFT length                  */
  VPS_ERR_NOMEM = -4
};

/* quantities of BoxField.spctrm (interp.py:573-583) */
enum vps_quantity { VPS_VELOCITY = 0, VPS_MOMENTUM = 1, VPS_ENERGY = 2,
                    VPS_VM = 3 /* BoxField form: v in channels 0..2, mass in channel 3 */,
                    VPS_WEIGHTED_VELOCITY = 4 /* ABI 8: w = rho^alpha v, alpha from vps_set_density_weight (below) */,
                    VPS_DENSITY = 5 /* ABI 11: the scalar s = rho^alpha (alpha = 1: the density itself), see below */,
                    VPS_LOG_DENSITY = 6 /* ABI 11: the scalar s = ln rho */,
                    /* an addition within ABI 13, vps_deposit_field ONLY: scalars of the second moment S2 = sum w rho_p |v_p|^2 of
                       a cell's contributions, see "Sub-grid velocity dispersion" below */
                    VPS_TOTAL_ENERGY = 7, VPS_SUBGRID_ENERGY = 8, VPS_DISPERSION = 9,
                    /* an addition within ABI 13, vps_deposit_field ONLY: the six components of that second moment as a tensor,
                       see "Sub-grid stress tensor" below */
                    VPS_SUBGRID_STRESS = 10, VPS_DISPERSION_TENSOR = 11,
                    /* an addition within ABI 13, vps_field_algebra_out ONLY: central differences of the velocity of a whole
                       gridded field, see "Velocity-gradient fields" below */
                    VPS_DIVERGENCE = 12, VPS_VORTICITY = 13, VPS_STRAIN_RATE = 14,
                    /* an addition within ABI 13, vps_field_algebra_out ONLY: the mass-weighted box filter of a whole gridded
                       field at a chosen half-width, see "Box-filtered fields" below.  The code 15 is left unassigned ON PURPOSE:
                       it is the code hosts and tests probe as "the first unknown quantity" (VPS_ERR_ARG, "quantity 15") and
                       stays that */
                    VPS_FILTERED_VM = 16, VPS_FILTERED_STRESS = 17 };
/* flags for vps_field_algebra */
#define VPS_FLAG_REFERENCE_MOMENTUM_BUG 1 /* py=pz=vx*mass as interp.py:523-525 */
#define VPS_FLAG_INPUT_IS_VM 2             /* channels already hold vx,vy,vz,mass (a BoxField) */
#define VPS_FLAG_REUSE_SORT 4              /* vps_deposit_fft_zy: work_dev still holds the bucketed records of the
                                              previous call with the SAME particles, N, Lbox, x0, nx -- skip the sort
                                              (several quantities of one snapshot) */
#define VPS_FLAG_SHARE_ENERGY 8            /* vps_deposit_fft_zy / vps_deposit_fft_z[_slab], momentum and kinetic energy of ONE snapshot:
                                              on the VPS_MOMENTUM call (all three components, no VPS_FLAG_REFERENCE_MOMENTUM_BUG) the
                                              launch ALSO leaves the z image of the energy field E = mass |v|^2 -- made of the same cell
                                              totals of rho v_c -- as a FOURTH component (workspace sized by
                                              vps_deposit_fft_zy_workspace_bytes_shared; a zimg_dev of four components); on the following
                                              VPS_ENERGY call (with VPS_FLAG_REUSE_SORT: same particles, N, Lbox, x0, nx, same
                                              workspace / zimg_dev) nothing is deposited: vps_deposit_fft_zy runs the y pass of that
                                              component, vps_deposit_fft_z[_slab] returns at once (the caller reads component 3).
                                              Same numbers as the energy launch of its own up to the order of float32 additions. */

#define VPS_FLAG_COMPONENTS(mask) (((mask) & 7) << 4) /* vps_deposit_fft_zy / vps_deposit_fft_z[_slab], velocity or momentum: produce
                                              ONLY the components in `mask` (bit c = component c; 0 = all three), in ascending
                                              order at the start of the output -- the scalar images / half spectra of the
                                              three-component call (up to the order of the LDS float adds).  For hosts that deal
                                              the scalar fields of a step out over several GPUs (whole grids, no exchange). */
#define VPS_FLAG_COMPONENT(c) VPS_FLAG_COMPONENTS(1 << (c))
#define VPS_FLAG_COMPONENT_MASK 0x70
#define VPS_FLAG_ASSIGN(order) ((((order) - 1) & 3) << 8) /* vps_deposit_field ONLY (an addition within ABI 13): deposit [rho v, rho]
                                              by cloud-in-cell (order 2: 0x100) or triangular-shaped cloud (order 3: 0x200) instead of
                                              NGP, by the direct route's rule (vps_deposit_assign) with the quantity formed in the owner
                                              brick's epilogue; see vps_deposit_field.  Order 1 is no bit at all: the NGP call.  The value
                                              0x300, and either bit on any other entry point that takes flags (vps_deposit_fft_zy,
                                              vps_deposit_fft_z[_slab], vps_field_algebra[_out], vps_nn_resample_quantity) or together
                                              with VPS_FLAG_INPUT_IS_VM: VPS_ERR_ARG before anything is enqueued. */
#define VPS_FLAG_ASSIGN_MASK 0x300
#define VPS_FLAG_FILTER(m) (((m) & 0xfff) << 12)   /* half-width m in cells, box of (2m+1)^3 cells */
#define VPS_FLAG_FILTER_MASK 0xfff000              /* VPS_FILTERED_VM / VPS_FILTERED_STRESS ONLY (an addition within ABI 13), see
                                              "Box-filtered fields"; no other code or entry point gives the field a meaning */

/* ---- lifecycle ---------------------------------------------------------- */
int vps_create(vps_ctx** out, int device_id);
int vps_destroy(vps_ctx* ctx);
const char* vps_last_error(const vps_ctx* ctx);   /* ctx may be NULL: global slot */
int vps_set_stream(vps_ctx* ctx, void* hip_stream);
int vps_sync(vps_ctx* ctx);
#define VPS_ABI_VERSION 13
int vps_version(void);                            /* ABI version (VPS_ABI_VERSION)  */
/* Tuning / test switches, process-wide.  The library never reads the environment: a stray variable in a user's job cannot
 * change a code path; the host sets what it wants explicitly (vpower/_ffi.py maps VPS_OPT_<NAME> variables once, at load,
 * and lists them in _ffi.OPTIONS).  Names: no_fast_binning, no_pair_binning, nn_query_centric, nn_column, nn_build_atomic, nn_kappa, nn_stats,
 * sort_groups, sort_staged, sort_atomic (all result-preserving), nn_ablate (timing-only builds; ignored by the product
 * build).  A NaN value restores the default.  Unknown names: VPS_ERR_ARG.
 * Further names: no_int_binning (1: float64 shells even where integer shells are exact), x_wg_per_cu (persistent x-pass workgroups
 * per CU, tuning), comm_fail_send (error-path tests: the n-th ncclSend fails without being issued).
 * Options that shape a WORKSPACE LAYOUT -- nn_build_atomic, sort_atomic, sort_staged, sort_groups -- must not change between a
 * *_workspace_bytes call and the run that uses the workspace sized with it (nor before a VPS_FLAG_REUSE_SORT call): the run
 * entry points take no size and recompute the layout under the current values. */
int vps_set_option(const char* name, double value);
double vps_get_option(const char* name, double dflt);
/* device facts for the host side: out[0]=CUs, out[1]=LDS bytes/CU, out[2]=wave size,
 * out[3]=HBM bytes total (MiB) */
int vps_device_info(vps_ctx* ctx, int64_t out[4]);
/* how the binning x pass will decide shells for the tables of the last vps_set_binning, under the current options:
 * 0 = general monotone shell walk; 1 = mirrored kx, float64 k^2 sums against float64 thresholds; 2 = mirrored kx, INTEGER
 * ix^2 + iy^2 + iz^2 against integer thresholds (exactly the same shells: chosen only where vps_set_binning has checked
 * that no threshold lies on an integer multiple of k2[1]); negative: no tables set */
int vps_binning_mode(vps_ctx* ctx);

/* Density-weighted velocity (ABI 8; an extension, the reference has no such quantity): VPS_WEIGHTED_VELOCITY is the vector
 * field w_c = rho^alpha v_c = (sum rho v_c) rho^(alpha - 1) with rho the cell's density total (NGP) or the nearest particle's
 * density (exact NN), rho = mass / Lcell^3 for a gridded field (VPS_FLAG_INPUT_IS_VM); w = 0 where rho = 0 for EVERY alpha,
 * 0 included.  alpha = 1/3: the scaling variable of supersonic turbulence; 1/2: the spectrum that integrates to the kinetic
 * energy density; alpha = 0 is VPS_VELOCITY and alpha = 1 is VPS_MOMENTUM / Lcell^3 (to float32 rounding: the power is formed
 * as exp2((alpha - 1) log2 rho) on the hardware units where VPS_VELOCITY takes a reciprocal).
 * vps_set_density_weight stores alpha (any finite double; else VPS_ERR_ARG) on the context, like vps_set_window; it is read
 * when a call is enqueued.  The quantity is taken by vps_deposit_field, vps_deposit_fft_zy[_supported], vps_deposit_fft_z[_slab],
 * vps_nn_resample_quantity, vps_field_algebra[_out]: three output channels, VPS_FLAG_COMPONENTS and VPS_FLAG_REUSE_SORT as for
 * VPS_VELOCITY.  VPS_ERR_ARG, before anything is enqueued: the quantity on a context whose alpha was never set; with
 * VPS_FLAG_SHARE_ENERGY or VPS_FLAG_REFERENCE_MOMENTUM_BUG.  Outside the contract: densities that are float32 denormals or
 * negative, and powers rho^(alpha - 1) (rho^alpha for gridded input) beyond the float32 range. */
int vps_set_density_weight(vps_ctx* ctx, double alpha);

/* Density and log-density (ABI 11; an extension): two SCALAR quantities, one output channel / spectrum / z image each, of the
 * rho that VPS_WEIGHTED_VELOCITY calls rho -- the cell's density total (NGP / CIC / TSC), the nearest particle's density
 * (exact NN), mass / Lcell^3 for a gridded field (VPS_FLAG_INPUT_IS_VM):
 *   VPS_DENSITY      s = rho^alpha, alpha from vps_set_density_weight; s = 0 where rho = 0 for every alpha.  alpha = 1 is the
 *                    plain density and takes NO transcendental: the float32 cell total goes into the transform as it is.
 *                    Otherwise the power is exp2(alpha log2 rho) on the hardware units.
 *   VPS_LOG_DENSITY  s = ln rho = log2 rho * ln 2, the natural logarithm of rho in the caller's units; s = 0 where rho = 0.
 *                    A reference density rho0 (s = ln(rho / rho0)) only moves the k = 0 mode, which no shell holds, AS LONG AS
 *                    NO CELL IS EMPTY; an empty cell enters the field as if it held rho = 1.  With a sparse NGP grid rescale the
 *                    densities (so that 1 is a sensible floor) or take the NN route, which has no empty cells.
 * Both are taken by vps_deposit_field, vps_deposit_fft_zy[_supported], vps_deposit_fft_z[_slab], vps_nn_resample_quantity and
 * vps_field_algebra[_out] (in place: channel 0); VPS_FLAG_REUSE_SORT as for every quantity.  VPS_ERR_ARG, before anything is
 * enqueued: VPS_DENSITY on a context whose alpha was never set; either code with VPS_FLAG_COMPONENTS, VPS_FLAG_SHARE_ENERGY or
 * VPS_FLAG_REFERENCE_MOMENTUM_BUG.  Outside the contract, as for the weighted velocity: densities that are float32 denormals
 * or negative, powers rho^alpha beyond the float32 range. */

/* Sub-grid velocity dispersion (an addition within ABI 13: no new symbol; an extension): three SCALAR quantities, one output
 * channel each, of what a cell's particles do around its mean velocity.  The sums run over the contributions to a cell, each
 * with its weight w (1 for NGP, the CIC / TSC weight with VPS_FLAG_ASSIGN); vol = Lcell^3; S2 = sum w rho_p |v_p|^2, formed per
 * contribution as (px^2 + py^2 + pz^2) / rho_p from its [rho v, rho] record (0 where rho_p = 0) and kept in a FIFTH channel of
 * the brick's LDS tile; P = sum w rho v and R = sum w rho are the four channels every quantity is made of:
 *   VPS_TOTAL_ENERGY    vol S2                         the kinetic energy of the cell's particles (no factor 1/2, as VPS_ENERGY)
 *   VPS_SUBGRID_ENERGY  vol (S2 - |P|^2 / R), >= 0     the part VPS_ENERGY = vol |P|^2 / R does not resolve
 *   VPS_DISPERSION      (S2 - |P|^2 / R) / R, >= 0     sigma^2 = <|v|^2> - |<v>|^2, density weighted
 * all 0 in a cell without mass; the difference is clamped at 0 from below and is exactly 0 in a cell with one NGP contribution.
 * VPS_ENERGY + VPS_SUBGRID_ENERGY = VPS_TOTAL_ENERGY cell by cell up to float32 rounding (the sub-grid energy subtracts the
 * resolved energy exactly as VPS_ENERGY forms it: the sum is the total to the rounding of that one subtraction), and the sum of VPS_TOTAL_ENERGY over
 * the cells is vol sum_p rho_p |v_p|^2 for NGP, CIC and TSC alike (the weights of a particle sum to 1).
 * Taken by vps_deposit_field ALONE (NGP and VPS_FLAG_ASSIGN(2 | 3), any x-slab, the workspaces of the 4-channel call).
 * VPS_ERR_ARG with a message naming the quantity, before anything is enqueued: vps_field_algebra[_out] (a 4-channel grid does
 * not hold a second moment), vps_nn_resample_quantity (one nearest particle has no dispersion), vps_deposit_fft_zy /
 * vps_deposit_fft_z[_slab] (vps_deposit_fft_zy_supported returns 0), and the codes with VPS_FLAG_REFERENCE_MOMENTUM_BUG or
 * VPS_FLAG_INPUT_IS_VM.  VPS_ERR_UNSUPPORTED, before anything is enqueued: a device whose LDS does not hold the 5-channel tile. */

/* Sub-grid stress tensor (an addition within ABI 13: no new symbol; an extension): the second moment itself, of which the three
 * scalars above are the trace.  S_ij = sum w rho_p v_i v_j, formed per contribution as p_i p_j / rho_p from its [rho v, rho]
 * record (0 where rho_p = 0), the way S2 is; P, R, vol and w as above.  SIX output channels each, in the order xx, yy, zz, xy,
 * xz, yz, laid out fields_dev[6][nx][N][N]:
 *   VPS_SUBGRID_STRESS     vol (S_ij - P_i P_j / R)      tau_ij, the sub-grid (Reynolds) stress of the coarse-grained momentum equation
 *   VPS_DISPERSION_TENSOR  (S_ij - P_i P_j / R) / R      sigma_ij = tau_ij / (vol R), the velocity-dispersion tensor
 * all 0 in a cell without mass.  A diagonal channel is clamped at 0 from below; an off-diagonal channel has either sign and is
 * not clamped.  P_i P_j / R is the float32 expression of the contribution's p_i p_j / rho_p, so a cell with ONE NGP contribution
 * is exactly 0 in all six channels.  The sum of the three diagonal channels is VPS_SUBGRID_ENERGY (VPS_DISPERSION) up to float32
 * rounding.
 * Taken by vps_deposit_field ALONE (NGP and VPS_FLAG_ASSIGN(2 | 3), any x-slab, the workspaces of the 4-channel call).  The one
 * sort of the call is followed by TWO accumulation launches over the same records, at every N: the diagonal half writes channels
 * 0..2, the off-diagonal half channels 3..5, each from an LDS tile of the four totals and three second-moment channels (7 cells
 * floats: 56 KiB, 112 KiB from N = 1024 on).  Both launches are timed under VPS_K_ALGEBRA.
 * VPS_ERR_ARG with a message naming the quantity, before anything is enqueued: every refusal of the three scalars above, and the
 * codes with VPS_FLAG_COMPONENTS.  VPS_ERR_UNSUPPORTED, before anything is enqueued: a device whose LDS does not hold the
 * 7-channel tile. */

/* Velocity-gradient fields (an addition within ABI 13: no new symbol; an extension): three quantities made of the nine first
 * derivatives of the velocity u of a WHOLE periodic grid, by second-order central differences.  With h = (float)(1 / (2 Lcell))
 * rounded once on the host, e_a the unit step along axis a and every index wrapped mod N,
 *   d_a u_c (i) = (u_c(i + e_a) - u_c(i - e_a)) * h
 *   VPS_DIVERGENCE   1 channel   (dx ux + dy uy) + dz uz                          the dilatation
 *   VPS_VORTICITY    3 channels  x: dy uz - dz uy, y: dz ux - dx uz, z: dx uy - dy ux
 *   VPS_STRAIN_RATE  6 channels  xx, yy, zz, xy, xz, yz (the order of the stress tensor): S_aa = d_a u_a,
 *                                S_xy = 0.5f * (dy ux + dx uy), S_xz = 0.5f * (dz ux + dx uz), S_yz = 0.5f * (dz uy + dy uz)
 * in float32 in exactly this order of operations, no fused multiply-add: exact for integer velocities and a power-of-two Lcell.
 * The transfer function of the scheme is sin(k Lcell) / Lcell for the wavenumber k: the derivative of the field as resolved at
 * the cell, which is the filter scale of everything the sub-grid quantities above mean -- no higher order is offered.
 * -tau_ij S_ij of VPS_SUBGRID_STRESS and VPS_STRAIN_RATE is the sub-grid energy flux.
 * Taken by vps_field_algebra_out ALONE: chans_dev [4][ncell] holds [v, mass] (VPS_FLAG_INPUT_IS_VM is required and is the only
 * flag taken; channel 3 is not read), out_dev [1 | 3 | 6][ncell] is required and must not overlap chans_dev, and
 * ncell = N^3 for an integer N >= 4 (with the call's ncell % 4 == 0: N even), the cell (ix, iy, iz) at (ix N + iy) N + iz.  N is
 * not tied to the FFT sizes.  Whole grids only: an x-slab would need its neighbours' boundary planes.  One launch on the
 * context's stream, timed under VPS_K_ALGEBRA; every output element has one writer and no atomics are used.
 * VPS_ERR_ARG with a message naming the quantity, before anything is enqueued: the in-place vps_field_algebra or a null
 * out_dev; a null chans_dev; overlapping buffers; chans_dev or out_dev not 16-byte aligned; an Lcell that is not positive and
 * finite, or whose h is not a positive finite float32; a call without VPS_FLAG_INPUT_IS_VM or with any other flag; an ncell that is
 * no cube, or N < 4; and the three codes on vps_deposit_field, vps_deposit_fft_zy, vps_deposit_fft_z[_slab] (vps_deposit_fft_zy_supported
 * returns 0) and vps_nn_resample_quantity. */

/* Box-filtered fields (an addition within ABI 13: no new symbol; an extension): the gridded field coarse-grained with a periodic
 * box of (2m+1)^3 cells, half-width m = (flags & VPS_FLAG_FILTER_MASK) >> 12, on the grid it already has -- the filter scale is
 * l = (2m+1) Lcell.  W(i) is the box centred on cell i, every index wrapped mod N.  Per cell, from chans_dev [4][ncell] =
 * [u_x, u_y, u_z, mass], in float32 with no fused multiply-add:  p_c = mass * u_c  and  s_ij = p_i * u_j (i <= j).  Box sums
 * M = sum_W mass, P_c = sum_W p_c, S_ij = sum_W s_ij; c = (float)(1 / (2m+1)^3) rounded once on the host.
 *   VPS_FILTERED_VM      4 channels  u~_c = P_c / M, mbar = M * c (both 0 where the box holds no mass): again a [v, mass] grid -- the Favre-filtered
 *                                    velocity and the filtered mass -- which every entry point that takes VPS_FLAG_INPUT_IS_VM
 *                                    reads (spectra, correlations, the gradient codes above, totals)
 *   VPS_FILTERED_STRESS  6 channels  xx, yy, zz, xy, xz, yz:  tau_l,ij = (S_ij - (P_i * P_j) / M) * c  in exactly this order of
 *                                    operations; a diagonal channel is clamped at 0 from below BEFORE the multiplication by c, an
 *                                    off-diagonal channel is not clamped; all six are 0 where M == 0.  Units of
 *                                    VPS_SUBGRID_STRESS: mass x velocity^2 per cell.
 * FIXED: the two products per cell, the division, the subtraction, the clamp and the multiplication by c, each one float32
 * rounding in the order written.  NOT FIXED: the order of the additions inside a box sum -- the kernel (filter.hip) adds along z
 * with a sliding sum inside groups of 4 (2 where N % 4 == 2) cells, keeps the x sum as a running sum that adds plane x + m and
 * removes plane x - m - 1 and restarts from a direct sum every x chunk of at most 64 planes, and adds along y directly: a sum
 * carries at most K = 6m + 134 roundings (filter.hip derives it).  A rounding of a sliding sum is relative to the window sum it is
 * made at: with A(i) = sum_W(i) |terms|, |error at (x, y, z)| <= K 2^-24 max A(x', y, z') over x' <= x in the chunk of x and z' <= z
 * in the group of z -- where the mass falls by many orders of magnitude within a chunk's planes, the sums of the faint region are
 * only that good.  Whether a box holds mass is decided EXACTLY (a count of the cells with mass != 0 is summed next to M, and
 * sums of ones are exact): a box without such a cell gives exact zeros in every channel, mbar included.  Sums of
 * integers below 2^24 are exact in any order.  The transfer function of the filter is prod_a sin((2m+1) k_a Lcell / 2) /
 * ((2m+1) sin(k_a Lcell / 2)).  tau_l is the stress of the GRIDDED field: on a particle-backed field it does not hold the
 * dispersion inside a cell, which stays VPS_SUBGRID_STRESS.
 * Taken by vps_field_algebra_out ALONE: VPS_FLAG_INPUT_IS_VM is required, out_dev [4 | 6][ncell] is required and must not overlap
 * chans_dev, ncell = N^3 for an even N >= 4, Lcell positive and finite (not otherwise used).  Whole grids only.  The call
 * allocates nothing: one launch on the context's stream, timed under VPS_K_ALGEBRA; every output element has one writer, no atomics.
 * VPS_ERR_ARG with a message naming the quantity, before anything is enqueued: the in-place vps_field_algebra or a null out_dev; a
 * null chans_dev; overlapping buffers; a buffer that is not 16-byte aligned; a call without VPS_FLAG_INPUT_IS_VM; any flag bit
 * other than VPS_FLAG_INPUT_IS_VM and the filter field; m == 0; 2m+1 > N; an ncell that is not the cube of an even N >= 4; an Lcell
 * that is not positive and finite; and the two codes on vps_deposit_field, vps_deposit_fft_zy, vps_deposit_fft_z[_slab]
 * (vps_deposit_fft_zy_supported returns 0) and vps_nn_resample_quantity.  VPS_ERR_UNSUPPORTED, before anything is enqueued: m > 8,
 * the largest half-width the kernel's LDS plan holds (the message names it); every 1 <= m <= 8 is taken at every even N >= 2m+2. */

/* ---- memory helpers (so the library is usable without torch) ------------ */
int vps_malloc(vps_ctx* ctx, void** dev, size_t bytes);
int vps_free(vps_ctx* ctx, void* dev);
int vps_memset(vps_ctx* ctx, void* dev, int value, size_t bytes);
int vps_memcpy_h2d(vps_ctx* ctx, void* dev, const void* host, size_t bytes); /* blocks */
int vps_memcpy_d2h(vps_ctx* ctx, void* host, const void* dev, size_t bytes); /* blocks */

/* ---- per-kernel timing (HIP events on the context's stream) -------------- */
/* When enabled every kernel launched by the library is bracketed by events.
 * vps_timing_get synchronises and returns, for kernel family `kind`, the launch
 * count and the summed duration in milliseconds since vps_timing_reset. */
enum vps_kernel_kind {
  VPS_K_DEPOSIT = 0, VPS_K_ALGEBRA = 1, VPS_K_FFT_Z = 2, VPS_K_FFT_Y = 3,
  VPS_K_FFT_X = 4, VPS_K_NN_BUILD = 5, VPS_K_NN_QUERY = 6, VPS_K_MISC = 7,
  /* exchange inside the library (vps_spectrum_zimages): one interval per kz chunk each --
   * EXCHANGE: the grouped ncclSend / ncclRecv of the chunk, on the communication stream;
   * EXCHANGE_WAIT: how long the context's stream stood still for it ahead of the chunk's x pass (the EXPOSED part) */
  VPS_K_EXCHANGE = 8, VPS_K_EXCHANGE_WAIT = 9,
  VPS_K_COUNT = 10
};
int vps_timing_enable(vps_ctx* ctx, int on);
int vps_timing_reset(vps_ctx* ctx);
int vps_timing_get(vps_ctx* ctx, int kind, int64_t* launches, double* total_ms);
/* per-launch durations (ms) of kind `kind` in launch order; *n_out = how many exist */
int vps_timing_list(vps_ctx* ctx, int kind, double* ms_out, int64_t cap, int64_t* n_out);

/* ---- stage A0: particle preprocessing ----------------------------------- */
/* In place on the device: coords[:,a] -= min(coords[:,a]) (scripts/parallel_optimized.py:280-282,
 * vpower/interp.py:169-175; exact in the dtype of pos) and v[:,a] -= sum(m v[:,a])/sum(m)
 * (script:285-289, interp.py:178-182; mean accumulated in float64, subtracted as float32).
 * min_out_host[3] / bulk_out_host[3] (may be NULL) receive what was subtracted.  Blocks. */
int vps_preprocess(vps_ctx* ctx, void* pos_dev, int pos_is_f64, float* vel_dev,
                   const float* mass_dev, int64_t np, int shift_to_origin,
                   int remove_bulk_velocity, double* min_out_host, double* bulk_out_host);

/* ---- conservation diagnostics -------------------------------------------- */
/* out_host[5] = sum m, sum m vx, sum m vy, sum m vz, sum m (vx^2+vy^2+vz^2), accumulated in float64:
 * the totals behind total_mass / total_momentum / total_kinetic_energy (x 0.5 on the host) of
 * GasParticles (vpower/interp.py:424-450) and BoxField (interp.py:639-666), i.e. check_conservation
 * (interp.py:1269-1319).  Component c of element i is v_dev[i*v_elem_stride + c*v_comp_stride]:
 * particles (vel [np][3]): strides 3, 1; a gridded field (chans [4][ncell] = vx,vy,vz,mass): strides 1, ncell
 * with mass_dev = chans + 3*ncell.  Blocks. */
int vps_totals(vps_ctx* ctx, const float* v_dev, int64_t v_elem_stride, int64_t v_comp_stride,
               const float* mass_dev, int64_t n, double out_host[5]);

/* ---- stage A1: nearest-grid-point deposition ---------------------------- */
/* Replaces deposit_to_grid (vpower/interp.py:996-1015).
 * Cell index per axis = int((pos // Lcell) % N) evaluated with numpy's
 * floor_divide/remainder algorithm in the dtype of pos (bit exact).
 * pos_dev: [np][3] float32 (pos_is_f64=0) or float64 (1).                        */
int vps_cell_index(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, int64_t np,
                   int N, double Lbox, int32_t* cell_dev /* [np][3] */);
/* Two-level bucket deposition (count -> scan -> scatter into per-brick buckets -> one
 * workgroup per brick accumulates in LDS and streams the tile out).
 * payload_dev: [np][C] float32, C in {1,3,4}.  grid_dev: [C][nx][N][N] float32 is
 * OVERWRITTEN: every cell of the slab is written exactly once (no memset needed);
 * particles whose x cell is outside [x0,x0+nx) are skipped.
 * work_dev: vps_deposit_workspace_bytes(np, C, N, nx) bytes of scratch.              */
size_t vps_deposit_workspace_bytes(int64_t np, int C, int N, int nx);
int vps_deposit_ngp(vps_ctx* ctx, const void* pos_dev, int pos_is_f64,
                    const float* payload_dev, int64_t np, int C,
                    int N, double Lbox, int x0, int nx, float* grid_dev, void* work_dev);
/* The fused hot-path form: deposits density_velocity_vector (interp.py:199-213) built on
 * the fly from vel_dev [np][3] and rho_dev [np], and applies the field algebra of
 * vps_field_algebra in the brick epilogue.  fields_dev: [ncomp][nx][N][N] float32,
 * ncomp = 3 (VPS_VELOCITY, VPS_MOMENTUM), 1 (VPS_ENERGY) or 4 (VPS_VM: vx,vy,vz,mass).
 * work_dev: vps_deposit_workspace_bytes(np, 4, N, nx).
 * With flags | VPS_FLAG_ASSIGN(order), order 2 (CIC) or 3 (TSC): the same fields of the CIC / TSC cell totals, on any x-slab.
 * The [rho v, rho] payload is deposited by the rule of vps_deposit_assign (below: its base cell, its six weight words, its
 * weights, the same expressions and rounding points), one sort record per particle, and the owner brick's epilogue turns the
 * four cell totals into the quantity (every quantity code; VPS_FLAG_REFERENCE_MOMENTUM_BUG as without the bits).  Only the
 * rows [x0, x0 + nx) are written, every cell exactly once by plain stores: no memset, no global float atomic.  Particles are
 * replicated -- every rank passes all np -- and no halo is exchanged: the sort is keyed by the brick geometry of the WHOLE
 * grid (that of vps_deposit_assign with C = 4), a particle none of whose `order` target rows lies in the slab is dropped by
 * its key, and the slab's bricks gather from their lower neighbours' buckets wherever those lie.
 * work_dev is then vps_deposit_assign_workspace_bytes(np, 4, N, order): the record arrays are sized for all np particles
 * although a rank of G keeps about np / G of them (a slab-sized workspace would need the particles compacted first).
 * Positions that are NaN, infinite or beyond 2^53 cells are skipped and any finite position wraps periodically, as in
 * vps_deposit_assign; np = 0 writes the quantity of an empty grid (zeros).  Timers: the sort under VPS_K_DEPOSIT, the
 * accumulation and epilogue under VPS_K_ALGEBRA.  The call stays a pure enqueue on the context's stream.
 * VPS_TOTAL_ENERGY, VPS_SUBGRID_ENERGY, VPS_DISPERSION (an addition within ABI 13; "Sub-grid velocity dispersion" above):
 * ncomp = 1, with and without VPS_FLAG_ASSIGN, the same sort records and the same workspaces; the brick's LDS tile carries a
 * fifth channel S2 = sum w rho_p |v_p|^2 (5 cells floats: 40 KiB, 80 KiB from N = 1024 on; VPS_ERR_UNSUPPORTED before anything
 * is enqueued where the context's LDS does not hold it), zeroed and streamed out with the other four.
 * VPS_SUBGRID_STRESS, VPS_DISPERSION_TENSOR ("Sub-grid stress tensor" above): ncomp = 6, one sort and two accumulation launches
 * with a 7-channel tile each. */
int vps_deposit_field(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                      const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx,
                      int quantity, int flags, float* fields_dev, void* work_dev);

/* The shortest form of stages A1 + A3 + the z and y passes of B (VPS_VELOCITY, VPS_MOMENTUM,
 * VPS_ENERGY; N in [64, 4096]): particle records are bucketed by "pencil" (one z-pass tile:
 * x, 16 y-lines, all z), each pencil is accumulated in LDS, turned into v = rho v / rho (or p, or
 * E = m |v|^2) and transformed along z without the real-space grid ever touching HBM; then the
 * y pass.  Outputs, per component c (3 for velocity / momentum, 1 for energy), the arrays
 * vps_fft_zy produces:
 *   spec_dev [ncomp][N/2][N][nx] complex64,  nyq_dev [ncomp][N][nx] complex64.
 * work_dev: vps_deposit_fft_zy_workspace_bytes(np, N, nx).                          */
int vps_deposit_fft_zy_supported(vps_ctx* ctx, int N, int quantity);
size_t vps_deposit_fft_zy_workspace_bytes_shared(int64_t np, int N, int nx);   /* ... with room for the fourth z image of VPS_FLAG_SHARE_ENERGY */
size_t vps_deposit_fft_zy_workspace_bytes(int64_t np, int N, int nx);
int vps_deposit_fft_zy(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                       const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx,
                       int quantity, int flags, void* spec_dev, void* nyq_dev, void* work_dev);

/* Higher-order assignment by expansion (extension): every particle becomes S = order^3 weighted
 * sub-particles at the centres of the cells it touches (order 2: cloud-in-cell, 3: triangular-shaped cloud; periodic):
 * pos_out_dev [np*S][3] float32, payload_out_dev [np*S][C] = payload * weight (C <= 4).  Depositing them with
 * vps_deposit_ngp gives the CIC / TSC grid; with replicated particles every slab gets its contributions without a halo. */
int vps_assign_expand(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* payload_dev, int64_t np,
                      int C, int N, double Lbox, int order, float* pos_out_dev, float* payload_out_dev);

/* Higher-order assignment, direct (ABI 13): the CIC / TSC grid of vps_assign_expand + vps_deposit_ngp from ONE record per
 * particle.  A particle is sorted (the two-level bucket sort of the NGP route) into the brick of its base cell c0 -- the lowest
 * cell it touches per axis: floor(s - 1/2) for CIC, floor(s) - 1 for TSC, s = (double)pos / (Lbox / N), periodic -- with a
 * record {cell-in-brick, payload[C], 6 weight words}: per axis two float32 numbers each rounded once from float64 (CIC 1 - f
 * and f; TSC a = 1/2 - d and b = 1/2 + d, the weights being a a / 2, 1/2 + a b, b b / 2), so that a small weight keeps its
 * relative precision.  The brick that OWNS a cell gathers: it walks its own bucket and those of the bricks holding the
 * order - 1 cells below its range on every axis (at most 8 buckets unless a partial last brick is narrower than that), adding
 * payload wx wy wz in LDS for the targets (c0 + j) mod N inside its own range.  Every (particle, offset) pair is counted
 * exactly once and grid_dev [C][N][N][N] float32 is OVERWRITTEN, every cell exactly once, by plain stores: no memset, no global
 * float atomic.  Sums agree with the expansion route up to float32 summation order.
 *   - the whole grid only (x0 = 0, nx = N), raw channels out (vps_field_algebra makes quantities of them); C in {1, 3, 4},
 *     order 2 (CIC) or 3 (TSC).  An x-slab of the QUANTITY fields of [rho v, rho] comes from vps_deposit_field with
 *     VPS_FLAG_ASSIGN(order); a slab of raw channels keeps the expansion route.
 *   - a position whose s is NaN or infinite, or beyond 2^53 cells, is SKIPPED (it deposits nowhere); positions any finite
 *     distance outside the box below that wrap periodically like the oracle's int64 %.
 *   - np = 0 writes zeros.  Bad np / N / Lbox / C / order and null buffers: VPS_ERR_ARG with a message.
 * work_dev: vps_deposit_assign_workspace_bytes(np, C, N, order) bytes (0: bad arguments): records of C + 7 words, twice, plus
 * 12 bytes of keys and ranks per particle -- against order^3 times the NGP workspace and 12 + 4 C bytes of expanded arrays per
 * sub-particle.  Timers: the sort under VPS_K_DEPOSIT, the accumulation under VPS_K_ALGEBRA, as in the NGP route. */
size_t vps_deposit_assign_workspace_bytes(int64_t np, int C, int N, int order);
int vps_deposit_assign(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* payload_dev, int64_t np, int C, int N,
                       double Lbox, int order, float* grid_dev, void* work_dev);
/* What vps_deposit_assign WOULD do (a pure host-side query like vps_deposit_plan).  out[] =
 *   0 bx, 1 by, 2 bz       cells of one brick per axis;  3 nbx, 4 nby, 5 nbz  bricks per axis (the last may be partial)
 *   6 nbuckets, 7 cells    bricks of the grid, cells per brick
 *   8 two_level            1: two-level sort, 0: one returning atomic per particle (option sort_atomic, or a geometry the
 *                          two-level sort does not cover)
 *   9 wide_keys            64-bit keys: nbuckets * cells does not fit 32 bits
 *   10 record_words        32-bit words of a record (C + 7)
 *   11 staged, 12 gshift   level-1 scatter staged in LDS; level-1 groups of 2^gshift buckets
 *   13 max_sources         the most source buckets any brick gathers from.
 * Tests aim particles with it. */
#define VPS_DEPOSIT_ASSIGN_PLAN_FIELDS 14
int vps_deposit_assign_plan(vps_ctx* ctx, int64_t np, int C, int N, int order, int64_t out[VPS_DEPOSIT_ASSIGN_PLAN_FIELDS]);

/* out_dev[np][4] = [vx*rho, vy*rho, vz*rho, rho]: GasParticles.density_velocity_vector
 * (vpower/interp.py:199-213).  vel_dev [np][3], rho_dev [np], float32.             */
int vps_density_velocity_vector(vps_ctx* ctx, const float* vel_dev, const float* rho_dev,
                                int64_t np, float* out_dev);

/* ---- stage A2: exact nearest-neighbour resampling ------------------------ */
/* Replaces ann_interpolate (vpower/interp.py:1018-1049; pyann k=1, eps=0) and the
 * per-cell Annoy query loop (scripts/parallel_optimized.py:337-358), as EXACT 1-NN:
 * squared distance ((qx-px)^2+(qy-py)^2)+(qz-pz)^2 in float64, lowest particle
 * index on exact ties.  Query lattice = qx_host[i] x qy_host[j] x qz_host[k]
 * (float64 host arrays, so both reference lattices are expressible: interp.py:1063
 * and parallel_optimized.py:343-345).  Only x rows [x0,x0+nx) of the lattice are
 * produced.  out_dev: [C][nx][nqy][nqz] float32 = payload of the NN;
 * nn_idx_dev (may be NULL): [nx][nqy][nqz] int32.
 * work_dev: vps_nn_workspace_bytes(np, pos_is_f64, nx*nqy*nqz) bytes of scratch (cell list, sorted
 * records, and the list of lattice points the scatter pass leaves to the exact fallback search).
 * Uniformly spaced axes (both reference lattices) take the particle-centric scatter search; any other
 * axes the query-centric ring search -- same results.                                             */
size_t vps_nn_workspace_bytes(int64_t np, int pos_is_f64, int64_t nq_slab);
int vps_nn_resample(vps_ctx* ctx, const void* pos_dev, int pos_is_f64,
                    const float* payload_dev, int64_t np, int C,
                    const double* qx_host, int nqx, const double* qy_host, int nqy,
                    const double* qz_host, int nqz, int x0, int nx,
                    float* out_dev, int32_t* nn_idx_dev, void* work_dev);
/* What the cell list of a search over np particles WOULD look like (ABI 10; a pure host-side query without a context, like
 * vps_nn_workspace_bytes: the geometry depends on np alone, and on the option nn_build_atomic).  out[] =
 *   0 M, 1 ncell           cells per axis of the list over the particles' bounding box, M^3
 *   2 sorted               1: two-level LDS bucket sort; 0: counting sort with one global atomic per particle (fewer than four
 *                          chunks, more groups than the sort covers, or option nn_build_atomic)
 *   3 gshift, 4 ngroups    level-1 groups of 2^gshift consecutive cells; 5 nchunks: level-1 chunks of particles
 *   6 lds_scatter, 7 lds_fine   bytes of dynamic LDS of the level-1 scatter and of the level-2 kernel (above 64 KiB the kernel's
 *                          limit is raised first); 0 when sorted = 0.
 * VPS_ERR_ARG: np < 1 or beyond int32 indices, or a null buffer. */
#define VPS_NN_PLAN_FIELDS 8
int vps_nn_plan(int64_t np, int pos_is_f64, int64_t nq_slab, int64_t out[VPS_NN_PLAN_FIELDS]);
/* What the last vps_nn_resample* call of this context ran (ABI 10; host-side, nothing is enqueued).  out[] =
 *   0 kind    VPS_NN_SEARCH_*: the ring search of non-uniform axes (or option nn_query_centric), the scatter kernel or the column
 *             kernel of uniform axes; -1: no search yet
 *   1 tiles   workgroups of that search kernel
 *   2 radii   1: the column kernel's per-tile radii were precomputed
 *   3 open    lattice points the scatter / column pass handed to the exact fallback (ring search: 0) -- read back only when the
 *             option nn_stats or the context's timing was on; -1 otherwise. */
enum { VPS_NN_SEARCH_RING = 0, VPS_NN_SEARCH_SCATTER = 1, VPS_NN_SEARCH_COLUMN = 2 };
int vps_nn_last_search(vps_ctx* ctx, int64_t out[4]);

/* The same search with the algebra of GasParticles.ann_interp_to_field (vpower/interp.py:272-273) in its epilogue:
 * rhov_dev [np][4] = density_velocity_vector; out_dev [4][nx][nqy][nqz] = vx, vy, vz (= rho v / rho of the nearest
 * particle) and mass (= rho * Lcell^3): the BoxField form, without a separate pass over the grid. */
int vps_nn_resample_field(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* rhov_dev,
                          int64_t np, const double* qx_host, int nqx, const double* qy_host, int nqy,
                          const double* qz_host, int nqz, int x0, int nx, double Lcell,
                          float* out_dev, int32_t* nn_idx_dev, void* work_dev);

/* ... and with the algebra of BoxField.spctrm's quantity as well (interp.py:501-557): out_dev [ncomp][nx][nqy][nqz] holds what
 * the spectrum of `quantity` transforms -- VPS_VELOCITY: v (3 channels); VPS_MOMENTUM: p = v * mass (3; with
 * VPS_FLAG_REFERENCE_MOMENTUM_BUG py = pz = px, interp.py:523-525); VPS_ENERGY: E = mass |v|^2 (1); VPS_VM: v and mass (4, =
 * vps_nn_resample_field); VPS_DENSITY / VPS_LOG_DENSITY (ABI 11): rho^alpha / ln rho of the nearest particle's density (1)
 * -- v = rho v / rho and mass = rho Lcell^3 of the nearest particle, rounded as the reference rounds them.
 * For `ann_interp_to_field(N).spctrm(q)`: no fourth channel is written and the z pass reads one array per component. */
int vps_nn_resample_quantity(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* rhov_dev,
                             int64_t np, const double* qx_host, int nqx, const double* qy_host, int nqy,
                             const double* qz_host, int nqz, int x0, int nx, double Lcell, int quantity, int flags,
                             float* out_dev, int32_t* nn_idx_dev, void* work_dev);

/* ---- stage A3: field algebra ------------------------------------------- */
/* chans_dev: [4][ncell] = rho*vx, rho*vy, rho*vz, rho (density_velocity_vector,
 * interp.py:199-213, after deposit/resample).  In place:
 *   VPS_VELOCITY: chans[0..2] = rho v / rho, 0 where rho==0 (interp.py:272, NaN->0
 *                 as interp.py:329-331);
 *   VPS_MOMENTUM: chans[0..2] = v * (rho*Lcell^3)            (interp.py:273,523-525);
 *   VPS_ENERGY  : chans[0]    = (rho*Lcell^3)*(vx^2+vy^2+vz^2) (interp.py:546);
 *   VPS_VM      : chans[0..2] = v, chans[3] = rho*Lcell^3   (BoxField, interp.py:272-275);
 *   VPS_DENSITY / VPS_LOG_DENSITY (ABI 11): chans[0] = rho^alpha / ln rho, from channel 3 alone (above).
 * With VPS_FLAG_INPUT_IS_VM the channels are taken as vx,vy,vz,mass instead (the density codes: rho = mass / Lcell^3). */
int vps_field_algebra(vps_ctx* ctx, int quantity, int flags, double Lcell,
                      float* chans_dev, int64_t ncell);
/* Out-of-place form: chans_dev is only read, the result's channels (3: velocity / momentum, 1: energy,
 * 4: VM) go to out_dev[c][ncell]; out_dev == NULL is the in-place call above.
 * VPS_FILTERED_VM / VPS_FILTERED_STRESS ("Box-filtered fields" above): this form only, ncell = N^3 a whole grid, the half-width
 * in VPS_FLAG_FILTER(m).
 * VPS_DIVERGENCE / VPS_VORTICITY / VPS_STRAIN_RATE ("Velocity-gradient fields" above): this form only, ncell = N^3 a whole grid
 * of [v, mass] channels, 1 / 3 / 6 output channels. */
int vps_field_algebra_out(vps_ctx* ctx, int quantity, int flags, double Lcell, const float* chans_dev,
                          int64_t ncell, float* out_dev);

/* ---- stage B+C: 3-D R2C FFT, |f|^2, shell binning ------------------------ */
/* Supported N: powers of two, 16 <= N <= 4096; 96, 192, 384, 768, 1536 (radix 3 / 6 / 12 / 24);
 * 250, 500, 1000, 2000 (radix 5 / 10 / 20).                                          */
int vps_fft_supported(int N);
/* Binning tables (host pointers, copied):
 *   k2_axis[N]   = fl(k*k) for k = 2*pi*fftfreq(N, Lcell)   (interp.py:1449,1460)
 *   thr[nbins+1] : thr[i] = smallest double t with fl(sqrt(t)) >= edge[i] (i<nbins),
 *                  thr[nbins] = smallest t with fl(sqrt(t)) > edge[nbins]; so that
 *                  thr[i] <= s < thr[i+1]  <=>  edge[i] <= sqrt(s) < edge[i+1] with the
 *                  last bin right-closed, i.e. numpy.histogram's rule
 *                  (interp.py:1474-1477, parallel_optimized.py:181-182).
 *   edge0, inv_spacing: a first guess b=(sqrt(s)-edge0)*inv_spacing, corrected with thr. */
int vps_set_binning(vps_ctx* ctx, int N, const double* k2_axis_host,
                    const double* thr_host, int nbins, double edge0, double inv_spacing);

/* Binning-only consumers: while `on`, the y passes (vps_fft_zy, vps_fft_zy_weighted, vps_deposit_fft_zy, vps_fft_y) do
 * not store rows (ky, kz) all of whose modes lie beyond the last shell edge of the current vps_set_binning tables --
 * fl(ky^2 + kz^2) >= thr[nbins]; with the default k range a fifth of the half spectrum -- and leave that memory untouched;
 * the binning x passes (vps_fft_x modes 0 / 3, vps_fft_x_bin) never read them.  Switch it off (the default) before any
 * call whose output is read in full (vps_fft_x modes 1, 2; vps_rfft3 and vps_power_grid do so themselves). */
int vps_set_bin_only(vps_ctx* ctx, int on);

/* Deconvolution of a mass-assignment window in the binning x pass (extension; the reference has no
 * higher-order assignment): inv_w2_axis_host[N] (float32, indexed like k2_axis, even in k) holds 1 / W(k)^2 of ONE axis,
 * W(k) = sinc(pi k / (2 k_Nyquist))^p with p = 1 (NGP), 2 (CIC), 3 (TSC); every |F(k)|^2 that vps_fft_x (modes 0, 3) and
 * vps_fft_x_bin accumulate is multiplied by the product of the three axis factors.  NULL switches it off (default). */
int vps_set_window(vps_ctx* ctx, int N, const float* inv_w2_axis_host);

/* Local part of the transform on an x-slab: z pass (R2C) and y pass.
 * field_dev: [nx][N][N] float32 real input (NOT modified).
 * spec_dev : [N/2][N][nx] complex64 = F_zy[kz][ky][x]   (kz < N/2)
 * nyq_dev  : [N][nx]      complex64 = F_zy[kz=N/2][ky][x]
 * work_dev : vps_fft_workspace_bytes(N,nx) bytes.
 * nx must be a multiple of 16 (or equal to N when N < 16... see vps_fft_supported). */
size_t vps_fft_workspace_bytes(int N, int nx);
int vps_fft_zy(vps_ctx* ctx, int N, int nx, const float* field_dev,
               void* spec_dev, void* nyq_dev, void* work_dev);
/* The same for the product field_dev * weight_dev (cell by cell; weight_dev NULL = vps_fft_zy): momentum
 * components v_c * mass of a gridded field (interp.py:523-525) without a separate algebra pass. */
int vps_fft_zy_weighted(vps_ctx* ctx, int N, int nx, const float* field_dev, const float* weight_dev,
                        void* spec_dev, void* nyq_dev, void* work_dev);

/* The same two passes as separate calls, for the chunked slab exchange of several ranks (G = number of x-slabs):
 *   vps_fft_z          z pass of field_dev (* weight_dev if not NULL) into a z image zimg_dev
 *                      (vps_fft_zimage_bytes(N, nx) bytes: B[x][kz][y], kz < N/2, followed by the Nyquist plane BN[x][y]);
 *   vps_deposit_fft_z  the fused deposit + field algebra + z pass of vps_deposit_fft_zy, stopping there: ncomp z images
 *                      (3: velocity / momentum, 1: energy) in zimg_dev; work_dev: vps_deposit_fft_z_workspace_bytes;
 *   vps_fft_y          y pass of chunk `chunk` of `nchunks` of a z image.  The kz < N/2 planes are cut into nchunks BANDS
 *                      of G*nkc planes (nkc = N/2/G/nchunks) and dealt out round-robin inside a band: slot j of rank h is
 *                      plane chunk*G*nkc + j*G + h (every rank gets planes of every |kz|, and the j-th planes of all ranks
 *                      are neighbours).  They are transformed and written as ONE send buffer for an equal-split all-to-all,
 *                      out_dev = [h][ slot 0 rows | slot 1 rows | ... | -- last chunk only -- Nyquist rows
 *                      F_zy[N/2][ky in rank h's N/G rows][x] (N/G*nx) ], each row nx complex64.  A slot holds all N rows of
 *                      its plane (row = ky), or -- inside a binning-only scope (vps_set_bin_only), vps_fft_y_packed() = 1
 *                      -- only the 2 kc + 1 rows |ky| <= kc that the slot's planes can still contribute to a shell (row ky
 *                      at position ky, row N - i at position 2 kc + 1 - i), so the rows nobody bins do not cross the node
 *                      either.  One destination's block is vps_fft_y_chunk_block(ctx, ..., packed) elements,
 *                      vps_fft_y_chunk_elems(...) (all rows, all G blocks) an upper bound of the whole buffer.  After the
 *                      exchange the G blocks a rank received (x running over the senders' slabs) go to
 *                      vps_fft_x_bin_chunk with the same `packed`.
 * This replaces the four allgathers per buffer flush of scripts/parallel_optimized.py:365-368 with one message per
 * scalar field (or several chunks of it, so that the exchange of one chunk overlaps the passes of its neighbours). */
size_t vps_fft_zimage_bytes(int N, int nx);
int vps_fft_z(vps_ctx* ctx, int N, int nx, const float* field_dev, const float* weight_dev, void* zimg_dev);
size_t vps_deposit_fft_z_workspace_bytes(int64_t np, int N, int nx);
int vps_deposit_fft_z(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                      const float* rho_dev, int64_t np, int N, double Lbox, int x0, int nx,
                      int quantity, int flags, void* zimg_dev, void* work_dev);
/* Ranks that hold a REPLICATED particle set but deposit one x-slab of it (scripts/parallel_optimized.py:272-276 loads the whole
 * snapshot on every rank): the sort workspace sized for the particles INSIDE the slab instead of all np --
 *   vps_count_in_slab                       that number, with the deposit's own bit-exact cell rule (one pass over the
 *                                           positions, blocks; < 0: error);
 *   vps_deposit_fft_z_workspace_bytes_slab  workspace for np particles of which at most np_slab lie in the slab: no per-input
 *                                           key array, compact {key, payload} and record arrays of np_slab entries (C5 on 8
 *                                           ranks: 52 GB -> 9 GB); the slab's particles are filtered into them by one pass
 *                                           over the positions, the sort runs on the compact arrays only;
 *   vps_deposit_fft_z_slab                  vps_deposit_fft_z on such a workspace; VPS_ERR_ARG if the slab holds more particles
 *                                           than the workspace has room for (np_slab + the filter pass's block slack; checked
 *                                           before anything is written past it). */
int64_t vps_count_in_slab(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, int64_t np, int N, double Lbox, int x0, int nx);
size_t vps_deposit_fft_z_workspace_bytes_slab(int64_t np, int64_t np_slab, int N, int nx);
int vps_deposit_fft_z_slab(vps_ctx* ctx, const void* pos_dev, int pos_is_f64, const float* vel_dev,
                           const float* rho_dev, int64_t np, int64_t np_slab, int N, double Lbox, int x0, int nx,
                           int quantity, int flags, void* zimg_dev, void* work_dev);
/* What the bucket sort of a deposit WOULD do (ABI 9; a pure host-side query like vps_fft_y_chunk_block: nothing is enqueued or
 * allocated): the bucket geometry and the sort's code path for np particles with C channels on the slab [x0, x0 + nx) of an N^3
 * grid, under the current options and the context's LDS size.  pencil = 0: the bricks of vps_deposit_ngp / vps_deposit_field
 * (C = 4); pencil = 1: the pencils of vps_deposit_fft_zy / vps_deposit_fft_z (C = 4 only); np_slab >= 0: the slab-sized
 * workspace of vps_deposit_fft_z_slab (pencils only), < 0: none.  out[] =
 *   0 bx, 1 by, 2 bz       cells of one bucket per axis
 *   3 nbuckets, 4 cells    buckets of the slab, cells per bucket; 5: cells is a power of two (shift instead of divide)
 *   6 two_level            1: two-level sort, 0: one returning atomic per particle (option sort_atomic, or more buckets than
 *                          the two-level sort covers)
 *   7 wide_keys            64-bit keys: nbuckets * cells does not fit 32 bits
 *   8 gshift, 9 ngroups    level-1 groups of 2^gshift buckets; 10 nchunks: level-1 chunks (table = ngroups * nchunks entries)
 *   11 staged              level-1 scatter staged in LDS, which takes 12 staged_lds bytes of dynamic LDS (above 64 KiB the
 *                          kernel's limit is raised first)
 *   13 recompute           the slab's particles are compacted before the sort (np_slab given and worth it)
 *   14 cap_in              entries of the key / record arrays.
 * Tests use it to prove which path a case took. */
#define VPS_DEPOSIT_PLAN_FIELDS 15
int vps_deposit_plan(vps_ctx* ctx, int64_t np, int C, int N, int x0, int nx, int pencil, int64_t np_slab,
                     int64_t out[VPS_DEPOSIT_PLAN_FIELDS]);
int64_t vps_fft_y_chunk_elems(int N, int nx, int G, int nchunks, int chunk);   /* -1: G, nchunks do not divide */
int vps_fft_y_packed(vps_ctx* ctx, int N);   /* 1: vps_fft_y packs rows now (binning-only scope with a row cut for N) */
int64_t vps_fft_y_chunk_block(vps_ctx* ctx, int N, int nx, int G, int nchunks, int chunk, int packed);   /* pure size query (host tables only). -1: bad arguments, -2: G x nchunks does not divide N/2, -3: packed without a row cut (vps_last_error says which) */
int vps_fft_y(vps_ctx* ctx, int N, int nx, const void* zimg_dev, int G, int nchunks, int chunk, void* out_dev);

/* x pass over `nlines` lines of length N.  Line i is made of nseg segments of
 * N/nseg contiguous complex64: element x of line i lives at
 *   in_dev[(x / seglen) * seg_stride + i * seglen + (x % seglen)],  seglen = N/nseg
 * (nseg=1: plain contiguous lines; nseg=G: the layout an all-to-all of G x-slabs
 * leaves behind).  Line i has global mode indices ky = (line0+i) % N and
 * kz = kz0 + (line0+i)/N.
 * mode 0: accumulate w*|F|^2 (w = 1 for kz in {0,N/2}, else 2) into
 *         psum_dev[nbins] (float64) and w into nsample_dev[nbins] (uint64) using
 *         the tables of vps_set_binning;  replaces _pair_power+_hist_sample
 *         (interp.py:1440-1482) / pair_power+hist_sample (parallel_optimized.py:145-190).
 * mode 3: as mode 0 but shell sums only (nsample_dev untouched): the counts depend on the
 *         mode lattice alone, so a vector spectrum counts once, on its first component.
 * mode 4: transform and discard (a timing aid: the pass without its epilogue).
 * mode 1: write the transformed lines to out_dev[i][kx] (complex64, contiguous).
 * mode 2: out_dev[i][kx] (float32) += |F|^2, no binning (component sums of
 *         _vector_power, interp.py:1386).
 * Real-space two-point statistics (an addition within ABI 13: no new symbol).  The power grid of a real field is real and
 * even, so its FORWARD transform is N^3 times the autocorrelation: no inverse transform exists or is needed.  Three modes,
 * whole lines of whole grids only -- nseg must be 1, else VPS_ERR_ARG before anything is enqueued:
 * mode 5: as mode 2, but out_dev is the BASE of a full [N][N][N] float32 grid indexed [kz][ky][kx], whatever line0 / kz0:
 *         the line (ky, kz), 0 <= kz <= N/2, adds |F(kx)|^2 at [kz][ky][kx] and, for 0 < kz < N/2, the same value at the
 *         Hermitian partner [N-kz][(N-ky)%N][(N-kx)%N].  The planes kz = 0 and N/2 write no mirror: their partners are
 *         lines of the same plane.  One writer per element and call, plain +=: the caller zeroes the grid, the components
 *         of a vector field accumulate over calls.  The result is a real field that vps_fft_zy accepts.  Like modes 1 and
 *         2 it reads every row: run the y pass outside a binning-only scope.  A kz range outside 0..N/2: VPS_ERR_ARG.
 * mode 6: the binning of mode 0 with w*Re F(kx) accumulated into psum_dev where mode 0 accumulates w*|F|^2, and w into
 *         nsample_dev; the imaginary part is ignored.  Tables (vps_set_binning: for a correlation function the axis table
 *         is fl(r*r), r = Lcell * min(i, N - i), the thresholds those of the r edges), multiplicity w, shell decision
 *         (vps_binning_mode), +-kx / +-ky pairing, row cut and float64 accumulation are those of mode 0.
 * mode 7: as mode 6, shell sums only (nsample_dev untouched), as mode 3 is to mode 0.
 *         Modes 6 / 7 return VPS_ERR_ARG before anything is enqueued while a window is set (vps_set_window: a k-space
 *         window on an r lattice is a caller's error) and for a null accumulator.  vps_fft_x_bin*, vps_spectrum_zimages
 *         and the chunked exchange do not take modes 5..7.  Any other mode: VPS_ERR_ARG ("mode must be 0..7").   */
int vps_fft_x(vps_ctx* ctx, int N, int64_t nlines, int64_t line0, int kz0,
              const void* in_dev, int nseg, int64_t seg_stride, int mode,
              double* psum_dev, unsigned long long* nsample_dev, void* out_dev);

/* Binning x pass of a VECTOR field: the ncomp (1..3) component spectra in_devs[c] (same layout and
 * arguments as vps_fft_x) are transformed line by line, their |F|^2 SUMMED, and the sum binned once
 * (mode 0 when count != 0, else mode 3) -- the component sum of _vector_power (interp.py:1386,
 * parallel_optimized.py:131-137) fused with _pair_power/_hist_sample.  in_devs is a HOST array of
 * device pointers. */
int vps_fft_x_bin(vps_ctx* ctx, int N, int64_t nlines, int64_t line0, int kz0,
                  const void* const* in_devs, int ncomp, int nseg, int64_t seg_stride, int count,
                  double* psum_dev, unsigned long long* nsample_dev);
/* Binning x pass of ONE received chunk of the slab exchange (layout: vps_fft_y): in_devs[c] = the G blocks this rank
 * received for component c, `packed` what the senders' vps_fft_y_packed() returned; count as in vps_fft_x_bin.  The last
 * chunk's Nyquist-plane rows are binned by the same call.
 * Rank-count limit: a received x line is G segments of nx = N / G points, and the x pass of the N = 1024, 2048, 4096 lines
 * (64, 128, 256 lanes per line) needs segments of at least one point per lane -- at most 16 ranks at those sizes; every
 * other N takes any G that divides N / 2.  More ranks: VPS_ERR_UNSUPPORTED at the entry of this call and of
 * vps_spectrum_zimages, before anything is enqueued. */
int vps_fft_x_bin_chunk(vps_ctx* ctx, int N, int nx, int G, int nchunks, int chunk, int rank, int packed,
                        const void* const* in_devs, int ncomp, int count, double* psum_dev,
                        unsigned long long* nsample_dev);

/* Helmholtz decomposition of a VECTOR field (ABI 7): vps_fft_x_bin / vps_fft_x_bin_chunk with the same arguments and one more
 * float64 accumulator, psum_comp_dev[nbins], into which the COMPRESSIVE (curl-free) part of every mode is binned with the
 * same shell decision, Hermitian multiplicity and window factor as its |F|^2:
 *     |D|^2 / |k'|^2,  D = k'x Fx + k'y Fy + k'z Fz   (0 where k' = 0),
 * k' = the integer mode numbers fftfreq(N) * N of each axis with the Nyquist entry N/2 set to 0 (odd under k -> -k, so that
 * a mode and its Hermitian partner get the same projection).  psum_dev / nsample_dev take exactly what vps_fft_x_bin adds
 * to them; the solenoidal part is psum_dev - psum_comp_dev (the axis-Nyquist modes, k' = 0, count as solenoidal).
 * in_devs[0..2] are the x, y, z components (x = the line axis, y = the row, z = the halved axis); ncomp must be 3 (else
 * VPS_ERR_ARG).  The chunk form has the rank-count limit of vps_fft_x_bin_chunk, refused at its entry. */
int vps_fft_x_bin_helmholtz(vps_ctx* ctx, int N, int64_t nlines, int64_t line0, int kz0,
                            const void* const* in_devs, int ncomp, int nseg, int64_t seg_stride, int count,
                            double* psum_dev, unsigned long long* nsample_dev, double* psum_comp_dev);
int vps_fft_x_bin_chunk_helmholtz(vps_ctx* ctx, int N, int nx, int G, int nchunks, int chunk, int rank, int packed,
                                  const void* const* in_devs, int ncomp, int count, double* psum_dev,
                                  unsigned long long* nsample_dev, double* psum_comp_dev);

/* ---- slab exchange inside the library: RCCL over xGMI (one process per GPU) -------------------------------------------
 * For hosts without a collective of their own (the Python host drives the same chunk pipeline through torch.distributed,
 * vpower/device.py).  Replaces the four comm.allgather per buffer flush and the two comm.Reduce of
 * scripts/parallel_optimized.py:365-368, 455-456.  RCCL is loaded at run time (dlopen): VPS_ERR_UNSUPPORTED without it.
 *   vps_comm_unique_id    rank 0: 128 bytes for the host to hand to every rank (ncclGetUniqueId)
 *   vps_comm_create       every rank, collectively: ncclCommInitRank on the context's device + a communication stream
 *   vps_spectrum_zimages  the x-side of the transform of ncomp (1..3) z images (vps_fft_z / vps_deposit_fft_z[_slab]) of this
 *                         rank's slab, nx = N / world: per kz chunk the y passes into the send buffers, ONE grouped
 *                         ncclSend / ncclRecv exchange per chunk on the communication stream, the binning x pass of the
 *                         received blocks (component |F|^2 summed before the shell search) -- all y passes are enqueued
 *                         first, so chunk c travels while c + 1 is transformed and is binned while c + 1 travels.  Needs the
 *                         tables of vps_set_binning; blocks carry only the rows a shell can reach.  Accumulates into
 *                         psum_dev / (count != 0) nsample_dev; xwork_dev: vps_spectrum_zimages_workspace_bytes.
 *                         At most 16 ranks for N = 1024, 2048, 4096 (vps_fft_x_bin_chunk): refused before any enqueue.
 *   vps_allreduce_shells  sum of the accumulators over the ranks (ncclAllReduce, float64 + uint64), on the context's stream */
int vps_comm_unique_id(char* id128);
int vps_comm_create(vps_ctx* ctx, int rank, int world, const char* id128);
int vps_comm_destroy(vps_ctx* ctx);
int vps_comm_info(vps_ctx* ctx, int* rank, int* world);
size_t vps_spectrum_zimages_workspace_bytes(int N, int nx, int G, int nchunks, int ncomp);
int vps_spectrum_zimages(vps_ctx* ctx, int N, int nx, const void* const* zimg_devs, int ncomp, int nchunks, void* xwork_dev,
                         int count, double* psum_dev, unsigned long long* nsample_dev);
int vps_allreduce_shells(vps_ctx* ctx, double* psum_dev, unsigned long long* nsample_dev, int nbins);

/* Single-GPU convenience: full |F(k)|^2 binning of one real field.
 * field_dev [N][N][N] float32 is preserved; work_dev: vps_power_workspace_bytes(N). */
size_t vps_power_workspace_bytes(int N);
int vps_power_bin(vps_ctx* ctx, int N, const float* field_dev, void* work_dev,
                  double* psum_dev, unsigned long long* nsample_dev);
/* Single-GPU half spectrum for the un-binned API (_vector_power/_scalar_power,
 * interp.py:1372-1421): out_dev [N/2+1][N][N] complex64 = F[kz][ky][kx].          */
int vps_rfft3(vps_ctx* ctx, int N, const float* field_dev, void* work_dev, void* out_dev);
/* Same transform, but power_dev [N/2+1][N][N] float32 += |F[kz][ky][kx]|^2 (caller zeroes
 * it; several components accumulate): the un-binned P grid of _vector_power.       */
int vps_power_grid(vps_ctx* ctx, int N, const float* field_dev, void* work_dev, float* power_dev);

/* ---- un-fused binning API (not on the hot path) --------------------------- */
/* out_dev[N^3] float64 = sqrt(kx*kx + ky*ky + kz*kz) over the meshgrid of the host axes,
 * C order 'ij': column 0 of _pair_power (interp.py:1449-1462); the three axes are
 * separate so that the per-axis shift of interp.py:1453-1458 can be applied.        */
int vps_pair_k(vps_ctx* ctx, int N, const double* kx_host, const double* ky_host,
               const double* kz_host, double* out_dev);
/* numpy.histogram(k, bins=edges, weights=w) and the unweighted counts in one pass:
 * edges[i] <= k < edges[i+1], last bin right-closed (interp.py:1474-1477).
 * k_dev, w_dev: float64[n] (w_dev may be NULL: weights 1); edges_host[nbins+1];
 * psum_dev float64[nbins] and nsample_dev uint64[nbins] are accumulated into.  Blocks.
 * A workgroup keeps the edges and its whole histogram in LDS, 20 nbins + 8 bytes: nbins is admitted up to
 * vps_hist_max_bins(ctx) (ABI 12) = (LDS bytes a workgroup of the device can have - 8) / 20 -- 8191 with 160 KiB, 3276 with
 * 64 KiB -- and refused beyond it with VPS_ERR_ARG and a message naming that value, before anything is enqueued. */
int vps_hist_max_bins(vps_ctx* ctx);
int vps_hist_pairs(vps_ctx* ctx, const double* k_dev, const double* w_dev, int64_t n,
                   const double* edges_host, int nbins, double* psum_dev,
                   unsigned long long* nsample_dev);

#ifdef __cplusplus
}
#endif
#endif /* VPS_HIP_H */
