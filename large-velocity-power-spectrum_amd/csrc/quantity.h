// What a quantity (include/vps_hip.h: vps_quantity) is, once: its channels, whether it is a scalar of rho, whether it needs the
// exponent of vps_set_density_weight -- and the two functions of rho that the density-weighted velocity and the scalar density
// quantities are made of.  Shared by the brick / grid epilogues (deposit.hip), the NN emit (nn.hip) and the pencil kernel
// (fft_pencil.h).  A new quantity starts here: its code in these five helpers, then its per-cell body in deposit.hip's cell_quantity.
// (The velocity-gradient codes are no per-cell algebra: a stencil over a whole grid, gradient.hip -- vps_quantity_gradient.
//  Nor are the box-filter codes: sums over a box of cells of a whole grid, filter.hip -- vps_quantity_filter.)
// Not part of the ABI.
#pragma once
#include "../../include/vps_hip.h"

// (15 is no code: include/vps_hip.h keeps it unassigned)
constexpr bool vps_quantity_valid(int q) {
  return (q >= VPS_VELOCITY && q <= VPS_STRAIN_RATE) || q == VPS_FILTERED_VM || q == VPS_FILTERED_STRESS;
}
// one output field, made from rho alone (channel 3 of [rho v, rho])
constexpr bool vps_quantity_scalar_rho(int q) { return q == VPS_DENSITY || q == VPS_LOG_DENSITY; }
// one output field that needs the second moment S2 = sum w rho_p |v_p|^2 next to the four cell totals: a fifth tile channel in
// the deposit kernels (vps_deposit_field), nothing a 4-channel grid, one nearest particle or the pencil kernel can give -- every
// other entry point refuses these codes (vps_refuse_second_moment)
constexpr bool vps_quantity_second_moment(int q) { return q >= VPS_TOTAL_ENERGY && q <= VPS_DISPERSION_TENSOR; }
// ... of which the two TENSOR quantities keep the six sums S_ij = sum w rho_p v_i v_j instead of their trace: six output fields
// (xx, yy, zz, xy, xz, yz), formed by TWO accumulation launches over the one sort's records -- the diagonal half and the
// off-diagonal half, each with three second-moment tile channels behind the four totals and three output fields
constexpr bool vps_quantity_tensor(int q) { return q == VPS_SUBGRID_STRESS || q == VPS_DISPERSION_TENSOR; }
// fields of central differences of a gridded velocity (divergence: 1 field; vorticity: 3; strain rate: 6, in the tensor order):
// a cell's value needs its six neighbours, which only a whole periodic grid of [v, mass] channels holds -- formed by
// vps_field_algebra_out alone (gradient.hip), every other entry point refuses these codes (vps_refuse_grid_only); no deposit, NN
// or pencil kernel is instantiated for them (deposit.hip: dispatch_quantity does not know them)
constexpr bool vps_quantity_gradient(int q) { return q >= VPS_DIVERGENCE && q <= VPS_STRAIN_RATE; }
// box sums of a whole grid's [u, mass] channels at a half-width of VPS_FLAG_FILTER: the filtered [v, mass] grid (4 fields) and the
// sub-filter stress (6, in the tensor order) -- formed by vps_field_algebra_out alone (filter.hip); refused everywhere else with
// the gradient codes, and no deposit, NN or pencil kernel is instantiated for them
constexpr bool vps_quantity_filter(int q) { return q == VPS_FILTERED_VM || q == VPS_FILTERED_STRESS; }
constexpr int vps_quantity_channels(int q) {
  return q == VPS_FILTERED_VM ? 4 : q == VPS_FILTERED_STRESS ? 6 : q == VPS_DIVERGENCE ? 1 : q == VPS_VORTICITY ? 3 : q == VPS_STRAIN_RATE ? 6 :
         q == VPS_VM ? 4 : vps_quantity_tensor(q) ? 6 :
         (q == VPS_ENERGY || vps_quantity_scalar_rho(q) || vps_quantity_second_moment(q)) ? 1 : 3;
}
// second-moment channels of ONE launch's LDS tile: the trace, or one half of the tensor
constexpr int vps_quantity_moment_channels(int q) { return vps_quantity_tensor(q) ? 3 : vps_quantity_second_moment(q) ? 1 : 0; }
// reads the context's alpha: VPS_ERR_ARG where it was never set (api.hip: vps_check_weighted)
constexpr bool vps_quantity_needs_alpha(int q) { return q == VPS_WEIGHTED_VELOCITY || q == VPS_DENSITY; }

#if defined(__HIPCC__)
// rho^a for rho > 0: exp2(a log2 rho) on the transcendental units (v_log_f32, v_exp_f32) with rho's binary exponent taken out
// first -- rho = m 2^e, m in [0.5, 1), so a log2 rho = n + (a e - n) + a log2 m with n = rint(a e): the logarithm's result and
// the argument of exp2 stay of order 1, where one ulp is 6e-8, instead of carrying one ulp of |log2 rho| (1e-6 at 2^13) into the
// exponent.  A positive field has a mean: a one-sided ulp of the straight form times that mean was 7e-6 of the rms in the
// thin-slab images.
__device__ __forceinline__ float vps_rho_pow(float r, float a) {
  const float e = (float)__builtin_amdgcn_frexp_expf(r);
  const float n = __builtin_rintf(a * e);
  const float f = __builtin_fmaf(a, e, -n) + a * __builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(r));
  return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(f), (int)n);
}

// Each function comes as its value for rho != 0 (_nz) and with the rule for empty cells -- 0 whatever the exponent is, the
// NaN -> 0 rule of interp.py:329-331 -- on top.  The pencil kernel and the gridded-field form of the weighted velocity select
// on a condition of their own and take the _nz form.  So does the density arm of the NN emit (nn.hip: nn_form_apply), which
// makes vps_rho_scalar's two selects in an order of its own, by hand (as its log-density arm keeps its own guard): the guarded vps_rho_scalar is the ONE copy for the brick and
// grid epilogues only, the _nz cores are the one copy of the arithmetic for every route.

// The weight factor rho^e of the density-weighted velocity (e = alpha - 1 on [rho v, rho] channels): the straight
// exp2(e log2 rho), one multiply between the two transcendentals.
__device__ __forceinline__ float vps_rho_weight_nz(float rho, float e) {
  return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(rho));
}
__device__ __forceinline__ float vps_rho_weight(float rho, float e) { return rho != 0.f ? vps_rho_weight_nz(rho, e) : 0.f; }

// The scalar density quantities: ln rho = log2 rho * ln 2 (VPS_LOG_DENSITY) or rho^alpha (VPS_DENSITY; alpha = 1 is rho itself,
// no transcendental: the pencil route settles that case on the host and never asks).
__device__ __forceinline__ float vps_rho_scalar_nz(float rho, bool log, float alpha) {
  return log ? __builtin_amdgcn_logf(rho) * 0.693147180559945309f : vps_rho_pow(rho, alpha);
}
__device__ __forceinline__ float vps_rho_scalar(float rho, int quantity, float alpha) {
  if (quantity == VPS_LOG_DENSITY) return rho != 0.f ? vps_rho_scalar_nz(rho, true, alpha) : 0.f;
  if (alpha == 1.f) return rho;
  return rho != 0.f ? vps_rho_scalar_nz(rho, false, alpha) : 0.f;
}
#endif
