// Complex arithmetic on (re, im) register pairs and the small DFTs (radix 2 .. 24) that the line transforms of fft_line.h
// are made of.
#pragma once
#include "fft_params.h"   // cf

namespace {

typedef float vps_f4 __attribute__((ext_vector_type(4)));

// (written on whole (re, im) pairs: the compiler then keeps a complex value in one aligned register pair and maps these
// onto v_pk_add / v_pk_mul / v_pk_fma with operand-select modifiers; the component-wise form was re-vectorised across
// DIFFERENT values and paid for it in register moves -- a fifth of the VALU instructions of the 2048-point passes)
__device__ __forceinline__ cf cadd(cf a, cf b) { return a + b; }
__device__ __forceinline__ cf csub(cf a, cf b) { return a - b; }
__device__ __forceinline__ cf cmul(cf a, cf b) {
  const cf t = a * make_float2(b.x, b.x);
  const cf s = make_float2(a.y, a.x) * make_float2(-b.y, b.y);
  return t + s;
}
// multiply by -i
__device__ __forceinline__ cf cmul_mi(cf a) { return make_float2(a.y, -a.x); }

#define VPS_SQRT1_2 0.70710678118654752440f
#define VPS_COS_PI_8 0.92387953251128675613f
#define VPS_SIN_PI_8 0.38268343236508977173f

// ---- small DFTs on registers, forward sign exp(-2 pi i nk/R), natural order ----
template <int R>
struct Dft;

template <>
struct Dft<1> {
  static __device__ __forceinline__ void run(cf*) {}
};
template <>
struct Dft<2> {
  static __device__ __forceinline__ void run(cf* v) {
    cf a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
  }
};
template <>
struct Dft<4> {
  static __device__ __forceinline__ void run(cf* v) {
    cf t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
    cf t2 = cadd(v[1], v[3]), t3 = cmul_mi(csub(v[1], v[3]));
    v[0] = cadd(t0, t2);
    v[1] = cadd(t1, t3);
    v[2] = csub(t0, t2);
    v[3] = csub(t1, t3);
  }
};
template <>
struct Dft<8> {
  static __device__ __forceinline__ void run(cf* v) {
    cf e[4] = {v[0], v[2], v[4], v[6]};
    cf o[4] = {v[1], v[3], v[5], v[7]};
    Dft<4>::run(e);
    Dft<4>::run(o);
    // o[k] *= w8^k
    cf o1 = make_float2((o[1].x + o[1].y) * VPS_SQRT1_2, (o[1].y - o[1].x) * VPS_SQRT1_2);
    cf o2 = cmul_mi(o[2]);
    cf o3 = make_float2((o[3].y - o[3].x) * VPS_SQRT1_2, -(o[3].x + o[3].y) * VPS_SQRT1_2);
    v[0] = cadd(e[0], o[0]);
    v[4] = csub(e[0], o[0]);
    v[1] = cadd(e[1], o1);
    v[5] = csub(e[1], o1);
    v[2] = cadd(e[2], o2);
    v[6] = csub(e[2], o2);
    v[3] = cadd(e[3], o3);
    v[7] = csub(e[3], o3);
  }
};
template <>
struct Dft<16> {
  static __device__ __forceinline__ void run(cf* v) {
    // n = 4*n1 + n2, k = k1 + 4*k2
    cf y[4][4];
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) {
      cf t[4] = {v[n2], v[4 + n2], v[8 + n2], v[12 + n2]};
      Dft<4>::run(t);
#pragma unroll
      for (int k1 = 0; k1 < 4; ++k1) y[n2][k1] = t[k1];
    }
    // twiddles w16^(n2*k1)
    const cf w1 = make_float2(VPS_COS_PI_8, -VPS_SIN_PI_8);
    const cf w2 = make_float2(VPS_SQRT1_2, -VPS_SQRT1_2);
    const cf w3 = make_float2(VPS_SIN_PI_8, -VPS_COS_PI_8);
    const cf w6 = make_float2(-VPS_SQRT1_2, -VPS_SQRT1_2);
    const cf w9 = make_float2(-VPS_COS_PI_8, VPS_SIN_PI_8);
    y[1][1] = cmul(y[1][1], w1);
    y[1][2] = cmul(y[1][2], w2);
    y[1][3] = cmul(y[1][3], w3);
    y[2][1] = cmul(y[2][1], w2);
    y[2][2] = cmul_mi(y[2][2]);
    y[2][3] = cmul(y[2][3], w6);
    y[3][1] = cmul(y[3][1], w3);
    y[3][2] = cmul(y[3][2], w6);
    y[3][3] = cmul(y[3][3], w9);
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) {
      cf t[4] = {y[0][k1], y[1][k1], y[2][k1], y[3][k1]};
      Dft<4>::run(t);
#pragma unroll
      for (int k2 = 0; k2 < 4; ++k2) v[k1 + 4 * k2] = t[k2];
    }
  }
};

// radix 3, 6 = 2 x 3, 12 = 2 x 6 (forward): lengths 3 * 2^a (N = 96, 192, 384, 768)
#define VPS_SQRT3_2 0.86602540378443864676f
template <>
struct Dft<3> {
  static __device__ __forceinline__ void run(cf* v) {
    const cf t = cadd(v[1], v[2]), d = csub(v[1], v[2]);
    const cf m = make_float2(v[0].x - 0.5f * t.x, v[0].y - 0.5f * t.y);
    const cf u = make_float2(VPS_SQRT3_2 * d.y, -VPS_SQRT3_2 * d.x);   // -i (sqrt(3)/2) d
    v[0] = cadd(v[0], t);
    v[1] = cadd(m, u);
    v[2] = csub(m, u);
  }
};
template <>
struct Dft<6> {
  static __device__ __forceinline__ void run(cf* v) {
    cf e[3] = {v[0], v[2], v[4]};
    cf o[3] = {v[1], v[3], v[5]};
    Dft<3>::run(e);
    Dft<3>::run(o);
    o[1] = cmul(o[1], make_float2(0.5f, -VPS_SQRT3_2));    // w6
    o[2] = cmul(o[2], make_float2(-0.5f, -VPS_SQRT3_2));   // w6^2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = cadd(e[k], o[k]);
      v[k + 3] = csub(e[k], o[k]);
    }
  }
};
template <>
struct Dft<12> {
  static __device__ __forceinline__ void run(cf* v) {
    cf e[6] = {v[0], v[2], v[4], v[6], v[8], v[10]};
    cf o[6] = {v[1], v[3], v[5], v[7], v[9], v[11]};
    Dft<6>::run(e);
    Dft<6>::run(o);
    // o[k] *= w12^k, w12 = exp(-i pi/6)
    o[1] = cmul(o[1], make_float2(VPS_SQRT3_2, -0.5f));
    o[2] = cmul(o[2], make_float2(0.5f, -VPS_SQRT3_2));
    o[3] = cmul_mi(o[3]);
    o[4] = cmul(o[4], make_float2(-0.5f, -VPS_SQRT3_2));
    o[5] = cmul(o[5], make_float2(-VPS_SQRT3_2, -0.5f));
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      v[k] = cadd(e[k], o[k]);
      v[k + 6] = csub(e[k], o[k]);
    }
  }
};

// radix 5 (forward, w = exp(-2 pi i/5)) and radix 10 = 2 x 5: lengths 2^a 5^b (N = 250, 500, 1000)
#define VPS_C1_5 0.30901699437494742410f    /* cos(2 pi/5) */
#define VPS_C2_5 (-0.80901699437494742410f) /* cos(4 pi/5) */
#define VPS_S1_5 0.95105651629515357212f    /* sin(2 pi/5) */
#define VPS_S2_5 0.58778525229247312917f    /* sin(4 pi/5) */
template <>
struct Dft<5> {
  static __device__ __forceinline__ void run(cf* v) {
    const cf a = cadd(v[1], v[4]), b = csub(v[1], v[4]);
    const cf c = cadd(v[2], v[3]), d = csub(v[2], v[3]);
    const cf t1 = make_float2(v[0].x + VPS_C1_5 * a.x + VPS_C2_5 * c.x, v[0].y + VPS_C1_5 * a.y + VPS_C2_5 * c.y);
    const cf t2 = make_float2(v[0].x + VPS_C2_5 * a.x + VPS_C1_5 * c.x, v[0].y + VPS_C2_5 * a.y + VPS_C1_5 * c.y);
    // u = -i * (s b +- s' d)
    const cf q1 = make_float2(VPS_S1_5 * b.x + VPS_S2_5 * d.x, VPS_S1_5 * b.y + VPS_S2_5 * d.y);
    const cf q2 = make_float2(VPS_S2_5 * b.x - VPS_S1_5 * d.x, VPS_S2_5 * b.y - VPS_S1_5 * d.y);
    const cf u1 = cmul_mi(q1), u2 = cmul_mi(q2);
    v[0] = make_float2(v[0].x + a.x + c.x, v[0].y + a.y + c.y);
    v[1] = cadd(t1, u1);
    v[4] = csub(t1, u1);
    v[2] = cadd(t2, u2);
    v[3] = csub(t2, u2);
  }
};
template <>
struct Dft<10> {
  static __device__ __forceinline__ void run(cf* v) {
    cf e[5] = {v[0], v[2], v[4], v[6], v[8]};
    cf o[5] = {v[1], v[3], v[5], v[7], v[9]};
    Dft<5>::run(e);
    Dft<5>::run(o);
    // o[k] *= w10^k, w10 = exp(-2 pi i/10): cos(pi/5) = -c2_5, sin(pi/5) = s2_5, cos(2pi/5) = c1_5, sin(2pi/5) = s1_5
    const cf w1 = make_float2(-VPS_C2_5, -VPS_S2_5), w2 = make_float2(VPS_C1_5, -VPS_S1_5);
    const cf w3 = make_float2(-VPS_C1_5, -VPS_S1_5), w4 = make_float2(VPS_C2_5, -VPS_S2_5);
    o[1] = cmul(o[1], w1);
    o[2] = cmul(o[2], w2);
    o[3] = cmul(o[3], w3);
    o[4] = cmul(o[4], w4);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      v[k] = cadd(e[k], o[k]);
      v[k + 5] = csub(e[k], o[k]);
    }
  }
};

// radix 24 = 8 x 3 and radix 20 = 5 x 4 (generated: twiddle constants are cos / sin of -2 pi m / N in double, printed to 17 digits)
template <>
struct Dft<24> {
  static __device__ __forceinline__ void run(cf* v) {
    // n = 3 n1 + n2, k = k1 + 8 k2: 3 x Dft<8>, twiddles w24^(n2 k1), 8 x Dft<3>
    cf y[3][8];
#pragma unroll
    for (int n2 = 0; n2 < 3; ++n2) {
      cf t[8];
#pragma unroll
      for (int n1 = 0; n1 < 8; ++n1) t[n1] = v[3 * n1 + n2];
      Dft<8>::run(t);
#pragma unroll
      for (int k1 = 0; k1 < 8; ++k1) y[n2][k1] = t[k1];
    }
    y[1][1] = cmul(y[1][1], make_float2(0.96592582628906831f, -0.25881904510252074f));
    y[1][2] = cmul(y[1][2], make_float2(0.86602540378443871f, -0.49999999999999994f));
    y[1][3] = cmul(y[1][3], make_float2(0.70710678118654757f, -0.70710678118654746f));
    y[1][4] = cmul(y[1][4], make_float2(0.50000000000000011f, -0.8660254037844386f));
    y[1][5] = cmul(y[1][5], make_float2(0.25881904510252074f, -0.96592582628906831f));
    y[1][6] = cmul_mi(y[1][6]);
    y[1][7] = cmul(y[1][7], make_float2(-0.25881904510252063f, -0.96592582628906831f));
    y[2][1] = cmul(y[2][1], make_float2(0.86602540378443871f, -0.49999999999999994f));
    y[2][2] = cmul(y[2][2], make_float2(0.50000000000000011f, -0.8660254037844386f));
    y[2][3] = cmul_mi(y[2][3]);
    y[2][4] = cmul(y[2][4], make_float2(-0.49999999999999978f, -0.86602540378443871f));
    y[2][5] = cmul(y[2][5], make_float2(-0.86602540378443871f, -0.49999999999999994f));
    y[2][6] = make_float2(-y[2][6].x, -y[2][6].y);
    y[2][7] = cmul(y[2][7], make_float2(-0.86602540378443882f, 0.49999999999999972f));
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) {
      cf t[3];
#pragma unroll
      for (int n2 = 0; n2 < 3; ++n2) t[n2] = y[n2][k1];
      Dft<3>::run(t);
#pragma unroll
      for (int k2 = 0; k2 < 3; ++k2) v[k1 + 8 * k2] = t[k2];
    }
  }
};
template <>
struct Dft<20> {
  static __device__ __forceinline__ void run(cf* v) {
    // n = 4 n1 + n2, k = k1 + 5 k2: 4 x Dft<5>, twiddles w20^(n2 k1), 5 x Dft<4>
    cf y[4][5];
#pragma unroll
    for (int n2 = 0; n2 < 4; ++n2) {
      cf t[5];
#pragma unroll
      for (int n1 = 0; n1 < 5; ++n1) t[n1] = v[4 * n1 + n2];
      Dft<5>::run(t);
#pragma unroll
      for (int k1 = 0; k1 < 5; ++k1) y[n2][k1] = t[k1];
    }
    y[1][1] = cmul(y[1][1], make_float2(0.95105651629515353f, -0.3090169943749474f));
    y[1][2] = cmul(y[1][2], make_float2(0.80901699437494745f, -0.58778525229247314f));
    y[1][3] = cmul(y[1][3], make_float2(0.58778525229247314f, -0.80901699437494745f));
    y[1][4] = cmul(y[1][4], make_float2(0.30901699437494745f, -0.95105651629515353f));
    y[2][1] = cmul(y[2][1], make_float2(0.80901699437494745f, -0.58778525229247314f));
    y[2][2] = cmul(y[2][2], make_float2(0.30901699437494745f, -0.95105651629515353f));
    y[2][3] = cmul(y[2][3], make_float2(-0.30901699437494734f, -0.95105651629515364f));
    y[2][4] = cmul(y[2][4], make_float2(-0.80901699437494734f, -0.58778525229247325f));
    y[3][1] = cmul(y[3][1], make_float2(0.58778525229247314f, -0.80901699437494745f));
    y[3][2] = cmul(y[3][2], make_float2(-0.30901699437494734f, -0.95105651629515364f));
    y[3][3] = cmul(y[3][3], make_float2(-0.95105651629515353f, -0.30901699437494751f));
    y[3][4] = cmul(y[3][4], make_float2(-0.80901699437494756f, 0.58778525229247303f));
#pragma unroll
    for (int k1 = 0; k1 < 5; ++k1) {
      cf t[4];
#pragma unroll
      for (int n2 = 0; n2 < 4; ++n2) t[n2] = y[n2][k1];
      Dft<4>::run(t);
#pragma unroll
      for (int k2 = 0; k2 < 4; ++k2) v[k1 + 5 * k2] = t[k2];
    }
  }
};

}  // namespace
