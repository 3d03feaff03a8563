// The gconv-LSTM cell (lib/gconv_lstm.py:188-218): its gate nonlinearities
// (z = tan, i = f = sigmoid, o = tanh in the reference; tanh / sigmoid for the
// standard gates), its update c' = f c + i z, h' = o tanh(c'), and that
// update's gradient.  This is the ONE definition: the pointwise cell kernels
// (lstm.hip), the one-launch h-step (lstm_fused.hip) and the Fourier
// synthesis' gate epilogue (fourier_lstm.hip) call lstm_cell_fwd /
// lstm_cell_bwd, which is why they agree bitwise on the same pre-activations.
// lstm_seq.hip's two kernels alone write them out by hand (the calls cost them
// time and registers; see there), held to this file by
// test_every_cell_site_agrees_bitwise.
// (dense_lstm.hip is another cell, TensorFlow's BasicLSTMCell, and takes only
// the scalar gate functions.)
//
// The device library's tanf / tanhf / expf + IEEE division cost ~350 VALU
// instructions per unit in the sequence kernel's gate epilogue (mostly range
// reduction for arguments no gate ever sees).  These forms keep a few ulp of
// accuracy (the parity bar is 1e-5 normwise against float64) in ~60:
//   tan:     Cody-Waite reduction by pi/2 (three-part constant, fused
//            multiply-adds: exact for |x| < 8192) + the Cephes minimax
//            polynomial on [-pi/4, pi/4] (relative error <= 4e-7), -1/tan
//            in odd quadrants; |x| >= 8192 or non-finite: the library tanf
//   sigmoid: 1 / (1 + exp(-a)) with the hardware 2^x and reciprocal (1 ulp each)
//   tanh:    |x| < 0.625: the Cephes odd polynomial (<= 2 ulp); else
//            1 - 2 / (exp(2|x|) + 1) with the sign restored (exp overflow
//            gives exactly +-1)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cheb_mi355.h"  // CG_LSTM_GATES_*

namespace cg {

__device__ __forceinline__ float gate_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// e^x as the hardware 2^x of x log2(e): the product's rounding (|x| 2^-24
// relative in the exponent) is <= 1.2e-6 relative for the |x| <= 20 that
// leave a sigmoid or tanh short of saturation; out of range it saturates to
// 0 / +inf like expf
__device__ __forceinline__ float gate_exp(float x) {
#pragma clang fp contract(off)
  return __builtin_amdgcn_exp2f(x * 1.44269504088896341f);
}

__device__ __forceinline__ float gate_sigmoid(float a) {
#pragma clang fp contract(off)
  return gate_rcp(1.f + gate_exp(-a));
}

__device__ __forceinline__ float gate_tanh(float x) {
#pragma clang fp contract(off)
  const float ax = fabsf(x);
  const float z = x * x;
  float p = -5.70498872745e-3f;
  p = __builtin_fmaf(p, z, 2.06390887954e-2f);
  p = __builtin_fmaf(p, z, -5.37397155531e-2f);
  p = __builtin_fmaf(p, z, 1.33314422036e-1f);
  p = __builtin_fmaf(p, z, -3.33332819422e-1f);
  const float small = __builtin_fmaf(p * z, x, x);
  const float e = gate_exp(2.f * ax);
  const float big = 1.f - 2.f * gate_rcp(e + 1.f);
  const float r = ax < 0.625f ? small : __builtin_copysignf(big, x);
  return x != x ? x : r;
}

__device__ __forceinline__ float gate_tan(float x) {
#pragma clang fp contract(off)
  if (!(fabsf(x) < 8192.f)) return tanf(x);  // huge or non-finite: the library routine
  const float k = __builtin_rintf(x * 0.636619772367581343f);  // x * 2/pi
  float r = __builtin_fmaf(-k, 1.57079637050628662109375f, x);
  r = __builtin_fmaf(-k, -4.37113900018624283e-8f, r);
  r = __builtin_fmaf(-k, -1.71512451438203e-15f, r);
  const float z = r * r;
  float p = 9.38540185543e-3f;
  p = __builtin_fmaf(p, z, 3.11992232697e-3f);
  p = __builtin_fmaf(p, z, 2.44301354525e-2f);
  p = __builtin_fmaf(p, z, 5.34112807005e-2f);
  p = __builtin_fmaf(p, z, 1.33387994085e-1f);
  p = __builtin_fmaf(p, z, 3.33331568548e-1f);
  const float t = __builtin_fmaf(p * z, r, r);
  const bool odd = (int(k) & 1) != 0;
  return odd ? -gate_rcp(t) : t;
}

// One cell update from the four pre-activations (gx + gh + bias, the caller's)
// and c_{t-1} = c_prev(): a callable, so that a caller's load of c stays
// behind the gates, where each kernel had it (moving it ahead of them changes
// the kernels' register allocation).  ref: the reference gate set
// (CG_LSTM_GATES_REFERENCE), a template parameter or a runtime field of the
// caller alike.
struct LstmCell {
  float z, i, f, o, c, h;  // gate activations (the act record), c', h'
};

template <typename CPrev>
__device__ __forceinline__ LstmCell lstm_cell_fwd(float az, float ai, float af, float ao,
                                                  CPrev&& c_prev, bool ref) {
#pragma clang fp contract(off)
  LstmCell s;
  s.z = ref ? gate_tan(az) : gate_tanh(az);
  s.i = gate_sigmoid(ai);
  s.f = gate_sigmoid(af);
  s.o = ref ? gate_tanh(ao) : gate_sigmoid(ao);
  const float cp = c_prev();
  s.c = s.f * cp + s.i * s.z;  // ft * c + it * zt (:215)
  s.h = s.o * gate_tanh(s.c);  // ot * tanh(new_c) (:218)
  return s;
}

// Its reverse (TF autodiff of the same expressions) from the act record: dh is
// the summed gradient w.r.t. h' (dh + dh_rec), dc points at the gradient
// w.r.t. c' or is NULL, and then nothing is added (x + 0 is not x for -0).
// (A pointer, at memory or at a value in registers: "absent" needs no second
// argument, and k_lstm_bwd's load of dc stays behind its test, where it was.)
// d[0..3] are the pre-activation gradients of z, i, f, o; dc_prev = dL/dc.
struct LstmCellGrad {
  float d[4], dc_prev;
};

__device__ __forceinline__ LstmCellGrad lstm_cell_bwd(float z, float i, float f, float o,
                                                      float c_prev, float c_out, float dh,
                                                      const float* dc, bool ref) {
#pragma clang fp contract(off)
  const float tc = gate_tanh(c_out);
  float dcn = dh * o * (1.f - tc * tc);
  if (dc) dcn = dcn + *dc;
  const float d_o = dh * tc;
  const float d_i = dcn * z, d_z = dcn * i, d_f = dcn * c_prev;
  LstmCellGrad g;
  g.d[0] = ref ? d_z * (1.f + z * z) : d_z * (1.f - z * z);  // tan' = 1 + tan^2
  g.d[1] = d_i * (i * (1.f - i));
  g.d[2] = d_f * (f * (1.f - f));
  g.d[3] = ref ? d_o * (1.f - o * o) : d_o * (o * (1.f - o));
  g.dc_prev = dcn * f;
  return g;
}

}  // namespace cg
