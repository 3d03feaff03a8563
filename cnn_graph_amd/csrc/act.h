// The activation of the residual / bias epilogues, y = act(v) with act one of
// the public header's CG_ACT_*, and its gradient from the OUTPUT y.  The ONE
// definition: k_act_fwd / k_act_bwd of epilogue.hip and the y stores of the
// resident and row-GEMM kernels call act_fwd / act_grad; the fast forward
// (tanh chosen at compile time, so its other instantiations hold no tanh
// code), k_grp_yred, k_bias_act_* and the Fourier residual block's EX modes
// branch on act themselves around the leaves act_relu / act_tanh and their
// gradients.  tanh here is cg::gate_tanh; k_bias_act_fwd alone keeps the
// library tanhf.
#pragma once
#include "../../include/cheb_mi355.h"  // CG_ACT_*
#include "lstm_gates.h"

namespace cg {

__device__ __forceinline__ float act_relu(float v) { return v > 0.f ? v : 0.f; }
__device__ __forceinline__ float act_tanh(float v) { return gate_tanh(v); }
__device__ __forceinline__ float4 act_relu(float4 v) {
  return make_float4(act_relu(v.x), act_relu(v.y), act_relu(v.z), act_relu(v.w));
}
__device__ __forceinline__ float4 act_tanh(float4 v) {
  return make_float4(act_tanh(v.x), act_tanh(v.y), act_tanh(v.z), act_tanh(v.w));
}

// (x by reference for one purpose only: assembly identical to the commit before
// this header; by value (noundef) the compiler folds the two tests differently.
// Once that identity no longer matters, pass x by value.)
__device__ __forceinline__ float act_fwd(const float& x, int act) {
  float v = x;
  if (act == CG_ACT_TANH) v = act_tanh(v);
  else if (act != CG_ACT_NONE) v = act_relu(v);
  return v;
}

// dz = g * act'(y) from the OUTPUT y (TF ReluGrad / TanhGrad)
__device__ __forceinline__ float act_relu_grad(float g, float y) { return y > 0.f ? g : 0.f; }
__device__ __forceinline__ float act_tanh_grad(float g, float y) {
#pragma clang fp contract(off)
  return g * (1.f - y * y);
}

// act CG_ACT_RELU or CG_ACT_TANH; CG_ACT_NONE has no y to read (dz = g),
// which is its caller's branch
__device__ __forceinline__ float act_grad(float g, float y, int act) {
  return act == CG_ACT_TANH ? act_tanh_grad(g, y) : act_relu_grad(g, y);
}

__device__ __forceinline__ float4 act_grad(float4 g, float4 y, int act) {
  return make_float4(act_grad(g.x, y.x, act), act_grad(g.y, y.y, act), act_grad(g.z, y.z, act),
                     act_grad(g.w, y.w, act));
}

}  // namespace cg
