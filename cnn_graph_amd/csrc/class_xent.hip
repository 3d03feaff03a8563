// The class loss of the pooled cgcnn classifier (lib/graph_model.py:249-258 as the
// fork left it in comments, lib/models.py:24-55): softmax cross-entropy of logits
// [N][C] against int32 labels [N], the L2 term of the regularised variables, the
// gradient, the prediction and the loss moving average, in two launches:
//   ce[n]      = log sum_c exp(x[n][c] - max_n) - (x[n][label_n] - max_n)
//   loss       = (1/N) sum_n ce[n] + reg_scale * 1/2 sum_{i in [rb, rb + rn)} w[i]^2
//   dlogits    = (exp(x - max - lse) - [c == label]) / N
//   pred[n]    = the FIRST maximum of row n;  correct = #{n : pred[n] == label_n}
//
// k_class_xent: 256 threads = four waves.  The first ceil(N / 4) workgroups take
// one row per wave, lane-strided over C, so any C >= 1 works (a row of C <= 64 is
// one load per lane); max and first-argmax, then the sum, by xor shuffles.  The
// workgroups after them each take one chunk of the regularised range and leave
// its sum of squares in the workspace (k_mse_part's fixed-order tree).
// k_class_xent_final: one workgroup adds the rows' ce and the chunks in a fixed
// order (lane-strided, then the LDS tree), counts the correct rows, finds the
// first row whose label is outside [0, C), and updates the moving average
// (k_mse_final's zero-debias convention).  No floating-point atomics: two
// calls agree bitwise.
//
// A label outside [0, C) is never used as an index: the row reads x[n][clamped],
// its ce and dlogits are NaN (TF's GPU kernel does the same), and status[0]
// receives the first such row + 1 (0: none).
//
// cg_class_xent_sum (the dense LSTM baseline's loss, lib/gconvRNN.py:328-332) is
// the same two launches with the caller's loss_scale in the place of 1/N (the
// kernels' inv_n), no regularised range and no moving average.
#include "cg_internal.h"

#include <cmath>

namespace cg {
namespace {

struct ClassXentArgs {
  const float* x;
  const int32_t* labels;
  int N, C;
  const float* reg;  // the first regularised parameter (params + reg_begin)
  int64_t reg_n, reg_chunk;
  int row_blocks;
  float inv_n;
  float* dx;      // NULL: evaluation
  int32_t* pred;  // NULL: not wanted
  float* ce;      // workspace [N]
  int32_t* flag;  // workspace [N]: bit 0 correct, bit 1 label out of range
  float* slab;    // workspace [reg chunks]
};

__global__ __launch_bounds__(256) void k_class_xent(ClassXentArgs a) {
#pragma clang fp contract(off)
  __shared__ float part[256];
  const int tid = int(threadIdx.x), lane = tid & 63, w = tid >> 6;
  if (int(blockIdx.x) >= a.row_blocks) {  // workgroup-uniform: a chunk of 1/2 sum w^2
    const int64_t z = int64_t(blockIdx.x) - a.row_blocks;
    const int64_t c0 = z * a.reg_chunk;
    const int64_t c1 = c0 + a.reg_chunk < a.reg_n ? c0 + a.reg_chunk : a.reg_n;
    float s = 0.f;
    for (int64_t i = c0 + tid; i < c1; i += 256) s = s + a.reg[i] * a.reg[i];
    part[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) part[tid] = part[tid] + part[tid + h];
      __syncthreads();
    }
    if (tid == 0) a.slab[z] = 0.5f * part[0];
    return;
  }
  const int64_t n = int64_t(blockIdx.x) * 4 + w;
  if (n >= a.N) return;  // wave-uniform; no barrier on this branch
  const int C = a.C;
  const float* row = a.x + n * C;
  const int lab = a.labels[n];
  const bool lab_ok = lab >= 0 && lab < C;
  const int li = lab < 0 ? 0 : (lab >= C ? C - 1 : lab);

  // max and its first index: a lane's columns ascend, so strict > keeps its
  // first; across lanes the greater value, then the smaller index
  float mx = -INFINITY;
  int mi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float v = row[c];
    if (v > mx || mi == 0x7fffffff) mx = v, mi = c;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o);
    const int oi = __shfl_xor(mi, o);
    if (oi != 0x7fffffff && (mi == 0x7fffffff || ov > mx || (ov == mx && oi < mi))) mx = ov, mi = oi;
  }
  float sum = 0.f;
  for (int c = lane; c < C; c += 64) sum = sum + expf(row[c] - mx);
  for (int o = 32; o > 0; o >>= 1) sum = sum + __shfl_xor(sum, o);
  const float lsum = logf(sum);  // log-sum-exp = mx + lsum
  const float nan = __builtin_nanf("");
  if (lane == 0) {
    a.ce[n] = lab_ok ? lsum + (mx - row[li]) : nan;
    a.flag[n] = (lab_ok && mi == lab ? 1 : 0) | (lab_ok ? 0 : 2);
    if (a.pred) a.pred[n] = mi;
  }
  if (a.dx) {
    float* drow = a.dx + n * C;
    for (int c = lane; c < C; c += 64) {
      const float g = (expf((row[c] - mx) - lsum) - (c == lab ? 1.f : 0.f)) * a.inv_n;
      drow[c] = lab_ok ? g : nan;
    }
  }
}

__global__ __launch_bounds__(256) void k_class_xent_final(const float* __restrict__ ce,
                                                          const int32_t* __restrict__ flag, int N,
                                                          const float* __restrict__ slab, int nslab,
                                                          float inv_n, float reg_scale,
                                                          float* __restrict__ loss,
                                                          float* __restrict__ ema, float decay,
                                                          int32_t* __restrict__ correct,
                                                          int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ float p_ce[256], p_rg[256];
  __shared__ int p_ok[256], p_bad[256];
  const int tid = int(threadIdx.x);
  float s = 0.f, r = 0.f;
  int ok = 0, bad = 0x7fffffff;
  for (int n = tid; n < N; n += 256) {
    s = s + ce[n];
    const int f = flag[n];
    ok += f & 1;
    if ((f & 2) && n < bad) bad = n;
  }
  for (int z = tid; z < nslab; z += 256) r = r + slab[z];
  p_ce[tid] = s, p_rg[tid] = r, p_ok[tid] = ok, p_bad[tid] = bad;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      p_ce[tid] = p_ce[tid] + p_ce[tid + h];
      p_rg[tid] = p_rg[tid] + p_rg[tid + h];
      p_ok[tid] += p_ok[tid + h];
      if (p_bad[tid + h] < p_bad[tid]) p_bad[tid] = p_bad[tid + h];
    }
    __syncthreads();
  }
  if (tid) return;
  float l = p_ce[0] * inv_n;
  if (nslab > 0) l = l + reg_scale * p_rg[0];
  *loss = l;
  if (correct) *correct = p_ok[0];
  if (status) *status = p_bad[0] == 0x7fffffff ? 0 : p_bad[0] + 1;
  if (ema) {  // k_mse_final's ExponentialMovingAverage(decay), zero-debiased
    const float d1 = 1.f - decay;
    const float biased = ema[0] - (ema[0] - l) * d1;
    const float step = ema[2] + 1.f;
    const float bias_factor = 1.f - powf(1.f - d1, step);
    ema[0] = biased;
    ema[1] = ema[1] - (ema[1] - biased / bias_factor);
    ema[2] = step;
  }
}

}  // namespace

size_t class_xent_ws_bytes(int N, int64_t reg_n) {
  const size_t chunks = reg_n > 0 ? size_t(mse_chunks(reg_n)) : 0;
  return align16((2 * size_t(N) + chunks) * sizeof(float));
}

hipError_t launch_class_xent(const float* logits, const int32_t* labels, int N, int C,
                             const float* reg, int64_t reg_n, float reg_scale, float row_scale,
                             float* loss, float* dlogits, float* ema, float decay, int32_t* pred,
                             int32_t* correct, int32_t* status, float* ws, hipStream_t s) {
  const int chunks = reg_n > 0 ? mse_chunks(reg_n) : 0;
  ClassXentArgs a;
  a.x = logits, a.labels = labels, a.N = N, a.C = C;
  a.reg = reg, a.reg_n = reg_n, a.reg_chunk = chunks ? (reg_n + chunks - 1) / chunks : 0;
  a.row_blocks = (N + 3) / 4;
  a.inv_n = row_scale;
  a.dx = dlogits, a.pred = pred;
  a.ce = ws, a.flag = reinterpret_cast<int32_t*>(ws + N), a.slab = ws + 2 * size_t(N);
  hipLaunchKernelGGL(k_class_xent, dim3(unsigned(a.row_blocks + chunks)), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_class_xent_final, dim3(1), dim3(256), 0, s, a.ce, a.flag, N, a.slab, chunks,
                     a.inv_n, reg_scale, loss, ema, decay, correct, status);
  return hipGetLastError();
}

}  // namespace cg
