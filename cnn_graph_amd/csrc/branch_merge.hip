// The two seams of the closeness / period / trend gconv-LSTM networks
// (lib/gconv_lstm.py:431-607), kernels and C entries (include/cheb_mi355.h):
//   k_branch_merge_fwd   X = ((y_0 w_0) + y_1 w_1) + ... with w_b [M][F] broadcast
//                        over the batch (:494-497, :528-531): every product and
//                        every sum rounded to fp32 in that order, no contraction
//   k_branch_merge_bwd   ONE launch for every branch, one pass over dout and the
//                        y_b: dy_b = dout w_b (the Mul gradient on x's side) and
//                        dw_b = sum_n dout y_b (its broadcast reduction), summed
//                        in a fixed order inside the workgroup, no atomics
//   k_concat_drop        tf.concat(output_arr, axis=2) of the branches' h_T (:451,
//                        :590) with each branch read through its own
//                        DropoutWrapper mask (drop_one of cg_internal.h, the
//                        arithmetic of k_dropout), and the split of the gradient
//                        back through the masks
// Each kernel has a dwordx4 form for rows that are a multiple of four floats
// on 16-byte aligned pointers and a scalar form; the host chooses per call.
#include "../../include/cheb_mi355.h"

#include <hip/hip_runtime.h>

#include "abi_checks.h"
#include "cg_internal.h"

namespace cg {
namespace {

constexpr int MAXB = 4;  // branches per call (the reference has two and three)

// the per-branch pointers and sizes, passed to the kernels by value
struct MergeArgs {
  const float* y[MAXB];
  const float* w[MAXB];
  float* dy[MAXB];
  float* dw[MAXB];
};
struct ConcatArgs {
  float* h[MAXB];  // forward: read; backward: written
  unsigned long long seed[MAXB];
  int H[MAXB];
  int off[MAXB + 1];  // column offset of branch b in the concatenation; off[B] = sum H
};

inline int grid1d(int64_t n, int per_block) {
  int64_t g = (n + per_block - 1) / per_block;
  return int(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// float i of a float or float4 (the kernels are written once for both widths)
template <typename V>
__device__ __forceinline__ float& lane(V& v, int i) {
  return reinterpret_cast<float*>(&v)[i];
}
template <typename V>
__device__ __forceinline__ float lval(const V& v, int i) {
  return reinterpret_cast<const float*>(&v)[i];
}

// V = float (n elements, w index i mod MF) or float4 (n and MF counted in
// float4: MF % 4 == 0, so a float4 of w never wraps)
template <typename V>
__global__ __launch_bounds__(256) void k_branch_merge_fwd(MergeArgs a, int B, int64_t n, int64_t MF,
                                                          V* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int L = sizeof(V) / 4;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    const int64_t j = i % MF;
    V acc;
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
      if (b < B) {
        const V yv = reinterpret_cast<const V*>(a.y[b])[i];
        const V wv = reinterpret_cast<const V*>(a.w[b])[j];
#pragma unroll
        for (int l = 0; l < L; ++l) {
          const float p = lval(yv, l) * lval(wv, l);
          lane(acc, l) = b == 0 ? p : lane(acc, l) + p;
        }
      }
    }
    out[i] = acc;
  }
}

// Workgroup = BM_COLS column lanes x BM_LANES batch lanes.  Batch lane r walks
// the samples n = r, r + BM_LANES, ... in ascending order (its dy stores on the
// way) and keeps one partial per branch; the partials meet in LDS and batch
// lane 0 adds them in the order r = 0 .. BM_LANES-1: a fixed order, so two
// calls agree bitwise.
constexpr int BM_COLS = 32;
constexpr int BM_LANES = 8;

template <typename V>
__global__ __launch_bounds__(BM_COLS* BM_LANES) void k_branch_merge_bwd(
    MergeArgs a, int B, int N, int64_t MF, const V* __restrict__ dout, int accumulate) {
#pragma clang fp contract(off)
  constexpr int L = sizeof(V) / 4;
  __shared__ V part[MAXB][BM_LANES][BM_COLS];
  const int c = threadIdx.x % BM_COLS, r = threadIdx.x / BM_COLS;
  const int64_t j = int64_t(blockIdx.x) * BM_COLS + c;  // the column (in units of V)
  const bool live = j < MF;
  V s[MAXB];
#pragma unroll
  for (int b = 0; b < MAXB; ++b)
#pragma unroll
    for (int l = 0; l < L; ++l) lane(s[b], l) = 0.f;
  if (live) {
    V wv[MAXB];
#pragma unroll
    for (int b = 0; b < MAXB; ++b)
      if (b < B && a.dy[b]) wv[b] = reinterpret_cast<const V*>(a.w[b])[j];
    for (int n = r; n < N; n += BM_LANES) {
      const int64_t i = int64_t(n) * MF + j;
      const V d = dout[i];
#pragma unroll
      for (int b = 0; b < MAXB; ++b) {
        if (b >= B) continue;
        if (a.dy[b]) {
          V o;
#pragma unroll
          for (int l = 0; l < L; ++l) lane(o, l) = lval(d, l) * lval(wv[b], l);
          reinterpret_cast<V*>(a.dy[b])[i] = o;
        }
        if (a.dw[b]) {
          const V yv = reinterpret_cast<const V*>(a.y[b])[i];
#pragma unroll
          for (int l = 0; l < L; ++l) lane(s[b], l) = lane(s[b], l) + lval(d, l) * lval(yv, l);
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < MAXB; ++b)
    if (b < B && a.dw[b]) part[b][r][c] = s[b];
  __syncthreads();
  if (r != 0 || !live) return;
#pragma unroll
  for (int b = 0; b < MAXB; ++b) {
    if (b >= B || !a.dw[b]) continue;
    V t = part[b][0][c];
    for (int q = 1; q < BM_LANES; ++q) {
      const V p = part[b][q][c];
#pragma unroll
      for (int l = 0; l < L; ++l) lane(t, l) = lane(t, l) + lval(p, l);
    }
    V* dst = reinterpret_cast<V*>(a.dw[b]) + j;
    if (accumulate) {
      const V old = *dst;
#pragma unroll
      for (int l = 0; l < L; ++l) lane(t, l) = lval(old, l) + lane(t, l);
    }
    *dst = t;
  }
}

// One thread per element (or float4) of the wide tensor [rows][S].  BWD 0:
// wide = drop(h_b) (the concat); BWD 1: h_b = drop'(wide) (the split).  The
// mask index is the flat index in branch b's own [rows][H_b]; keep == 1 moves
// the values untouched (cg_dropout_* is not called then either).
template <typename V, int BWD>
__global__ __launch_bounds__(256) void k_concat_drop(ConcatArgs a, int B, int64_t n, float keep,
                                                     float* __restrict__ wide) {
  constexpr int L = sizeof(V) / 4;
  const int S = a.off[B] / L;  // the wide row in units of V
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    const int64_t row = i / S;
    const int col = int(i - row * S) * L;
    int b = 0;
#pragma unroll
    for (int q = 1; q < MAXB; ++q)
      if (q < B && col >= a.off[q]) b = q;
    const int64_t e = row * a.H[b] + (col - a.off[b]);  // flat index inside branch b
    V* hp = reinterpret_cast<V*>(a.h[b] + e);
    V* wp = reinterpret_cast<V*>(wide) + i;
    V v = BWD ? *wp : *hp;
    if (keep < 1.f) {
#pragma unroll
      for (int l = 0; l < L; ++l) lane(v, l) = drop_one(lane(v, l), keep, a.seed[b], e + l, BWD);
    }
    if (BWD)
      *hp = v;
    else
      *wp = v;
  }
}

inline bool sizes_ok(int32_t B, int32_t N, int32_t M) { return B >= 1 && B <= MAXB && N >= 1 && M >= 1; }

// the checks and the argument block the two concat entries share; *vec: every
// H_b a multiple of four and every pointer 16-byte aligned
int concat_args(const char* who, int32_t B, int32_t N, int32_t M, const int32_t* H,
                       float* const* h, float keep, const uint64_t* seed, const float* wide,
                       cg::ConcatArgs* a, bool* vec) {
  if (!cg::sizes_ok(B, N, M)) return fail(CG_ERR_ARG, "%s: bad sizes (B=%d N=%d M=%d)", who, B, N, M);
  if (!H || !h || !seed || !wide) return fail(CG_ERR_ARG, "%s: null pointer", who);
  if (!(keep > 0.f && keep <= 1.f)) return fail(CG_ERR_ARG, "%s: keep = %g outside (0, 1]", who, keep);
  *vec = al16(wide);
  int64_t S = 0;
  for (int b = 0; b < B; ++b) {
    if (H[b] < 1) return fail(CG_ERR_ARG, "%s: H[%d] = %d", who, b, H[b]);
    if (!h[b]) return fail(CG_ERR_ARG, "%s: null branch pointer %d", who, b);
    if (h[b] == wide) return fail(CG_ERR_ARG, "%s: the output must not alias an input", who);
    for (int q = 0; q < b; ++q)
      if (h[q] == h[b]) return fail(CG_ERR_ARG, "%s: the branches must be distinct buffers", who);
    a->h[b] = h[b];
    a->seed[b] = seed[b];
    a->H[b] = H[b];
    a->off[b] = int(S);
    S += H[b];
    *vec = *vec && H[b] % 4 == 0 && al16(h[b]);
  }
  if (S > INT32_MAX) return fail(CG_ERR_ARG, "%s: the concatenated row is too long", who);
  a->off[B] = int(S);
  return CG_OK;
}

template <int BWD>
int concat_launch(const cg::ConcatArgs& a, int32_t B, int32_t N, int32_t M, float keep,
                         bool vec, float* wide, void* stream) {
  const int64_t n = int64_t(N) * M * a.off[B];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((cg::k_concat_drop<float4, BWD>), dim3(cg::grid1d(n / 4, 256)), dim3(256), 0, s,
                       a, B, n / 4, keep, wide);
  else
    hipLaunchKernelGGL((cg::k_concat_drop<float, BWD>), dim3(cg::grid1d(n, 256)), dim3(256), 0, s, a,
                       B, n, keep, wide);
  CG_HIP(hipGetLastError());
  return ok();
}

}  // namespace
}  // namespace cg

using cg::al16;
using cg::fail;
using cg::ok;

extern "C" {

int cg_branch_merge_forward(int32_t B, int32_t N, int32_t M, int32_t F, const float* const* y,
                            const float* const* w, float* out, void* stream) {
  if (!cg::sizes_ok(B, N, M) || F < 1)
    return fail(CG_ERR_ARG, "branch_merge_forward: bad sizes (B=%d N=%d M=%d F=%d)", B, N, M, F);
  if (!y || !w || !out) return fail(CG_ERR_ARG, "branch_merge_forward: null pointer");
  cg::MergeArgs a{};
  const int64_t MF = int64_t(M) * F, n = int64_t(N) * MF;
  bool vec = MF % 4 == 0 && al16(out);
  for (int b = 0; b < B; ++b) {
    if (!y[b] || !w[b]) return fail(CG_ERR_ARG, "branch_merge_forward: null y[%d] / w[%d]", b, b);
    if (out == y[b] || out == w[b])
      return fail(CG_ERR_ARG, "branch_merge_forward: out must not alias the inputs");
    a.y[b] = y[b];
    a.w[b] = w[b];
    vec = vec && al16(y[b]) && al16(w[b]);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(cg::k_branch_merge_fwd<float4>, dim3(cg::grid1d(n / 4, 256)), dim3(256), 0, s,
                       a, B, n / 4, MF / 4, reinterpret_cast<float4*>(out));
  else
    hipLaunchKernelGGL(cg::k_branch_merge_fwd<float>, dim3(cg::grid1d(n, 256)), dim3(256), 0, s, a,
                       B, n, MF, out);
  CG_HIP(hipGetLastError());
  return ok();
}

int cg_branch_merge_backward(int32_t B, int32_t N, int32_t M, int32_t F, const float* dout,
                             const float* const* y, const float* const* w, float* const* dy,
                             float* const* dw, int32_t accumulate_dw, void* stream) {
  if (!cg::sizes_ok(B, N, M) || F < 1)
    return fail(CG_ERR_ARG, "branch_merge_backward: bad sizes (B=%d N=%d M=%d F=%d)", B, N, M, F);
  if (!dout || !y || !w) return fail(CG_ERR_ARG, "branch_merge_backward: null pointer");
  cg::MergeArgs a{};
  const int64_t MF = int64_t(M) * F;
  bool vec = MF % 4 == 0 && al16(dout), any = false;
  for (int b = 0; b < B; ++b) {
    if (!y[b] || !w[b]) return fail(CG_ERR_ARG, "branch_merge_backward: null y[%d] / w[%d]", b, b);
    a.y[b] = y[b];
    a.w[b] = w[b];
    a.dy[b] = dy ? dy[b] : nullptr;
    a.dw[b] = dw ? dw[b] : nullptr;
    any = any || a.dy[b] || a.dw[b];
    vec = vec && al16(y[b]) && al16(w[b]) && al16(a.dy[b]) && al16(a.dw[b]);
  }
  if (!any) return fail(CG_ERR_ARG, "branch_merge_backward: every dy and dw entry is null");
  const void* outs[2 * cg::MAXB];
  int nout = 0;
  for (int b = 0; b < B; ++b) {
    if (a.dy[b]) outs[nout++] = a.dy[b];
    if (a.dw[b]) outs[nout++] = a.dw[b];
  }
  for (int i = 0; i < nout; ++i) {
    bool bad = outs[i] == dout;
    for (int b = 0; b < B; ++b) bad = bad || outs[i] == a.y[b] || outs[i] == a.w[b];
    for (int q = 0; q < i; ++q) bad = bad || outs[i] == outs[q];
    if (bad)
      return fail(CG_ERR_ARG, "branch_merge_backward: dy / dw must be distinct buffers that do "
                              "not alias the inputs");
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 block(cg::BM_COLS * cg::BM_LANES);
  if (vec) {
    const int64_t cols = MF / 4;
    hipLaunchKernelGGL(cg::k_branch_merge_bwd<float4>, dim3(unsigned((cols + cg::BM_COLS - 1) / cg::BM_COLS)),
                       block, 0, s, a, B, N, cols, reinterpret_cast<const float4*>(dout),
                       accumulate_dw != 0);
  } else {
    hipLaunchKernelGGL(cg::k_branch_merge_bwd<float>, dim3(unsigned((MF + cg::BM_COLS - 1) / cg::BM_COLS)),
                       block, 0, s, a, B, N, MF, dout, accumulate_dw != 0);
  }
  CG_HIP(hipGetLastError());
  return ok();
}

int cg_concat_drop_forward(int32_t B, int32_t N, int32_t M, const int32_t* H, const float* const* h,
                           float keep, const uint64_t* seed, float* out, void* stream) {
  cg::ConcatArgs a{};
  bool vec = false;
  // (the forward only reads the branches: the kernels share one argument block)
  if (int rc = cg::concat_args("concat_drop_forward", B, N, M, H, const_cast<float* const*>(h), keep, seed,
                           out, &a, &vec))
    return rc;
  return cg::concat_launch<0>(a, B, N, M, keep, vec, out, stream);
}

int cg_concat_drop_backward(int32_t B, int32_t N, int32_t M, const int32_t* H, const float* dx,
                            float keep, const uint64_t* seed, float* const* dh, void* stream) {
  cg::ConcatArgs a{};
  bool vec = false;
  if (int rc = cg::concat_args("concat_drop_backward", B, N, M, H, dh, keep, seed, dx, &a, &vec)) return rc;
  // (the backward only reads dx)
  return cg::concat_launch<1>(a, B, N, M, keep, vec, const_cast<float*>(dx), stream);
}

}  // extern "C"
