// The per-step output head of the structured-sequence gconv-LSTM and its
// softmax cross-entropy over the vertices (lib/gconvRNN.py:306-317, :326-340),
// forward and backward in ONE pass over hs [T][N][M][H]:
//   hd[m,:]   = drop_one(hs[t,n,m,:], keep, seed, e, 0)      (keep == 1: hd = hs)
//   logit[m]  = hd[m,:] . w + b
//   ce[t,n]   = log sum_m exp(logit[m]) - logit[label[t,n]]  (max-subtracted)
//   dlogit[m] = loss_scale (softmax[m] - [m == label])
//   dw = sum dlogit[m] hd[m,:],  db = sum dlogit[m],  dhs = drop_one(dlogit[m] w, ., 1)
//
// k_seq_xent: one 256-thread workgroup per (t, n).  A row of H values is owned
// by LPR lanes (a power of two <= 64, up to four columns per lane), the
// workgroup's 256 / LPR lane groups take the rows round robin.  Phase 1 streams
// the tile once: a lane group reduces its row's logit by xor shuffles, keeps it
// in LDS (M floats) and folds the row into its own online softmax state
// (running max, sum, and S = sum exp(logit - max) hd[m,:] in the lanes' column
// registers).  The groups' states are then combined in group order, which
// gives log-sum-exp and, with the label's row stashed on the way,
//   sum_m dlogit[m] hd[m,:] = loss_scale (S / sum - hd[label,:])
// without holding the 128 KB tile.  Phase 2 writes dhs from the logits in LDS
// and w in registers: no second read of hs.
//
// No floating-point atomics: a pair's dw, db and ce go to the workspace
// ([H + 2][T*N], row major so the reduction reads them coalesced) and
// k_seq_xent_sum adds them in a fixed order -- two calls agree bitwise.
//
// A label outside [0, M) is never used as an index: that pair's ce, dhs and
// partials are NaN (TF's GPU kernel does the same).
#include "cg_internal.h"

#include <cmath>

namespace cg {
namespace {

constexpr int kXT = 256;  // threads of k_seq_xent

struct XentArgs {
  const float* hs;
  const float* w;
  const float* b;
  const int32_t* labels;
  int T, N, M, H;
  int lpr;  // lanes per row
  float keep;
  unsigned long long seed;
  float loss_scale;
  float* logits;  // [N][M][T] or NULL
  float* ce;      // [T][N] or NULL
  float* dhs;     // NULL: forward only
  float* part;    // [H + 2][T*N]: dw columns, db, ce
  float* lgbuf;   // [T*N][M] logits scratch of the GL build
};

// the DropoutWrapper's mask on the head's operand and on its gradient: the
// arithmetic of k_dropout (drop_one), uncontracted
__device__ __forceinline__ float xent_drop(float x, const XentArgs& a, int64_t e, int bwd) {
#pragma clang fp contract(off)
  return drop_one(x, a.keep, a.seed, e, bwd);
}

// VEC: H % 4 == 0 and 16-byte aligned hs / dhs, a lane owns columns 4c .. 4c+3
// (one dwordx4); else columns c, c + LPR, c + 2 LPR, c + 3 LPR.
// GL: the pair's logits live in global scratch instead of LDS (M past the LDS budget).
template <bool VEC, bool GL>
__global__ __launch_bounds__(kXT) void k_seq_xent(XentArgs a) {
  extern __shared__ float s_lg[];     // [M] logits (!GL)
  __shared__ float s_S[kXT * 4];      // [G][LPR * 4] the groups' S
  __shared__ float s_mx[kXT], s_sum[kXT], s_fac[kXT];
  __shared__ float s_hl[256];         // hd[label, :]
  __shared__ float s_red[kXT / 64];

  const int tid = int(threadIdx.x);
  const int M = a.M, H = a.H, LPR = a.lpr;
  const int G = kXT / LPR, grp = tid / LPR, c = tid % LPR;
  const int64_t p = blockIdx.x, P = int64_t(a.T) * a.N;
  const int64_t base = p * M * H;
  float* lg = GL ? a.lgbuf + p * M : s_lg;
  const int lab = a.labels[p];
  const bool lab_ok = lab >= 0 && lab < M;
  const bool drop = a.keep < 1.f;
  const float nan = __builtin_nanf("");

  int col[4];
  float wv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    col[j] = VEC ? 4 * c + j : c + j * LPR;
    wv[j] = col[j] < H ? a.w[col[j]] : 0.f;
  }
  const float bias = a.b[0];

  // ---- phase 1: one read of the tile ----------------------------------------------
  constexpr int U = 4;  // rows in flight per lane group
  float mx = -INFINITY, sum = 0.f, S[4] = {0.f, 0.f, 0.f, 0.f};
  for (int m0 = grp; m0 - grp < M; m0 += U * G) {  // the same trip count in every group
    float v[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int m = m0 + u * G;
      const float* row = a.hs + base + int64_t(m) * H;
      if (VEC) {
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < M && col[0] < H) q = *reinterpret_cast<const float4*>(row + col[0]);
        v[u][0] = q.x, v[u][1] = q.y, v[u][2] = q.z, v[u][3] = q.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[u][j] = (m < M && col[j] < H) ? row[col[j]] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int m = m0 + u * G;
      const bool live = m < M;  // uniform over the lane group
      if (drop && live) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col[j] < H) v[u][j] = xent_drop(v[u][j], a, base + int64_t(m) * H + col[j], 0);
      }
      float dot = v[u][0] * wv[0];
      dot = fmaf(v[u][1], wv[1], dot);
      dot = fmaf(v[u][2], wv[2], dot);
      dot = fmaf(v[u][3], wv[3], dot);
      for (int o = LPR >> 1; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
      if (live) {
        const float logit = dot + bias;
        if (c == 0) lg[m] = logit;
        if (m == lab) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (col[j] < H) s_hl[col[j]] = v[u][j];
        }
        // online softmax: one exponential per row
        const float d = logit - mx;
        const float ex = expf(-fabsf(d));
        const float keep_old = d > 0.f ? ex : 1.f, e_new = d > 0.f ? 1.f : ex;
        mx = d > 0.f ? logit : mx;
        sum = fmaf(sum, keep_old, e_new);
#pragma unroll
        for (int j = 0; j < 4; ++j) S[j] = fmaf(S[j], keep_old, e_new * v[u][j]);
      }
    }
  }
  if (c == 0) s_mx[grp] = mx, s_sum[grp] = sum;
#pragma unroll
  for (int j = 0; j < 4; ++j) s_S[grp * (4 * LPR) + (VEC ? 4 * c + j : c + j * LPR)] = S[j];
  __syncthreads();

  // ---- the groups' states in group order ---------------------------------------------
  float MX = -INFINITY;
  for (int g = 0; g < G; ++g) MX = fmaxf(MX, s_mx[g]);
  if (tid < G) s_fac[tid] = expf(s_mx[tid] - MX);  // a group that saw no row: exp(-inf) = 0
  __syncthreads();
  float SUM = 0.f;
  for (int g = 0; g < G; ++g) SUM = fmaf(s_sum[g], s_fac[g], SUM);
  const float lsum = logf(SUM);  // log-sum-exp = MX + lsum
  if (a.dhs && tid < H) {
    float Sf = 0.f;
    for (int g = 0; g < G; ++g) Sf = fmaf(s_S[g * (4 * LPR) + tid], s_fac[g], Sf);
    a.part[int64_t(tid) * P + p] = lab_ok ? a.loss_scale * (Sf / SUM - s_hl[tid]) : nan;
  }
  if (tid == 0) {
    const float cev = lab_ok ? lsum + (MX - lg[lab]) : nan;
    a.part[int64_t(H + 1) * P + p] = cev;
    if (a.ce) a.ce[p] = cev;
  }
  if (a.logits) {  // pred_out [N][M][T]
    const int64_t t = p / a.N, n = p % a.N;
    for (int m = tid; m < M; m += kXT) a.logits[(n * M + m) * a.T + t] = lg[m];
  }
  if (!a.dhs) return;

  // ---- phase 2: dhs from the logits, one write of the tile ----------------------------
  float dbacc = 0.f;
  for (int m = grp; m < M; m += G) {
    float dl = a.loss_scale * (expf((lg[m] - MX) - lsum) - (m == lab ? 1.f : 0.f));
    if (!lab_ok) dl = nan;
    if (c == 0) dbacc += dl;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = dl * wv[j];
      if (drop && col[j] < H) o[j] = xent_drop(o[j], a, base + int64_t(m) * H + col[j], 1);
    }
    float* row = a.dhs + base + int64_t(m) * H;
    if (VEC) {
      if (col[0] < H) *reinterpret_cast<float4*>(row + col[0]) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col[j] < H) row[col[j]] = o[j];
    }
  }
  for (int o = 32; o > 0; o >>= 1) dbacc += __shfl_xor(dbacc, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = dbacc;
  __syncthreads();
  if (tid == 0) {
    float db = 0.f;
    for (int q = 0; q < kXT / 64; ++q) db += s_red[q];
    a.part[int64_t(H) * P + p] = db;
  }
}

// One wave per output: rows j < H of part -> dw[j], row H -> db, row H + 1 ->
// loss = loss_scale * sum ce.  Lane l adds the pairs l, l + 64, ... in order,
// then a fixed xor tree.
__global__ __launch_bounds__(256) void k_seq_xent_sum(const float* __restrict__ part, int64_t P, int H,
                                                      float loss_scale, int grads, float* loss,
                                                      float* dw, float* db) {
  const int j = int(blockIdx.x) * 4 + int(threadIdx.x >> 6);
  const int lane = int(threadIdx.x & 63);
  if (j > H + 1 || (!grads && j != H + 1)) return;  // wave-uniform
  const float* row = part + int64_t(j) * P;
  float acc = 0.f;
  for (int64_t q = lane; q < P; q += 64) acc += row[q];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane) return;
  if (j < H) dw[j] = acc;
  else if (j == H) *db = acc;
  else *loss = loss_scale * acc;
}

}  // namespace

// LDS budget for a pair's logits; past it they go through global scratch
constexpr int kXentLdsM = 8192;

size_t seq_xent_ws_bytes(int64_t P, int M, int H) {
  size_t fl = size_t(H + 2) * size_t(P);
  if (M > kXentLdsM) fl += size_t(P) * size_t(M);
  return align16(fl * sizeof(float));
}

hipError_t launch_seq_xent(const float* hs, const float* w, const float* b, const int32_t* labels,
                           int T, int N, int M, int H, float keep, unsigned long long seed,
                           float loss_scale, float* logits, float* ce, float* loss, float* dhs,
                           float* dw, float* db, float* ws, hipStream_t s) {
  const int64_t P = int64_t(T) * N;
  const bool vec = H % 4 == 0 && (reinterpret_cast<uintptr_t>(hs) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(dhs) & 15) == 0;
  const int cols = vec ? H / 4 : H;
  int lpr = 1;
  while (lpr < cols && lpr < 64) lpr <<= 1;
  const bool gl = M > kXentLdsM;
  XentArgs a{hs, w, b, labels, T, N, M, H, lpr, keep, seed, loss_scale, logits, ce, dhs, ws,
             ws + size_t(H + 2) * size_t(P)};
  const size_t lds = gl ? 0 : size_t(M) * sizeof(float);
  auto k = vec ? (gl ? k_seq_xent<true, true> : k_seq_xent<true, false>)
               : (gl ? k_seq_xent<false, true> : k_seq_xent<false, false>);
  hipLaunchKernelGGL(k, dim3(unsigned(P)), dim3(kXT), lds, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int grads = dhs != nullptr;
  hipLaunchKernelGGL(k_seq_xent_sum, dim3(unsigned((H + 2 + 3) / 4)), dim3(256), 0, s, ws, P, H,
                     loss_scale, grads, loss, dw, db);
  return hipGetLastError();
}

}  // namespace cg
