// The dense LSTM baseline of lib/gconvRNN.py::Model (model_type='lstm', :257-262,
// :280-285, :314-315): a TF 1.x BasicLSTMCell under static_rnn from the zero
// state, every step a flat [N, num_node] vector.  Two kernels, one launch each:
//
// k_dlstm_fwd: all T steps.  gx [T][N][4H] is the input projection of every step
// (one GEMM, the caller's); gate blocks i | j | f | o, TF's column order:
//   a   = (gx_t + h_{t-1} Wh) + bias
//   c_t = c_{t-1} * sigmoid(a_f + forget_bias) + sigmoid(a_i) * tanh(a_j)
//   h_t = tanh(c_t) * sigmoid(a_o)
// (another cell than lstm_gates.h's lstm_cell_fwd: its own expressions stay here)
// k_dlstm_bwd: the whole BPTT, t = T-1 .. 0: dh = dhs_t + dh_rec, the gate
// backward from act and cs, dpre_t stored, dh_rec = dpre_t Wh^T.
//
// Tiling (both): a workgroup owns 16 batch rows for the whole sequence and has
// H/16 waves; wave w owns hidden units [16w, 16w + 16).  The products run
// TRANSPOSED on v_mfma_f32_16x16x4_f32 (exact f32) so that one lane ends up
// with all four gates of the same (row, unit):
//   forward   D^T = Wh^T h^T: A = Wh[k][gate column], B = h[row][k]; four
//             accumulators (one per gate block), lane (r = lane & 15,
//             q = lane >> 4) holds row r, units 16w + 4q + 0..3 of each gate
//   backward  D^T = Wh dpre^T: A = Wh[unit][column], B = dpre[row][column]; the
//             4H columns are dealt round-robin to four accumulators that are
//             added in a fixed order: the same lane ownership
// c (forward) and dc, dh_rec (backward) never leave registers.  h_t / dpre_t go
// through a double-buffered LDS tile [k][16 rows] (the next product's B operand,
// one ds_read_b32 per lane at 64 ks + lane, conflict-free): ONE barrier a step.
// Step 0 of the forward and step 0 of the backward run no product.  Batch rows
// are independent, so nothing here waits on another workgroup: no cooperative
// launch, no flags, no atomics.  Every sum has a fixed order: two calls agree
// bitwise, and the act == NULL forward runs the same arithmetic.
//
// Wh: staged into LDS once where both kernels' images fit in 160 KB (H <= 80),
// with a row stride that puts the lanes' four k rows on disjoint banks
// (forward [H][4H + 16]; backward transposed, [4H][H or H + 16]); above that
// the A operand is read from global memory each step (Wh is <= 256 KB: L2).
//   LDS bytes      H = 16     32     48     64     80   |  96    112    128
//   forward         7168  22528  46080  77824 117760   | 12288  14336  16384
//   backward       12288  40960  61440 114688 143360   | 49152  57344  65536
//
// A ragged last tile computes its dead rows from zeros and stores nothing for
// them.  gx, hs, cs, act, dhs and dpre move as float4 (16-byte aligned, checked
// by the entry); Wh and bias are read one float at a time (views at any offset).
#include "cg_internal.h"
#include "launch.h"
#include "lstm_gates.h"

namespace cg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DlstmFwdArgs {
  int T, N, H;
  const float* gx;
  const float* Wh;
  const float* bias;
  float forget_bias;
  float* hs;
  float* cs;
  float* act;  // NULL: inference
};

struct DlstmBwdArgs {
  int T, N, H;
  const float* dhs;
  const float* act;
  const float* cs;
  const float* Wh;
  float* dpre;
};

__device__ __forceinline__ float4 ld4(const float* p, bool live) {
  return live ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void st4(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float at(const float4& v, int e) {
  return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w;
}

__host__ __device__ inline int fwd_stride(int H) { return 4 * H + 16; }
__host__ __device__ inline int bwd_stride(int H) { return H % 32 == 0 ? H + 16 : H; }

template <bool kRes>
__global__ __launch_bounds__(512) void k_dlstm_fwd(DlstmFwdArgs a) {
#pragma clang fp contract(off)
  extern __shared__ float lds[];
  const int H = a.H, G = 4 * H;
  const int tid = int(threadIdx.x), lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int S = kRes ? fwd_stride(H) : G;
  float* hbuf = lds + (kRes ? H * S : 0);  // [2][H][16]
  if (kRes)
    for (int i = tid; i < H * G; i += int(blockDim.x)) lds[(i / G) * S + i % G] = a.Wh[i];
  const float* W = kRes ? lds : a.Wh;
  const int64_t n = int64_t(blockIdx.x) * 16 + r;
  const bool live = n < a.N;
  const int u0 = w * 16 + q * 4;
  float b[4][4], c[4] = {0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < 4; ++g)
    for (int e = 0; e < 4; ++e) b[g][e] = a.bias[g * H + u0 + e];
  const float* wp = W + q * S + w * 16 + r;  // A: Wh[4 ks + q][g H + 16 w + r]
  __syncthreads();
  for (int t = 0; t < a.T; ++t) {
    const int64_t row = int64_t(t) * a.N + n;
    float4 x[4];
    for (int g = 0; g < 4; ++g) x[g] = ld4(a.gx + row * G + g * H + u0, live);
    f32x4 acc[4];
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t > 0) {
      const float* hb = hbuf + (t & 1) * H * 16;  // h_{t-1}
      for (int ks = 0; ks < H / 4; ++ks) {
        const float bv = hb[64 * ks + lane];  // B: h[row r][4 ks + q]
        const float* wk = wp + 4 * ks * S;
#pragma unroll
        for (int g = 0; g < 4; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wk[g * H], bv, acc[g], 0, 0, 0);
      }
    }
    float* hn = hbuf + ((t + 1) & 1) * H * 16;
    float hv[4], av[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gi = gate_sigmoid((at(x[0], e) + acc[0][e]) + b[0][e]);
      const float gj = gate_tanh((at(x[1], e) + acc[1][e]) + b[1][e]);
      const float gf = gate_sigmoid(((at(x[2], e) + acc[2][e]) + b[2][e]) + a.forget_bias);
      const float go = gate_sigmoid((at(x[3], e) + acc[3][e]) + b[3][e]);
      c[e] = c[e] * gf + gi * gj;
      hv[e] = gate_tanh(c[e]) * go;
      av[0][e] = gi, av[1][e] = gj, av[2][e] = gf, av[3][e] = go;
      hn[(u0 + e) * 16 + r] = hv[e];
    }
    if (live) {
      st4(a.hs + row * H + u0, hv);
      st4(a.cs + row * H + u0, c);
      if (a.act)
        for (int g = 0; g < 4; ++g) st4(a.act + row * G + g * H + u0, av[g]);
    }
    __syncthreads();
  }
}

template <bool kRes>
__global__ __launch_bounds__(512) void k_dlstm_bwd(DlstmBwdArgs a) {
#pragma clang fp contract(off)
  extern __shared__ float lds[];
  const int H = a.H, G = 4 * H;
  const int tid = int(threadIdx.x), lane = tid & 63, w = tid >> 6, r = lane & 15, q = lane >> 4;
  const int S = bwd_stride(H);
  float* dpbuf = lds + (kRes ? G * S : 0);  // [2][4H][16]
  if (kRes)  // transposed: Wt[column][unit]
    for (int i = tid; i < H * G; i += int(blockDim.x)) lds[(i % G) * S + i / G] = a.Wh[i];
  const int64_t n = int64_t(blockIdx.x) * 16 + r;
  const bool live = n < a.N;
  const int u0 = w * 16 + q * 4;
  // A: Wh[16 w + r][4 ks + q]
  const float* wp = kRes ? lds + q * S + w * 16 + r : a.Wh + int64_t(w * 16 + r) * G + q;
  const int wstep = kRes ? 4 * S : 4;
  float dc[4] = {0.f, 0.f, 0.f, 0.f}, dhr[4] = {0.f, 0.f, 0.f, 0.f};
  float4 ct = ld4(a.cs + (int64_t(a.T - 1) * a.N + n) * H + u0, live);
  int cur = 0;
  for (int t = a.T - 1; t >= 0; --t) {
    const int64_t row = int64_t(t) * a.N + n;
    const float4 dh4 = ld4(a.dhs + row * H + u0, live);
    float4 g4[4];
    for (int g = 0; g < 4; ++g) g4[g] = ld4(a.act + row * G + g * H + u0, live);
    const float4 cp = ld4(a.cs + (row - a.N) * H + u0, live && t > 0);
    float* dp = dpbuf + cur * G * 16;
    float d[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gi = at(g4[0], e), gj = at(g4[1], e), gf = at(g4[2], e), go = at(g4[3], e);
      const float dh = at(dh4, e) + dhr[e];
      const float tc = gate_tanh(at(ct, e));
      const float dcv = dc[e] + (dh * go) * (1.f - tc * tc);
      d[0][e] = (dcv * gj) * (gi * (1.f - gi));
      d[1][e] = (dcv * gi) * (1.f - gj * gj);
      d[2][e] = (dcv * at(cp, e)) * (gf * (1.f - gf));
      d[3][e] = (dh * tc) * (go * (1.f - go));
      dc[e] = dcv * gf;
      for (int g = 0; g < 4; ++g) dp[(g * H + u0 + e) * 16 + r] = d[g][e];
    }
    if (live)
      for (int g = 0; g < 4; ++g) st4(a.dpre + row * G + g * H + u0, d[g]);
    ct = cp;
    if (t == 0) break;  // uniform: step 0 ran no h product
    __syncthreads();
    f32x4 acc[4];
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k4 = 0; k4 < H; k4 += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ks = k4 + j;
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[ks * wstep], dp[64 * ks + lane], acc[j], 0,
                                                      0, 0);
      }
    }
    for (int e = 0; e < 4; ++e) dhr[e] = (acc[0][e] + acc[1][e]) + (acc[2][e] + acc[3][e]);
    cur ^= 1;
  }
}

}  // namespace

size_t dlstm_lds_bytes(int H, bool backward, bool resident) {
  const size_t tile = size_t(backward ? 4 * H : H) * 16 * 2;
  const size_t w = !resident ? 0 : backward ? size_t(4 * H) * bwd_stride(H) : size_t(H) * fwd_stride(H);
  return (w + tile) * sizeof(float);
}

bool dlstm_ok(int H) { return H >= 16 && H <= 128 && H % 16 == 0; }

bool dlstm_resident(int H) {
  return dlstm_lds_bytes(H, false, true) <= size_t(kLdsBytes) &&
         dlstm_lds_bytes(H, true, true) <= size_t(kLdsBytes);
}

hipError_t launch_dlstm_fwd(int T, int N, int H, const float* gx, const float* Wh,
                            const float* bias, float forget_bias, float* hs, float* cs, float* act,
                            hipStream_t s) {
  const DlstmFwdArgs a{T, N, H, gx, Wh, bias, forget_bias, hs, cs, act};
  const bool res = dlstm_resident(H);
  const dim3 grid(unsigned((N + 15) / 16)), block(unsigned(4 * H));
  return launch_big_lds(res ? k_dlstm_fwd<true> : k_dlstm_fwd<false>, grid, block,
                        dlstm_lds_bytes(H, false, res), s, a);
}

hipError_t launch_dlstm_bwd(int T, int N, int H, const float* dhs, const float* act,
                            const float* cs, const float* Wh, float* dpre, hipStream_t s) {
  const DlstmBwdArgs a{T, N, H, dhs, act, cs, Wh, dpre};
  const bool res = dlstm_resident(H);
  const dim3 grid(unsigned((N + 15) / 16)), block(unsigned(4 * H));
  return launch_big_lds(res ? k_dlstm_bwd<true> : k_dlstm_bwd<false>, grid, block,
                        dlstm_lds_bytes(H, true, res), s, a);
}

}  // namespace cg
