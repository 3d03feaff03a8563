// gconv-LSTM with the Fourier filter (lib/gconv_lstm.py:116-133, :183-221 with
// filter_type = "fourier_conv", lib/filter.py:11-42):
//
//   xh = U^T x, hh = U^T h_{t-1}                       (analysis, per sample)
//   gh[n, m, :] = Wx[m] xh[n, m, :] + Wh[m] hh[n, m, :]  (per frequency m)
//   a = U gh + b ; gates ; c' = f c + i z ; h' = o tanh(c')   (synthesis + epilogue)
//
// Because the inverse transform is linear the x and h parts are summed in the
// spectral domain and synthesised ONCE per step, with the gate update in the
// synthesis' epilogue: the pre-activations never reach HBM.
//
// Spectral tensor layout: sample-major [N][M][C], the same as the vertex-domain
// tensors (frequency m in the place of vertex v).  The steps of a layer are then
// contiguous slices of one [T][N][M][C] buffer, and the stacked (t, n) rows of
// the weight gradient have ONE stride.
//
// Kernels
//   k_gft<X3>  out[n] = A in[n], A = U^T (analysis) or U (synthesis), as ONE
//              GEMM [M x M] x [M x (N C)] whose column j = (n, c) lives at
//              n M C + c with row stride C: no transpose passes.  128 x 128
//              block tile, 4 waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32).
//              X3: the exact three-term bf16 split (split_bf16.h): A comes
//              pre-split, zero-padded and pre-swizzled into MFMA fragment order
//              (k_gft_prepare, once per graph: a fragment is one coalesced
//              16-byte load per lane), the moving operand is split on the fly
//              while it is staged into LDS (each element once per block).
//              !X3: v_mfma_f32_32x32x2_f32 on the padded f32 copies.
//              Gate mode (synthesis, C = 4H): a block's 128 columns are the
//              four gates of 32 units of ONE sample, so the block owns every
//              gate of the (vertex, unit) pairs it finishes; the accumulators
//              go through LDS to lstm_gates.h's lstm_cell_fwd.
//              EX (the residual block, cg_fres_*): the moving operand is staged
//              as in * [mask_y > 0] (the ReLU backward, kept in dz by the first
//              row block of each column tile), and the store is
//              out = act(acc + residual) or out += acc.
//              DR (the LSTM -> head seam, cg_fres_*_drop; a template parameter,
//              so the other instantiations are unchanged): DR = 1 stages the
//              operand as drop_one(in[e], keep, seed, e, 0), DR = 2 stores
//              drop_one(acc, keep, seed, e, 1); e is the flat [N][M][C] index
//              both already form as their load / store address.
//   k_fmix     the per-frequency contraction, one wave per (m, 32 x 32 tile)
//              on v_mfma_f32_32x32x2_f32 with strided operands: forward,
//              transposed and weight-gradient forms are the same kernel with
//              other strides.  One wave runs the whole k range in order, so the
//              weight gradient (k = the stacked rows) is bitwise reproducible.
#include "act.h"
#include "cg_internal.h"
#include "lstm_gates.h"
#include "split_bf16.h"

namespace cg {
namespace {

using x3::bf16x8;
using x3::f32x16;
using x3::Split3;

constexpr int kGftTile = 128;  // block tile (rows and columns); gft_pad() pads M to it

struct GftArgs {
  const void* A;     // prepared operand of this direction (bf16 fragments or f32 k-major)
  const float* in;
  float* out;
  int M, Mp, C, N;
  int gate;          // 1: gate epilogue (C == 4H), column tiles = N * ceil(H / 32)
  int H, ref;        // ref: reference gate functions
  const float* bias;
  const float* c_prev;
  float* c_out;
  float* h_out;
  float* act;
  // EX only
  const float* mask_y;  // staged operand = in * [mask_y > 0]; NULL = in
  float* dz;            // receives the staged operand; NULL = not kept
  const float* res;     // out = act(acc + res); NULL = 0
  int relu, accum;      // accum: out += acc
  // DR only
  float keep;
  unsigned long long seed;
};

// element offset of row 0 of column jj of column tile bx (row stride C); false = padding
__device__ __forceinline__ bool gft_col(const GftArgs& a, int bx, int jj, int64_t* off) {
  if (a.gate) {
    const int UB = (a.H + 31) >> 5;
    const int n = bx / UB, ub = bx - n * UB;
    const int u = ub * 32 + (jj & 31);
    *off = int64_t(n) * a.M * a.C + (jj >> 5) * a.H + u;
    return u < a.H;
  }
  const int64_t j = int64_t(bx) * kGftTile + jj;
  const int64_t n = j / a.C;
  *off = n * a.M * a.C + (j - n * a.C);
  return j < int64_t(a.N) * a.C;
}

template <bool X3, bool EX, int DR = 0>
__global__ __launch_bounds__(256) void k_gft(GftArgs a) {
#pragma clang fp contract(off)
  // X3: 2 buffers x 3 terms x 128 columns x 48 B (16 k as bf16 + 16 B of padding:
  // a 48-byte column stride keeps the 16-byte fragment reads off each other's banks)
  // f32: 2 buffers x 16 k x 132 floats.  Gate epilogue: 64 rows x 129 floats.
  __shared__ __attribute__((aligned(16))) char smem[36864];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int sj = tid & 127, sh = tid >> 7;  // staged column, k half
  int64_t soff;
  const bool sval = gft_col(a, blockIdx.x, sj, &soff);
  const int KS = (a.M + 15) >> 4, KSp = a.Mp >> 4, RT = a.Mp >> 5;
  const int rt0 = blockIdx.y * 4 + wr * 2;  // first 32-row tile of this wave

  f32x16 acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;

  float v[8];
  [[maybe_unused]] float vy[8];  // EX: mask_y at the addresses of v
  auto ldB = [&](int ks) {
    const int k0 = ks * 16 + sh * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool ok = sval && k0 + q < a.M;
      const int64_t e = soff + int64_t(k0 + q) * a.C;
      v[q] = ok ? a.in[e] : 0.f;
      if constexpr (EX) vy[q] = (ok && a.mask_y) ? a.mask_y[e] : 1.f;
    }
  };
  ldB(0);
  for (int ks = 0; ks < KS; ++ks) {
    const int buf = ks & 1;
    if constexpr (EX) {
      // the mask where the loads are consumed, so that they stay in flight during
      // the MFMAs; every row block stages the whole k range of its column tile,
      // so the blocks of row 0 alone keep the masked operand
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = act_relu_grad(v[q], vy[q]);
      if (a.dz && blockIdx.y == 0 && sval) {
        const int k0 = ks * 16 + sh * 8;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (k0 + q < a.M) a.dz[soff + int64_t(k0 + q) * a.C] = v[q];
      }
    }
    if constexpr (DR == 1) {
      // the mask where the loads are consumed (as EX's); a padding element is 0
      // and stays 0, its index addresses nothing
      const int k0 = ks * 16 + sh * 8;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        v[q] = drop_one(v[q], a.keep, a.seed, soff + int64_t(k0 + q) * a.C, 0);
    }
    if constexpr (X3) {
      bf16x8* L = reinterpret_cast<bf16x8*>(smem) + buf * (3 * 128 * 3);
      const Split3 sp = x3::split3(v);
      L[(0 * 128 + sj) * 3 + sh] = sp.hi;
      L[(1 * 128 + sj) * 3 + sh] = sp.mid;
      L[(2 * 128 + sj) * 3 + sh] = sp.lo;
      const bf16x8* Ap = reinterpret_cast<const bf16x8*>(a.A);
      Split3 xa[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int64_t f = (int64_t(rt0 + r) * KSp + ks) * 64 + lane;
        xa[r].hi = Ap[f];
        xa[r].mid = Ap[f + int64_t(RT) * KSp * 64];
        xa[r].lo = Ap[f + 2 * int64_t(RT) * KSp * 64];
      }
      __syncthreads();
      if (ks + 1 < KS) ldB(ks + 1);  // in flight during the MFMAs
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = wc * 64 + c * 32 + i;
        Split3 yb;
        yb.hi = L[(0 * 128 + col) * 3 + h];
        yb.mid = L[(1 * 128 + col) * 3 + h];
        yb.lo = L[(2 * 128 + col) * 3 + h];
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[r][c] = x3::mfma32_x3(xa[r], yb, acc[r][c]);
      }
    } else {
      float* L = reinterpret_cast<float*>(smem) + buf * (16 * 132);
#pragma unroll
      for (int q = 0; q < 8; ++q) L[(sh * 8 + q) * 132 + sj] = v[q];
      const float* Af = reinterpret_cast<const float*>(a.A);
      float av[2][8];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int s = 0; s < 8; ++s)
          av[r][s] = Af[int64_t(ks * 16 + 2 * s + h) * a.Mp + (rt0 + r) * 32 + i];
      __syncthreads();
      if (ks + 1 < KS) ldB(ks + 1);
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float b = L[(2 * s + h) * 132 + wc * 64 + c * 32 + i];
#pragma unroll
          for (int r = 0; r < 2; ++r)
            acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[r][s], b, acc[r][c], 0, 0, 0);
        }
    }
  }

  if (EX || !a.gate) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      int64_t off;
      if (!gft_col(a, blockIdx.x, wc * 64 + c * 32 + i, &off)) continue;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = (rt0 + r) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
          if (row >= a.M) continue;
          const int64_t e = off + int64_t(row) * a.C;
          float val = acc[r][c][q];
          if constexpr (EX) {  // residual and out read at the store's own address
            if (a.res) val = val + a.res[e];
            if (a.relu) val = act_relu(val);
            if (a.accum) val = a.out[e] + val;
          }
          if constexpr (DR == 2) val = drop_one(val, a.keep, a.seed, e, 1);
          a.out[e] = val;
        }
    }
    return;
  }

  // gate epilogue: the block's tile in two halves of 64 rows through LDS
  float* tile = reinterpret_cast<float*>(smem);  // [64][129]
  const int H = a.H;
  const int UB = (H + 31) >> 5;
  const int n = blockIdx.x / UB, ub = blockIdx.x - n * UB;
  const int u = ub * 32 + (tid & 31);
  float bz = 0.f, bi = 0.f, bf = 0.f, bo = 0.f;
  if (a.bias && u < H) bz = a.bias[u], bi = a.bias[H + u], bf = a.bias[2 * H + u], bo = a.bias[3 * H + u];
  for (int half = 0; half < 2; ++half) {
    __syncthreads();  // the k loop's fragment reads / the previous half's gate reads
    if (wr == half) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int q = 0; q < 16; ++q)
            tile[(r * 32 + (q & 3) + 8 * (q >> 2) + 4 * h) * 129 + wc * 64 + c * 32 + i] = acc[r][c][q];
    }
    __syncthreads();
    for (int it = 0; it < 8; ++it) {
      const int rl = it * 8 + (tid >> 5);
      const int row = blockIdx.y * kGftTile + half * 64 + rl;
      if (row >= a.M || u >= H) continue;
      const float* tr = tile + rl * 129 + (tid & 31);
      const float az = tr[0] + bz, ai = tr[32] + bi, af = tr[64] + bf, ao = tr[96] + bo;
      const int64_t e = (int64_t(n) * a.M + row) * H + u;
      const LstmCell s = lstm_cell_fwd(
          az, ai, af, ao, [&] { return a.c_prev ? a.c_prev[e] : 0.f; }, a.ref);
      a.c_out[e] = s.c;
      a.h_out[e] = s.h;
      if (a.act) {
        float* ar = a.act + (int64_t(n) * a.M + row) * 4 * H + u;
        ar[0] = s.z, ar[H] = s.i, ar[2 * H] = s.f, ar[3 * H] = s.o;
      }
    }
  }
}

// One thread per 16-byte fragment unit (direction d, 32-row tile rt, 16-deep k
// step ks, lane): the 8 values A_d[rt 32 + lane % 32][ks 16 + 8 (lane / 32) + j]
// split into the three bf16 terms; A_0 = U^T, A_1 = U, zero outside M.
__global__ __launch_bounds__(256) void k_gft_prepare_x3(const float* __restrict__ U, int M, int Mp,
                                                        bf16x8* __restrict__ out) {
  const int RT = Mp >> 5, KSp = Mp >> 4;
  const int64_t per = int64_t(RT) * KSp * 64, total = 2 * per;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int d = int(e / per);
    const int64_t f = e - d * per;
    const int lane = int(f & 63);
    const int ks = int((f >> 6) % KSp), rt = int((f >> 6) / KSp);
    const int r = rt * 32 + (lane & 31);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = ks * 16 + 8 * (lane >> 5) + j;
      v[j] = (r < M && k < M) ? (d == 0 ? U[int64_t(k) * M + r] : U[int64_t(r) * M + k]) : 0.f;
    }
    const Split3 sp = x3::split3(v);
    bf16x8* o = out + d * 3 * per + f;
    o[0] = sp.hi;
    o[per] = sp.mid;
    o[2 * per] = sp.lo;
  }
}

// f32 operands k-major and zero-padded: out[d][k][r] = A_d[r][k]
__global__ __launch_bounds__(256) void k_gft_prepare_f32(const float* __restrict__ U, int M, int Mp,
                                                         float* __restrict__ out) {
  const int64_t per = int64_t(Mp) * Mp, total = 2 * per;
  for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
    const int d = int(e / per);
    const int64_t f = e - d * per;
    const int k = int(f / Mp), r = int(f - int64_t(k) * Mp);
    out[e] = (r < M && k < M) ? (d == 0 ? U[int64_t(k) * M + r] : U[int64_t(r) * M + k]) : 0.f;
  }
}

struct MixArgs {
  const float* A;
  const float* B;
  const float* add;
  float* C;
  int64_t sAm, sAa, sAk, sBm, sBk, sBb, sCm, sCa, sCb;
  int M, Na, Nb, Kd, ta, tb;
};

// C[m][a][b] = add[m][a][b] + sum_k A[m][a][k] B[m][k][b], every index strided
__global__ __launch_bounds__(256) void k_fmix(MixArgs p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int i = lane & 31, h = lane >> 5;
  const int64_t gw = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int per = p.ta * p.tb;
  if (gw >= int64_t(p.M) * per) return;
  const int m = int(gw / per), rem = int(gw - int64_t(m) * per);
  const int at = rem / p.tb, bt = rem - at * p.tb;
  const int ai = at * 32 + i, bi = bt * 32 + i;
  const bool aok = ai < p.Na, bok = bi < p.Nb;
  const float* Ap = p.A + m * p.sAm + (aok ? ai : 0) * p.sAa;
  const float* Bp = p.B + m * p.sBm + (bok ? bi : 0) * p.sBb;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  for (int k0 = 0; k0 < p.Kd; k0 += 8) {  // four k pairs' loads in flight
    float av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + 2 * s + h;
      const bool kok = k < p.Kd;
      av[s] = (aok && kok) ? Ap[k * p.sAk] : 0.f;
      bv[s] = (bok && kok) ? Bp[k * p.sBk] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
  }
  if (!bok) return;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int ar = at * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
    if (ar >= p.Na) continue;
    const int64_t o = m * p.sCm + ar * p.sCa + bi * p.sCb;
    p.C[o] = p.add ? p.add[o] + acc[q] : acc[q];
  }
}

inline int grid_1d(int64_t n, int per_block) {
  const int64_t g = (n + per_block - 1) / per_block;
  return int(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

}  // namespace

int gft_pad(int M) { return (M + kGftTile - 1) / kGftTile * kGftTile; }

size_t gft_basis_bytes(int M) {
  const size_t Mp = size_t(gft_pad(M));
  return 2 * 3 * Mp * Mp * 2 + 2 * Mp * Mp * 4;  // bf16 fragments, then the f32 copies
}

hipError_t launch_gft_prepare(const float* U, int M, void* basis, hipStream_t s) {
  const int Mp = gft_pad(M);
  const int64_t units = 2 * int64_t(Mp >> 5) * (Mp >> 4) * 64;
  hipLaunchKernelGGL(k_gft_prepare_x3, dim3(grid_1d(units, 256)), dim3(256), 0, s, U, M, Mp,
                     static_cast<bf16x8*>(basis));
  float* f32 = reinterpret_cast<float*>(static_cast<char*>(basis) + size_t(6) * Mp * Mp * 2);
  hipLaunchKernelGGL(k_gft_prepare_f32, dim3(grid_1d(2 * int64_t(Mp) * Mp, 256)), dim3(256), 0, s, U,
                     M, Mp, f32);
  return hipGetLastError();
}

// One launch of k_gft in the mode the call needs: plain (all null), the gate
// epilogue g, the residual block's EX modes e, or the seam's dropout d (DR 1
// on the analysis' operand, DR 2 on the synthesis' store).
struct GftDrop {
  float keep;
  unsigned long long seed;
};

template <bool EX, int DR>
static void gft_launch(bool x3, dim3 grid, hipStream_t s, const GftArgs& a) {
  if (x3)
    hipLaunchKernelGGL((k_gft<true, EX, DR>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((k_gft<false, EX, DR>), grid, dim3(256), 0, s, a);
}

static hipError_t launch_gft_any(const void* basis, int inverse, int N, int M, int C, const float* in,
                                 float* out, bool x3, const GftGate* g, const GftEx* e,
                                 const GftDrop* d, hipStream_t s) {
  GftArgs a{};
  const size_t Mp = size_t(gft_pad(M));
  const char* b = static_cast<const char*>(basis);
  // direction 0 = U^T (analysis), 1 = U (synthesis)
  a.A = x3 ? b + size_t(inverse ? 1 : 0) * 3 * Mp * Mp * 2
           : b + 6 * Mp * Mp * 2 + size_t(inverse ? 1 : 0) * Mp * Mp * 4;
  a.in = in;
  a.out = out;
  a.M = M, a.Mp = int(Mp), a.C = C, a.N = N;
  int64_t ctiles = (int64_t(N) * C + kGftTile - 1) / kGftTile;
  if (g) {
    a.gate = 1, a.H = g->H, a.ref = g->gates == CG_LSTM_GATES_REFERENCE;
    a.bias = g->bias, a.c_prev = g->c_prev, a.c_out = g->c_out, a.h_out = g->h_out, a.act = g->act;
    ctiles = int64_t(N) * ((g->H + 31) / 32);
  }
  if (ctiles > 2147483647) return hipErrorInvalidValue;
  const dim3 grid(unsigned(ctiles), unsigned(Mp / kGftTile));
  if (d) {
    a.keep = d->keep, a.seed = d->seed;
    if (inverse)
      gft_launch<false, 2>(x3, grid, s, a);
    else
      gft_launch<false, 1>(x3, grid, s, a);
  } else if (e) {
    a.mask_y = e->mask_y, a.dz = e->dz, a.res = e->residual;
    a.relu = e->relu, a.accum = e->accumulate;
    gft_launch<true, 0>(x3, grid, s, a);
  } else {
    gft_launch<false, 0>(x3, grid, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_gft(const void* basis, int inverse, int N, int M, int C, const float* in,
                      float* out, bool x3, const GftGate* g, hipStream_t s) {
  return launch_gft_any(basis, inverse, N, M, C, in, out, x3, g, nullptr, nullptr, s);
}

hipError_t launch_gft_ex(const void* basis, int inverse, int N, int M, int C, const float* in,
                         float* out, bool x3, const GftEx& e, hipStream_t s) {
  return launch_gft_any(basis, inverse, N, M, C, in, out, x3, nullptr, &e, nullptr, s);
}

hipError_t launch_gft_drop(const void* basis, int inverse, int N, int M, int C, const float* in,
                           float* out, bool x3, float keep, unsigned long long seed, hipStream_t s) {
  const GftDrop d{keep, seed};
  return launch_gft_any(basis, inverse, N, M, C, in, out, x3, nullptr, nullptr, &d, s);
}

hipError_t launch_fmix(int form, int64_t R, int M, int Cin, int Cout, const float* W, const float* x,
                       const float* g, const float* add, float* out, hipStream_t s) {
  MixArgs p{};
  p.M = M;
  p.add = add;
  p.C = out;
  const int64_t sx = int64_t(M) * Cin, sg = int64_t(M) * Cout;
  if (form == 0) {  // out[r][m][o] = add + sum_i x[r][m][i] W[m][o][i]
    p.A = x, p.sAm = Cin, p.sAa = sx, p.sAk = 1;
    p.B = W, p.sBm = int64_t(Cout) * Cin, p.sBk = 1, p.sBb = Cin;
    p.sCm = Cout, p.sCa = sg, p.sCb = 1;
    p.Na = int(R), p.Nb = Cout, p.Kd = Cin;
  } else if (form == 1) {  // out[r][m][i] = sum_o g[r][m][o] W[m][o][i]
    p.A = g, p.sAm = Cout, p.sAa = sg, p.sAk = 1;
    p.B = W, p.sBm = int64_t(Cout) * Cin, p.sBk = Cin, p.sBb = 1;
    p.sCm = Cin, p.sCa = sx, p.sCb = 1;
    p.Na = int(R), p.Nb = Cin, p.Kd = Cout;
  } else {  // out[m][o][i] = sum_r g[r][m][o] x[r][m][i]   (r in order)
    p.A = g, p.sAm = Cout, p.sAa = 1, p.sAk = sg;
    p.B = x, p.sBm = Cin, p.sBk = sx, p.sBb = 1;
    p.sCm = int64_t(Cout) * Cin, p.sCa = Cin, p.sCb = 1;
    p.Na = Cout, p.Nb = Cin, p.Kd = int(R);
  }
  p.ta = (p.Na + 31) / 32, p.tb = (p.Nb + 31) / 32;
  const int64_t waves = int64_t(M) * p.ta * p.tb;
  if ((waves + 3) / 4 > 2147483647) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_fmix, dim3(unsigned((waves + 3) / 4)), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace cg
