// C ABI of the Fourier filter family (see include/cheb_mi355.h): cg_fourier_*,
// cg_gft*, cg_fourier_mix, cg_flstm_* and cg_fres_* with its dropout seam --
// argument validation, workspace layout and the launch sequences.
#include "../../include/cheb_mi355.h"

#include <hip/hip_runtime.h>

#include "abi_checks.h"
#include "cg_internal.h"

using cg::al256;
using cg::fail;
using cg::need_ws;
using cg::ok;

extern "C" {

// ---- Fourier filter (lib/graph_conv.py:83-111) ----------------------------------
static bool fourier_shape_ok(int32_t N, int32_t M, int32_t Fin, int32_t Fout) {
  if (N < 1 || M < 1 || Fin < 1 || Fout < 1 || N > 65535) return false;
  const int64_t big = int64_t(N) * (Fin > Fout ? Fin : Fout) * M;
  return big < (int64_t(1) << 31) && M <= 65535 * 32;
}

static void fourier_ws(int32_t N, int32_t M, int32_t Fin, int32_t Fout, size_t* fwd, size_t* bwd) {
  const size_t xin = size_t(N) * Fin * M * 4, yout = size_t(N) * Fout * M * 4;
  if (fwd) *fwd = (Fin > 1 ? al256(xin) : 0) + al256(yout) + (Fout > 1 ? al256(yout) : 0);
  if (bwd) *bwd = (Fout > 1 ? al256(yout) : 0) + al256(yout) + al256(xin) + (Fin > 1 ? al256(xin) : 0);
}

int cg_fourier_workspace_bytes(int32_t N, int32_t M, int32_t Fin, int32_t Fout, size_t* fwd_bytes,
                               size_t* bwd_bytes) {
  if (!fourier_shape_ok(N, M, Fin, Fout)) return fail(CG_ERR_ARG, "fourier: bad shape");
  fourier_ws(N, M, Fin, Fout, fwd_bytes, bwd_bytes);
  return ok();
}

int cg_fourier_forward(int32_t N, int32_t M, int32_t Fin, int32_t Fout, const float* U,
                       const float* W, const float* x, float* xhat, float* y, void* workspace,
                       size_t ws_bytes, void* stream) {
  if (!U || !W || !x || !xhat || !y) return fail(CG_ERR_ARG, "fourier_forward: null pointer");
  if (!fourier_shape_ok(N, M, Fin, Fout)) return fail(CG_ERR_ARG, "fourier_forward: bad shape");
  size_t need;
  fourier_ws(N, M, Fin, Fout, &need, nullptr);
  if (int rc = need_ws("fourier_forward", workspace, ws_bytes, need)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  const size_t xin = size_t(N) * Fin * M * 4, yout = size_t(N) * Fout * M * 4;
  const float* xs = x;
  if (Fin > 1) {  // [N][M][Fin] -> [N][Fin][M]
    float* xt = reinterpret_cast<float*>(w);
    w += al256(xin);
    CG_HIP(cg::launch_transpose_batched(x, N, M, Fin, xt, s));
    xs = xt;
  }
  float* Yh = reinterpret_cast<float*>(w);
  w += al256(yout);
  // Xh = x U  (every signal row against the eigenvector matrix: U^T x of :90)
  CG_HIP(cg::launch_gemm_f32(false, false, N * Fin, M, M, xs, M, U, M, xhat, M, 1, s));
  CG_HIP(cg::launch_fourier_mix(xhat, W, N, M, Fin, Fout, Yh, s));
  // y = Yh U^T (inverse transform, :97)
  float* yt = Fout > 1 ? reinterpret_cast<float*>(w) : y;
  CG_HIP(cg::launch_gemm_f32(false, true, N * Fout, M, M, Yh, M, U, M, yt, M, 1, s));
  if (Fout > 1) CG_HIP(cg::launch_transpose_batched(yt, N, Fout, M, y, s));
  return ok();
}

int cg_fourier_backward(int32_t N, int32_t M, int32_t Fin, int32_t Fout, const float* U,
                        const float* W, const float* xhat, const float* dy, float* dx, float* dW,
                        void* workspace, size_t ws_bytes, void* stream) {
  if (!U || !W || !xhat || !dy) return fail(CG_ERR_ARG, "fourier_backward: null pointer");
  if (!fourier_shape_ok(N, M, Fin, Fout)) return fail(CG_ERR_ARG, "fourier_backward: bad shape");
  size_t need;
  fourier_ws(N, M, Fin, Fout, nullptr, &need);
  if (int rc = need_ws("fourier_backward", workspace, ws_bytes, need)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  const size_t xin = size_t(N) * Fin * M * 4, yout = size_t(N) * Fout * M * 4;
  const float* dys = dy;
  if (Fout > 1) {
    float* dyt = reinterpret_cast<float*>(w);
    w += al256(yout);
    CG_HIP(cg::launch_transpose_batched(dy, N, M, Fout, dyt, s));
    dys = dyt;
  }
  float* dYh = reinterpret_cast<float*>(w);
  w += al256(yout);
  float* dXh = reinterpret_cast<float*>(w);
  w += al256(xin);
  CG_HIP(cg::launch_gemm_f32(false, false, N * Fout, M, M, dys, M, U, M, dYh, M, 1, s));
  if (dW) CG_HIP(cg::launch_fourier_dw(dYh, xhat, N, M, Fin, Fout, dW, s));
  if (dx) {
    CG_HIP(cg::launch_fourier_mix_t(dYh, W, N, M, Fin, Fout, dXh, s));
    float* dxt = Fin > 1 ? reinterpret_cast<float*>(w) : dx;
    CG_HIP(cg::launch_gemm_f32(false, true, N * Fin, M, M, dXh, M, U, M, dxt, M, 1, s));
    if (Fin > 1) CG_HIP(cg::launch_transpose_batched(dxt, N, Fin, M, dx, s));
  }
  return ok();
}

// ---- gconv-LSTM with the Fourier filter (fourier_lstm.hip) -----------------------
static int check_gft(const char* what, int32_t N, int32_t M, int32_t C, const void* basis,
                     size_t basis_bytes) {
  if (N < 1 || M < 1 || C < 1) return fail(CG_ERR_ARG, "%s: bad shape N=%d M=%d C=%d", what, N, M, C);
  if (M > (1 << 20)) return fail(CG_ERR_ARG, "%s: M=%d too large", what, M);
  if (int64_t(N) * M * C >= (int64_t(1) << 31))
    return fail(CG_ERR_ARG, "%s: N*M*C = %lld exceeds 2^31", what, (long long)(int64_t(N) * M * C));
  if (!basis) return fail(CG_ERR_ARG, "%s: null basis", what);
  if (basis_bytes < cg::gft_basis_bytes(M) || !cg::al16(basis))
    return fail(CG_ERR_ARG, "%s: basis too small or not 16-byte aligned: %zu < %zu", what, basis_bytes,
                cg::gft_basis_bytes(M));
  return CG_OK;
}

static bool flstm_ok(int32_t M, int32_t H, int32_t Fin) {
  return M >= 1 && M <= (1 << 20) && Fin >= 1 && H >= 8 && H % 8 == 0 && H <= 4096;
}

// the summed gate spectrum ghat_x + Wh hhat, [N][M][4H]
static size_t flstm_ws(int32_t N, int32_t M, int32_t H) { return al256(size_t(N) * M * 4 * H * 4); }

int cg_gft_workspace_bytes(int32_t M, size_t* basis_bytes) {
  if (M < 1 || M > (1 << 20) || !basis_bytes) return fail(CG_ERR_ARG, "gft_workspace_bytes: bad arguments");
  *basis_bytes = cg::gft_basis_bytes(M);
  return ok();
}

int cg_gft_prepare(int32_t M, const float* U, void* basis, size_t basis_bytes, void* stream) {
  if (!U) return fail(CG_ERR_ARG, "gft_prepare: null U");
  int rc = check_gft("gft_prepare", 1, M, 1, basis, basis_bytes);
  if (rc) return rc;
  CG_HIP(cg::launch_gft_prepare(U, M, basis, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_gft(int32_t inverse, int32_t N, int32_t M, int32_t C, const void* basis, size_t basis_bytes,
           const float* in, float* out, void* stream) {
  int rc = check_gft("gft", N, M, C, basis, basis_bytes);
  if (rc) return rc;
  if (!in || !out || in == out) return fail(CG_ERR_ARG, "gft: null or aliased in / out");
  CG_HIP(cg::launch_gft(basis, inverse != 0, N, M, C, in, out, cg::option(cg::kOptGemmX3) != 0,
                        nullptr, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_fourier_mix(int32_t form, int64_t R, int32_t M, int32_t Cin, int32_t Cout, const float* W,
                   const float* x, const float* g, const float* add, float* out, void* stream) {
  if (form < 0 || form > 2) return fail(CG_ERR_ARG, "fourier_mix: unknown form %d", form);
  if (R < 1 || M < 1 || Cin < 1 || Cout < 1)
    return fail(CG_ERR_ARG, "fourier_mix: bad shape R=%lld M=%d Cin=%d Cout=%d", (long long)R, M, Cin,
                Cout);
  if (R * M * int64_t(Cin > Cout ? Cin : Cout) >= (int64_t(1) << 31) ||
      int64_t(M) * Cin * Cout >= (int64_t(1) << 31))
    return fail(CG_ERR_ARG, "fourier_mix: a tensor exceeds 2^31 elements");
  if (!out || (form != 2 && !W) || (form != 1 && !x) || (form != 0 && !g))
    return fail(CG_ERR_ARG, "fourier_mix: null operand for form %d", form);
  if (form != 0 && add) return fail(CG_ERR_ARG, "fourier_mix: add is for form 0 only");
  CG_HIP(cg::launch_fmix(form, R, M, Cin, Cout, W, x, g, add, out,
                         reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_flstm_supported(int32_t M, int32_t H, int32_t Fin, int32_t* supported) {
  if (!supported) return fail(CG_ERR_ARG, "flstm_supported: null output");
  if (M < 1 || H < 1 || Fin < 1) return fail(CG_ERR_ARG, "flstm_supported: bad shape");
  *supported = flstm_ok(M, H, Fin) ? 1 : 0;
  return ok();
}

int cg_flstm_workspace_bytes(int32_t N, int32_t M, int32_t H, size_t* bytes) {
  if (N < 1 || M < 1 || H < 1 || !bytes) return fail(CG_ERR_ARG, "flstm_workspace_bytes: bad arguments");
  *bytes = flstm_ws(N, M, H);
  return ok();
}

int cg_flstm_step(int32_t N, int32_t M, int32_t H, int32_t gates, const void* basis,
                  size_t basis_bytes, const float* h_prev, const float* c_prev, const float* ghat_x,
                  const float* Wh, const float* bias, float* c_out, float* h_out, float* act,
                  float* hhat, void* workspace, size_t ws_bytes, void* stream) {
  if (N < 1 || M < 1 || H < 1) return fail(CG_ERR_ARG, "flstm_step: bad shape N=%d M=%d H=%d", N, M, H);
  if (!flstm_ok(M, H, 1)) return fail(CG_ERR_ARG, "flstm_step: needs H %% 8 == 0 (H=%d)", H);
  if (gates != CG_LSTM_GATES_REFERENCE && gates != CG_LSTM_GATES_STANDARD)
    return fail(CG_ERR_ARG, "flstm_step: unknown gate set %d", gates);
  int rc = check_gft("flstm_step", N, M, 4 * H, basis, basis_bytes);
  if (rc) return rc;
  if (!ghat_x || !c_out || !h_out) return fail(CG_ERR_ARG, "flstm_step: null ghat_x / c_out / h_out");
  if (h_prev && (!Wh || !hhat)) return fail(CG_ERR_ARG, "flstm_step: h_prev needs Wh and hhat");
  const size_t need = flstm_ws(N, M, H);
  if (h_prev && (rc = need_ws("flstm_step", workspace, ws_bytes, need))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool x3 = cg::option(cg::kOptGemmX3) != 0;
  const float* ghat = ghat_x;
  if (h_prev) {
    float* sum = static_cast<float*>(workspace);
    CG_HIP(cg::launch_gft(basis, 0, N, M, H, h_prev, hhat, x3, nullptr, s));
    CG_HIP(cg::launch_fmix(0, N, M, H, 4 * H, Wh, hhat, nullptr, ghat_x, sum, s));
    ghat = sum;
  }
  cg::GftGate g{H, gates == CG_LSTM_GATES_REFERENCE ? 0 : 1, bias, c_prev, c_out, h_out, act};
  CG_HIP(cg::launch_gft(basis, 1, N, M, 4 * H, ghat, nullptr, x3, &g, s));
  return ok();
}

// ---- residual block with the Fourier filter (k_gft's EX modes, k_fmix) -------------
// One body per direction serves the plain entries and the LSTM -> head seam
// (cg_fres_*_drop: the DropoutWrapper's mask inside the transforms).  drop ==
// nullptr is the plain call, launch for launch; `what` names the entry in the
// error text.
struct Drop {
  float keep;
  uint64_t seed;
};

static int check_fres(const char* what, int32_t N, int32_t M, int32_t Fin, int32_t Fout,
                      const void* basis, size_t basis_bytes) {
  if (N < 1 || M < 1 || Fin < 1 || Fout < 1)
    return fail(CG_ERR_ARG, "%s: bad shape N=%d M=%d Fin=%d Fout=%d", what, N, M, Fin, Fout);
  int rc = check_gft(what, N, M, Fin > Fout ? Fin : Fout, basis, basis_bytes);
  if (rc) return rc;
  if (int64_t(M) * Fin * Fout >= (int64_t(1) << 31))
    return fail(CG_ERR_ARG, "%s: M*Fin*Fout exceeds 2^31", what);
  return CG_OK;
}

static int check_act(const char* what, int32_t act) {
  if (act != CG_ACT_NONE && act != CG_ACT_RELU)
    return fail(CG_ERR_ARG, "%s: act must be CG_ACT_NONE or CG_ACT_RELU, got %d", what, act);
  return CG_OK;
}

static int check_keep(const char* what, float keep_prob) {
  if (!(keep_prob > 0.f && keep_prob <= 1.f))
    return fail(CG_ERR_ARG, "%s: keep_prob must be in (0, 1], got %g", what, double(keep_prob));
  return CG_OK;
}

// forward: yhat [N][M][Fout].  backward: ghat [N][M][Fout], then dxhat [N][M][Fin].
static void fres_ws(int32_t N, int32_t M, int32_t Fin, int32_t Fout, size_t* fwd, size_t* bwd) {
  const size_t xin = al256(size_t(N) * M * Fin * 4), yout = al256(size_t(N) * M * Fout * 4);
  if (fwd) *fwd = yout;
  if (bwd) *bwd = yout + xin;
}

static int fres_forward_impl(const char* what, int32_t N, int32_t M, int32_t Fin, int32_t Fout,
                             const void* basis, size_t basis_bytes, const float* W, const float* x,
                             const float* residual, int32_t act, float* xhat, float* y,
                             void* workspace, size_t ws_bytes, void* stream, const Drop* drop) {
  int rc = check_fres(what, N, M, Fin, Fout, basis, basis_bytes);
  if (rc) return rc;
  if (!W || !x || !xhat || !y) return fail(CG_ERR_ARG, "%s: null W / x / xhat / y", what);
  if ((rc = check_act(what, act))) return rc;
  size_t need;
  fres_ws(N, M, Fin, Fout, &need, nullptr);
  if ((rc = need_ws(what, workspace, ws_bytes, need))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool x3 = cg::option(cg::kOptGemmX3) != 0;
  float* yhat = static_cast<float*>(workspace);
  if (drop)  // the analysis stages x through the mask
    CG_HIP(cg::launch_gft_drop(basis, 0, N, M, Fin, x, xhat, x3, drop->keep, drop->seed, s));
  else
    CG_HIP(cg::launch_gft(basis, 0, N, M, Fin, x, xhat, x3, nullptr, s));
  CG_HIP(cg::launch_fmix(0, N, M, Fin, Fout, W, xhat, nullptr, nullptr, yhat, s));
  const cg::GftEx e{nullptr, nullptr, residual, act == CG_ACT_RELU, 0};
  CG_HIP(cg::launch_gft_ex(basis, 1, N, M, Fout, yhat, y, x3, e, s));
  return ok();
}

static int fres_backward_impl(const char* what, int32_t N, int32_t M, int32_t Fin, int32_t Fout,
                              const void* basis, size_t basis_bytes, const float* W,
                              const float* xhat, const float* dy, const float* y, int32_t act,
                              float* dz, float* dx, int32_t dx_accumulate, float* dW,
                              void* workspace, size_t ws_bytes, void* stream, const Drop* drop) {
  int rc = check_fres(what, N, M, Fin, Fout, basis, basis_bytes);
  if (rc) return rc;
  if (!W || !xhat || !dy || !dW) return fail(CG_ERR_ARG, "%s: null W / xhat / dy / dW", what);
  if ((rc = check_act(what, act))) return rc;
  if (act == CG_ACT_RELU && !y) return fail(CG_ERR_ARG, "%s: act relu needs y", what);
  if (dx_accumulate && !dx) return fail(CG_ERR_ARG, "%s: dx_accumulate needs dx", what);
  size_t yout, need;  // the forward's size is ghat's, so dxhat's offset
  fres_ws(N, M, Fin, Fout, &yout, &need);
  if (!dx) need = yout;  // no dxhat
  if ((rc = need_ws(what, workspace, ws_bytes, need))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool x3 = cg::option(cg::kOptGemmX3) != 0;
  float* ghat = static_cast<float*>(workspace);
  float* dxhat = reinterpret_cast<float*>(static_cast<char*>(workspace) + yout);
  const cg::GftEx mask{act == CG_ACT_RELU ? y : nullptr, dz, nullptr, 0, 0};
  CG_HIP(cg::launch_gft_ex(basis, 0, N, M, Fout, dy, ghat, x3, mask, s));
  CG_HIP(cg::launch_fmix(2, N, M, Fin, Fout, nullptr, xhat, ghat, nullptr, dW, s));
  if (dx) {
    CG_HIP(cg::launch_fmix(1, N, M, Fin, Fout, W, nullptr, ghat, nullptr, dxhat, s));
    if (drop) {  // the synthesis stores dx through the mask (dx =, never +=)
      CG_HIP(cg::launch_gft_drop(basis, 1, N, M, Fin, dxhat, dx, x3, drop->keep, drop->seed, s));
    } else {
      const cg::GftEx acc{nullptr, nullptr, nullptr, 0, dx_accumulate != 0};
      CG_HIP(cg::launch_gft_ex(basis, 1, N, M, Fin, dxhat, dx, x3, acc, s));
    }
  }
  return ok();
}

int cg_fres_workspace_bytes(int32_t N, int32_t M, int32_t Fin, int32_t Fout, size_t* fwd_bytes,
                            size_t* bwd_bytes) {
  if (N < 1 || M < 1 || Fin < 1 || Fout < 1 || !fwd_bytes || !bwd_bytes)
    return fail(CG_ERR_ARG, "fres_workspace_bytes: bad arguments");
  fres_ws(N, M, Fin, Fout, fwd_bytes, bwd_bytes);
  return ok();
}

int cg_fres_forward(int32_t N, int32_t M, int32_t Fin, int32_t Fout, const void* basis,
                    size_t basis_bytes, const float* W, const float* x, const float* residual,
                    int32_t act, float* xhat, float* y, void* workspace, size_t ws_bytes,
                    void* stream) {
  return fres_forward_impl("fres_forward", N, M, Fin, Fout, basis, basis_bytes, W, x, residual, act,
                           xhat, y, workspace, ws_bytes, stream, nullptr);
}

int cg_fres_backward(int32_t N, int32_t M, int32_t Fin, int32_t Fout, const void* basis,
                     size_t basis_bytes, const float* W, const float* xhat, const float* dy,
                     const float* y, int32_t act, float* dz, float* dx, int32_t dx_accumulate,
                     float* dW, void* workspace, size_t ws_bytes, void* stream) {
  return fres_backward_impl("fres_backward", N, M, Fin, Fout, basis, basis_bytes, W, xhat, dy, y, act,
                            dz, dx, dx_accumulate, dW, workspace, ws_bytes, stream, nullptr);
}

// keep_prob == 1 is the identity: the plain call's launches, so its bits
int cg_fres_forward_drop(int32_t N, int32_t M, int32_t Fin, int32_t Fout, const void* basis,
                         size_t basis_bytes, const float* W, const float* x, float keep_prob,
                         uint64_t seed, const float* residual, int32_t act, float* xhat, float* y,
                         void* workspace, size_t ws_bytes, void* stream) {
  int rc = check_keep("fres_forward_drop", keep_prob);
  if (rc) return rc;
  const Drop d{keep_prob, seed};
  return fres_forward_impl("fres_forward_drop", N, M, Fin, Fout, basis, basis_bytes, W, x, residual,
                           act, xhat, y, workspace, ws_bytes, stream, keep_prob == 1.f ? nullptr : &d);
}

int cg_fres_backward_drop(int32_t N, int32_t M, int32_t Fin, int32_t Fout, const void* basis,
                          size_t basis_bytes, const float* W, const float* xhat, const float* dy,
                          const float* y, int32_t act, float keep_prob, uint64_t seed, float* dz,
                          float* dx, float* dW, void* workspace, size_t ws_bytes, void* stream) {
  int rc = check_keep("fres_backward_drop", keep_prob);
  if (rc) return rc;
  if (!dx) return fail(CG_ERR_ARG, "fres_backward_drop: dx is required");
  const Drop d{keep_prob, seed};
  return fres_backward_impl("fres_backward_drop", N, M, Fin, Fout, basis, basis_bytes, W, xhat, dy, y,
                            act, dz, dx, 0, dW, workspace, ws_bytes, stream,
                            keep_prob == 1.f ? nullptr : &d);
}

}  // extern "C"
