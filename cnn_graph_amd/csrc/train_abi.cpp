// C ABI of the training ops (see include/cheb_mi355.h): loss, dropout, clip,
// seq_xent, class_xent, slice and stack, weight and bias gradients, bias_act, gemm, pooling,
// perm, the batch gather and the optimizers -- argument validation and the launches.
#include "../../include/cheb_mi355.h"

#include <hip/hip_runtime.h>

#include "abi_checks.h"
#include "cg_internal.h"

using cg::al256;
using cg::dw_slab_bytes;
using cg::fail;
using cg::need_ws;
using cg::ok;

extern "C" {

int cg_mse_loss_workspace_bytes(int64_t n, size_t* bytes) {
  if (!bytes || n < 1) return fail(CG_ERR_ARG, "mse_loss: bad arguments");
  *bytes = al256(size_t(cg::mse_chunks(n)) * 4);
  return ok();
}

int cg_mse_loss(const float* pred, const float* labels, int64_t n, float* loss, float* dpred,
                void* workspace, size_t ws_bytes, void* stream) {
  if (!pred || !labels || !loss || n < 1) return fail(CG_ERR_ARG, "mse_loss: bad arguments");
  if (int rc = need_ws("mse_loss", workspace, ws_bytes, al256(size_t(cg::mse_chunks(n)) * 4)))
    return rc;
  CG_HIP(cg::launch_mse(pred, labels, n, static_cast<float*>(workspace), loss, dpred,
                        reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_mse_loss_ema(const float* pred, const float* labels, int64_t n, float* loss, float* dpred,
                    float* ema, float decay, void* workspace, size_t ws_bytes, void* stream) {
  if (!pred || !labels || !loss || !ema || n < 1 || !(decay >= 0.f && decay <= 1.f))
    return fail(CG_ERR_ARG, "mse_loss_ema: bad arguments");
  if (int rc = need_ws("mse_loss_ema", workspace, ws_bytes, al256(size_t(cg::mse_chunks(n)) * 4)))
    return rc;
  CG_HIP(cg::launch_mse(pred, labels, n, static_cast<float*>(workspace), loss, dpred,
                        reinterpret_cast<hipStream_t>(stream), ema, decay));
  return ok();
}

int cg_dropout_forward(const float* x, int64_t n, float keep_prob, uint64_t seed, float* y,
                       void* stream) {
  if (!x || !y || n < 1 || !(keep_prob > 0.f && keep_prob <= 1.f))
    return fail(CG_ERR_ARG, "dropout_forward: bad arguments (keep_prob=%g)", keep_prob);
  CG_HIP(cg::launch_dropout(x, y, n, keep_prob, seed, 0, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_dropout_backward(const float* dy, int64_t n, float keep_prob, uint64_t seed, float* dx,
                        void* stream) {
  if (!dy || !dx || n < 1 || !(keep_prob > 0.f && keep_prob <= 1.f))
    return fail(CG_ERR_ARG, "dropout_backward: bad arguments (keep_prob=%g)", keep_prob);
  CG_HIP(cg::launch_dropout(dy, dx, n, keep_prob, seed, 1, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_clip_by_norm(float* t, int64_t n, float clip_norm, int32_t* nonfinite, void* stream) {
  if (!t || n < 1 || !(clip_norm > 0.f))
    return fail(CG_ERR_ARG, "clip_by_norm: bad arguments (n=%lld, clip_norm=%g)", (long long)n,
                clip_norm);
  CG_HIP(cg::launch_clip_norm(t, n, clip_norm, nonfinite, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_seq_xent_workspace_bytes(int32_t T, int32_t N, int32_t M, int32_t H, size_t* out) {
  if (!out || T < 1 || N < 1 || M < 1 || H < 1 || int64_t(T) * N > INT32_MAX)
    return fail(CG_ERR_ARG, "seq_xent_workspace_bytes: bad arguments");
  if (H > 256) return fail(CG_ERR_UNSUPPORTED, "seq_xent: H = %d, the head supports H <= 256", H);
  *out = al256(cg::seq_xent_ws_bytes(int64_t(T) * N, M, H));
  return ok();
}

int cg_seq_xent_head(const float* hs, const float* w, const float* b, const int32_t* labels,
                     int32_t T, int32_t N, int32_t M, int32_t H, float keep, uint64_t seed,
                     float loss_scale, float* logits, float* ce, float* loss, float* dhs, float* dw,
                     float* db, void* ws, size_t ws_bytes, void* stream) {
  if (!hs || !w || !b || !labels || !loss || (dhs && (!dw || !db)))
    return fail(CG_ERR_ARG, "seq_xent_head: null pointer");
  if (T < 1 || N < 1 || M < 1 || H < 1 || int64_t(T) * N > INT32_MAX)
    return fail(CG_ERR_ARG, "seq_xent_head: bad sizes (T=%d N=%d M=%d H=%d)", T, N, M, H);
  if (!(keep > 0.f && keep <= 1.f))
    return fail(CG_ERR_ARG, "seq_xent_head: keep = %g outside (0, 1]", keep);
  if (H > 256) return fail(CG_ERR_UNSUPPORTED, "seq_xent: H = %d, the head supports H <= 256", H);
  const size_t need = al256(cg::seq_xent_ws_bytes(int64_t(T) * N, M, H));
  if (int rc = need_ws("seq_xent_head", ws, ws_bytes, need)) return rc;
  CG_HIP(cg::launch_seq_xent(hs, w, b, labels, T, N, M, H, keep, seed, loss_scale, logits, ce, loss,
                             dhs, dw, db, static_cast<float*>(ws),
                             reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_class_xent_workspace_bytes(int32_t N, int32_t C, int64_t reg_n, size_t* bytes) {
  if (!bytes || N < 1 || C < 1 || reg_n < 0)
    return fail(CG_ERR_ARG, "class_xent_workspace_bytes: bad arguments");
  if (int rc = cg::below_2_31("class_xent: logits", N, C)) return rc;
  *bytes = al256(cg::class_xent_ws_bytes(N, reg_n));
  return ok();
}

int cg_class_xent_ema(const float* logits, const int32_t* labels, int32_t N, int32_t C,
                      const float* params, int64_t reg_begin, int64_t reg_n, float reg_scale,
                      float* loss, float* dlogits, float* ema, float decay, int32_t* pred,
                      int32_t* correct, int32_t* status, void* workspace, size_t ws_bytes,
                      void* stream) {
  if (!logits || !labels || !loss) return fail(CG_ERR_ARG, "class_xent_ema: null pointer");
  if (N < 1 || C < 1) return fail(CG_ERR_ARG, "class_xent_ema: bad sizes (N=%d C=%d)", N, C);
  if (int rc = cg::below_2_31("class_xent_ema: logits", N, C)) return rc;
  if (reg_begin < 0 || reg_n < 0 || (reg_n > 0 && !params))
    return fail(CG_ERR_ARG, "class_xent_ema: bad regularised range [%lld, +%lld)",
                (long long)reg_begin, (long long)reg_n);
  if (ema && !(decay >= 0.f && decay <= 1.f))
    return fail(CG_ERR_ARG, "class_xent_ema: decay = %g outside [0, 1]", decay);
  if (int rc = cg::no_alias("class_xent_ema: dlogits", {dlogits}, {logits})) return rc;
  if (int rc = need_ws("class_xent_ema", workspace, ws_bytes, al256(cg::class_xent_ws_bytes(N, reg_n))))
    return rc;
  CG_HIP(cg::launch_class_xent(logits, labels, N, C, reg_n > 0 ? params + reg_begin : nullptr, reg_n,
                               reg_scale, float(1.0 / double(N)), loss, dlogits, ema, decay, pred,
                               correct, status, static_cast<float*>(workspace),
                               reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_class_xent_sum(const float* logits, const int32_t* labels, int32_t N, int32_t C,
                      float loss_scale, float* loss, float* dlogits, float* ce, int32_t* pred,
                      int32_t* correct, int32_t* status, void* workspace, size_t ws_bytes,
                      void* stream) {
  if (!logits || !labels || !loss) return fail(CG_ERR_ARG, "class_xent_sum: null pointer");
  if (N < 1 || C < 1) return fail(CG_ERR_ARG, "class_xent_sum: bad sizes (N=%d C=%d)", N, C);
  if (int rc = cg::below_2_31("class_xent_sum: logits", N, C)) return rc;
  if (int rc = cg::no_alias("class_xent_sum: dlogits", {dlogits}, {logits})) return rc;
  if (int rc = need_ws("class_xent_sum", workspace, ws_bytes, al256(cg::class_xent_ws_bytes(N, 0))))
    return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  CG_HIP(cg::launch_class_xent(logits, labels, N, C, nullptr, 0, 0.f, loss_scale, loss, dlogits,
                               nullptr, 0.f, pred, correct, status, ws, s));
  if (ce)  // the rows' ce are the workspace's first N floats
    CG_HIP(hipMemcpyAsync(ce, ws, size_t(N) * sizeof(float), hipMemcpyDeviceToDevice, s));
  return ok();
}

int cg_slice_channels(const float* x, int64_t rows, int32_t C, int32_t c0, int32_t c1, float* out,
                      void* stream) {
  if (!x || !out || rows < 1 || C < 1 || c0 < 0 || c1 <= c0 || c1 > C)
    return fail(CG_ERR_ARG, "slice_channels: bad arguments (C=%d, [%d, %d))", C, c0, c1);
  CG_HIP(cg::launch_slice_channels(x, rows, C, c0, c1, out, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_stack_merge_forward(int32_t N, int32_t M, int32_t F, const float* out_i, const float* w_i,
                           int32_t accumulate, float* y, void* stream) {
  if (N < 1 || M < 1 || F < 1 || !out_i || !w_i || !y)
    return fail(CG_ERR_ARG, "stack_merge_forward: bad arguments");
  if (out_i == y) return fail(CG_ERR_ARG, "stack_merge_forward: y must not alias out_i");
  CG_HIP(cg::launch_stack_merge_fwd(out_i, w_i, N, int64_t(M) * F, accumulate, y,
                                    reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_stack_merge_backward(int32_t N, int32_t M, int32_t F, const float* dy, const float* out_i,
                            const float* w_i, float* dout_i, float* dw_i, void* stream) {
  if (N < 1 || M < 1 || F < 1 || !dy || !out_i || !w_i || (!dout_i && !dw_i))
    return fail(CG_ERR_ARG, "stack_merge_backward: bad arguments");
  if (dout_i && (dout_i == out_i || dout_i == dy))
    return fail(CG_ERR_ARG, "stack_merge_backward: dout_i must not alias dy / out_i");
  CG_HIP(cg::launch_stack_merge_bwd(dy, out_i, w_i, N, int64_t(M) * F, dout_i, dw_i,
                                    reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_weight_grad_workspace_bytes(int64_t R, int32_t FinK, int32_t Fout, size_t* bytes) {
  if (!bytes || R < 1 || FinK < 1 || Fout < 1) return fail(CG_ERR_ARG, "weight_grad: bad arguments");
  *bytes = dw_slab_bytes(R, 0, FinK, Fout);
  return ok();
}

int cg_weight_grad(int64_t R, int32_t FinK, int32_t Fout, const float* basis, const float* dy,
                   float* dW, int32_t accumulate, void* workspace, size_t ws_bytes, void* stream) {
  if (!basis || !dy || !dW || R < 1 || FinK < 1 || Fout < 1)
    return fail(CG_ERR_ARG, "weight_grad: bad arguments");
  if (int rc = need_ws("weight_grad", workspace, ws_bytes, dw_slab_bytes(R, 0, FinK, Fout))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* slabs = static_cast<float*>(workspace);
  CG_HIP(cg::launch_dw_slabs(basis, dy, R, FinK, Fout, slabs, s));
  CG_HIP(cg::launch_reduce_slabs_acc(slabs, cg::dw_chunks(R), int64_t(FinK) * Fout, dW,
                                     accumulate != 0, s));
  return ok();
}

int cg_weight_grad_planes(int64_t R, int32_t Fin, int32_t K, int32_t Fout, const float* planes,
                          int64_t plane_stride, const float* dy, float* dW, int32_t accumulate,
                          void* workspace, size_t ws_bytes, void* stream) {
  if (!planes || !dy || !dW || R < 1 || Fin < 1 || K < 1 || Fout < 1 || plane_stride < R * Fin)
    return fail(CG_ERR_ARG, "weight_grad_planes: bad arguments");
  const int FinK = Fin * K;
  if (int rc = need_ws("weight_grad_planes", workspace, ws_bytes, dw_slab_bytes(R, 0, FinK, Fout)))
    return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* slabs = static_cast<float*>(workspace);
  CG_HIP(cg::launch_dw_slabs(planes, dy, R, FinK, Fout, slabs, s, Fin, plane_stride, K));
  CG_HIP(cg::launch_reduce_slabs_acc(slabs, cg::dw_chunks(R), int64_t(FinK) * Fout, dW,
                                     accumulate != 0, s));
  return ok();
}

int cg_bias_grad_workspace_bytes(int64_t R, int32_t C, size_t* bytes) {
  if (!bytes || R < 1 || C < 1) return fail(CG_ERR_ARG, "bias_grad: bad arguments");
  *bytes = cg::colsum_ws_bytes(R, C);
  return ok();
}

int cg_bias_grad(int64_t R, int32_t C, const float* dy, float* db, int32_t accumulate,
                 void* workspace, size_t ws_bytes, void* stream) {
  if (!dy || !db || R < 1 || C < 1) return fail(CG_ERR_ARG, "bias_grad: bad arguments");
  if (int rc = need_ws("bias_grad", workspace, ws_bytes, cg::colsum_ws_bytes(R, C))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* slabs = static_cast<float*>(workspace);
  CG_HIP(cg::launch_colsum_slabs(dy, R, C, slabs, s));
  CG_HIP(cg::launch_reduce_slabs_acc(slabs, cg::colsum_chunks(R), C, db, accumulate != 0, s));
  return ok();
}

// ---- bias + activation (b1relu / b1tanh / b2relu) and fc GEMM -----------------
int cg_bias_act_forward(int64_t n, int32_t bias_len, const float* x, const float* bias,
                        int32_t act, float* y, void* stream) {
  if (!x || !y || n < 1) return fail(CG_ERR_ARG, "bias_act_forward: bad arguments");
  if (act < CG_ACT_NONE || act > CG_ACT_TANH) return fail(CG_ERR_ARG, "unknown activation %d", act);
  if (bias && (bias_len < 1 || n % bias_len))
    return fail(CG_ERR_ARG, "bias_act_forward: n=%lld is not a multiple of bias_len=%d",
                (long long)n, bias_len);
  CG_HIP(cg::launch_bias_act_fwd(x, bias, bias ? bias_len : 1, act, n, y,
                                 reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_act_forward(int64_t n, float* y, const float* residual, int32_t act, void* stream) {
  if (!y || n < 1) return fail(CG_ERR_ARG, "act_forward: bad arguments");
  if (act < CG_ACT_NONE || act > CG_ACT_TANH) return fail(CG_ERR_ARG, "unknown activation %d", act);
  if (residual == y) return fail(CG_ERR_ARG, "act_forward: residual aliases y");
  CG_HIP(cg::launch_act_fwd(y, residual, act, n, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_bias_act_workspace_bytes(int64_t n, int32_t bias_len, size_t* bytes) {
  if (!bytes || n < 1 || bias_len < 1 || n % bias_len)
    return fail(CG_ERR_ARG, "bias_act_workspace_bytes: bad arguments");
  *bytes = cg::colsum_ws_bytes(n / bias_len, bias_len);
  return ok();
}

int cg_bias_act_backward(int64_t n, int32_t bias_len, const float* dy, const float* y, int32_t act,
                         float* dz, float* db, int32_t accumulate, void* workspace,
                         size_t ws_bytes, void* stream) {
  if (!dy || !dz || n < 1) return fail(CG_ERR_ARG, "bias_act_backward: bad arguments");
  if (act < CG_ACT_NONE || act > CG_ACT_TANH) return fail(CG_ERR_ARG, "unknown activation %d", act);
  if (act != CG_ACT_NONE && !y) return fail(CG_ERR_ARG, "bias_act_backward: activation needs y");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  CG_HIP(cg::launch_bias_act_bwd(dy, y, act, n, dz, s));
  if (!db) return ok();
  if (bias_len < 1 || n % bias_len)
    return fail(CG_ERR_ARG, "bias_act_backward: n=%lld is not a multiple of bias_len=%d",
                (long long)n, bias_len);
  const int64_t R = n / bias_len;
  if (int rc = need_ws("bias_act", workspace, ws_bytes, cg::colsum_ws_bytes(R, bias_len))) return rc;
  float* slabs = static_cast<float*>(workspace);
  CG_HIP(cg::launch_colsum_slabs(dz, R, bias_len, slabs, s));
  CG_HIP(cg::launch_reduce_slabs_acc(slabs, cg::colsum_chunks(R), bias_len, db, accumulate != 0, s));
  return ok();
}

int cg_gemm_f32(int32_t trans_a, int32_t trans_b, int32_t M, int32_t N, int32_t K, const float* A,
                int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc, void* stream) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1) return fail(CG_ERR_ARG, "gemm_f32: bad arguments");
  if (lda < (trans_a ? M : K) || ldb < (trans_b ? K : N) || ldc < N)
    return fail(CG_ERR_ARG, "gemm_f32: leading dimension too small (lda=%d ldb=%d ldc=%d)", lda, ldb,
                ldc);
  if ((M + 63) / 64 > 2147483647 / 2 || (N + 63) / 64 > 65535)
    return fail(CG_ERR_ARG, "gemm_f32: N=%d too large for the grid", N);
  CG_HIP(cg::launch_gemm_f32(trans_a != 0, trans_b != 0, M, N, K, A, lda, B, ldb, C, ldc, 1,
                             reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_perm_gather(const float* x, const int32_t* perm, int32_t N, int32_t M_in, int32_t M_out,
                   int32_t F, float* out, void* stream) {
  if (!x || !perm || !out || N < 1 || M_in < 1 || M_out < 1 || F < 1)
    return fail(CG_ERR_ARG, "perm_gather: bad arguments");
  CG_HIP(cg::launch_perm_gather(x, perm, N, M_in, M_out, F, out,
                                reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_batch_gather(const float* data, const float* labels, const int32_t* idx, int32_t N, int64_t S,
                    int64_t row, int64_t lrow, float* x, float* y, void* stream) {
  if (!data || !idx || !x) return fail(CG_ERR_ARG, "batch_gather: null data / idx / x");
  if (N < 1 || S < 1 || row < 1)
    return fail(CG_ERR_ARG, "batch_gather: bad sizes (N=%d S=%lld row=%lld)", N, (long long)S,
                (long long)row);
  if (!labels != !y)
    return fail(CG_ERR_ARG, "batch_gather: labels and y go together (both or neither)");
  if (labels && lrow < 1) return fail(CG_ERR_ARG, "batch_gather: lrow = %lld", (long long)lrow);
  if (int rc = cg::below_2_31("batch_gather: x", N, row)) return rc;
  if (labels)
    if (int rc = cg::below_2_31("batch_gather: y", N, lrow)) return rc;
  if (int rc = cg::no_alias("batch_gather: x / y", {x, y}, {data, labels})) return rc;
  if (int rc = cg::all_distinct("batch_gather: x / y", {x, y})) return rc;
  CG_HIP(cg::launch_batch_gather(data, labels, idx, N, S, row, lrow, x, y,
                                 reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_maxpool_forward(const float* x, int32_t N, int32_t M, int32_t F, int32_t p, float* y,
                       int32_t* argmax, void* stream) {
  if (!x || !y || N < 1 || M < 1 || F < 1 || p < 1 || M % p)
    return fail(CG_ERR_ARG, "maxpool_forward: bad arguments (M=%d p=%d)", M, p);
  CG_HIP(cg::launch_maxpool_fwd(x, N, M, F, p, y, argmax, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_maxpool_backward(const float* dy, const int32_t* argmax, int32_t N, int32_t M, int32_t F,
                        int32_t p, float* dx, void* stream) {
  if (!dy || !argmax || !dx || N < 1 || M < 1 || F < 1 || p < 1 || M % p)
    return fail(CG_ERR_ARG, "maxpool_backward: bad arguments (M=%d p=%d)", M, p);
  CG_HIP(cg::launch_maxpool_bwd(dy, argmax, N, M, F, p, dx, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_avgpool_forward(const float* x, int32_t N, int32_t M, int32_t F, int32_t p, float* y,
                       void* stream) {
  if (!x || !y || N < 1 || M < 1 || F < 1 || p < 1 || M % p)
    return fail(CG_ERR_ARG, "avgpool_forward: bad arguments (M=%d p=%d)", M, p);
  CG_HIP(cg::launch_avgpool_fwd(x, N, M, F, p, y, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_avgpool_backward(const float* dy, int32_t N, int32_t M, int32_t F, int32_t p, float* dx,
                        void* stream) {
  if (!dy || !dx || N < 1 || M < 1 || F < 1 || p < 1 || M % p)
    return fail(CG_ERR_ARG, "avgpool_backward: bad arguments (M=%d p=%d)", M, p);
  CG_HIP(cg::launch_avgpool_bwd(dy, N, M, F, p, dx, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_adam_update(float* param, const float* grad, float* m, float* v, int64_t n, float lr,
                   float beta1, float beta2, float eps, int32_t step, float grad_scale,
                   void* stream) {
  if (!param || !grad || !m || !v || n < 0 || step < 1)
    return fail(CG_ERR_ARG, "adam_update: bad arguments");
  if (n == 0) return ok();
  CG_HIP(cg::launch_adam(param, grad, m, v, n, cg::adam_lr_t(lr, beta1, beta2, step), beta1, beta2, eps,
                         grad_scale,
                         reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_sgd_update(float* param, const float* grad, int64_t n, float lr, float grad_scale,
                  void* stream) {
  if (!param || !grad || n < 0) return fail(CG_ERR_ARG, "sgd_update: bad arguments");
  if (n == 0) return ok();
  CG_HIP(cg::launch_sgd(param, grad, n, lr, grad_scale, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_momentum_update(float* param, const float* grad, float* accum, int64_t n, float lr,
                       float momentum, float grad_scale, float reg, int64_t reg_begin,
                       int64_t reg_n, void* stream) {
  if (!param || !grad || n < 0 || !(momentum >= 0.f) || (momentum != 0.f && !accum))
    return fail(CG_ERR_ARG, "momentum_update: bad arguments (momentum=%g)", momentum);
  if (reg_begin < 0 || reg_n < 0 || reg_begin > n || reg_n > n - reg_begin)
    return fail(CG_ERR_ARG, "momentum_update: regularised range [%lld, +%lld) outside [0, %lld)",
                (long long)reg_begin, (long long)reg_n, (long long)n);
  if (int rc = cg::all_distinct("momentum_update: param / grad / accum", {param, grad, accum}))
    return rc;
  if (n == 0) return ok();
  CG_HIP(cg::launch_momentum(param, grad, accum, n, lr, momentum, grad_scale, reg, reg_begin, reg_n,
                             reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_rmsprop_update(float* param, const float* grad, float* ms, float* mom, int64_t n, float lr,
                      float rho, float momentum, float eps, float grad_scale, void* stream) {
  if (!param || !grad || !ms || !mom || n < 0 || !(eps > 0.f))
    return fail(CG_ERR_ARG, "rmsprop_update: bad arguments");
  if (n == 0) return ok();
  CG_HIP(cg::launch_rmsprop(param, grad, ms, mom, n, lr, rho, momentum, eps, grad_scale,
                            reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

}  // extern "C"
