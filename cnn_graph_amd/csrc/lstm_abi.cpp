// C ABI of the gconv-LSTM family (see include/cheb_mi355.h): cg_lstm_* and the
// sequence launches' fault hook cg_plan_set_seq_fault_test -- argument validation
// and the launches.
#include "../../include/cheb_mi355.h"
#include "../../include/cheb_mi355_testing.h"

#include <hip/hip_runtime.h>

#include "abi_checks.h"
#include "abi_plan.h"
#include "cg_internal.h"

using cg::al16;
using cg::al256;
using cg::check_device;
using cg::dw_slab_bytes;
using cg::fail;
using cg::need_ws;
using cg::ok;

extern "C" {

static size_t lstm_wgrad_rows(int32_t H, int32_t Fin, int32_t K) {
  return size_t(H + Fin) * size_t(K) + 1;
}

int cg_lstm_weight_grads_workspace_bytes(int64_t R, int32_t H, int32_t Fin, int32_t K,
                                         size_t* bytes) {
  if (!bytes || R < 1 || H < 1 || Fin < 1 || K < 1)
    return fail(CG_ERR_ARG, "lstm_weight_grads: bad arguments");
  const size_t rows = lstm_wgrad_rows(H, Fin, K);
  *bytes = dw_slab_bytes(R, 0, int(rows), 4 * H) + al256(rows * size_t(4 * H) * 4);
  return ok();
}

int cg_lstm_weight_grads(int64_t R, int32_t H, int32_t Fin, int32_t K, const float* h_planes,
                         int64_t h_plane_stride, const float* x_planes, int64_t x_plane_stride,
                         const float* dpre, float* dWh, float* dWx, float* db, void* workspace,
                         size_t ws_bytes, void* stream) {
  if (!h_planes || !x_planes || !dpre || !dWh || !dWx || !db || R < 1 || H < 1 || Fin < 1 ||
      K < 1 || h_plane_stride < R * H || x_plane_stride < R * Fin)
    return fail(CG_ERR_ARG, "lstm_weight_grads: bad arguments");
  if (4 * H > 256 || Fin * K + 1 > 64)
    return fail(CG_ERR_UNSUPPORTED, "lstm_weight_grads: needs 4H <= 256, Fin*K < 64 (H=%d Fin=%d K=%d)",
                H, Fin, K);
  size_t need = 0;
  int rc = cg_lstm_weight_grads_workspace_bytes(R, H, Fin, K, &need);
  if (rc) return rc;
  if ((rc = need_ws("lstm_weight_grads", workspace, ws_bytes, need))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int rows = int(lstm_wgrad_rows(H, Fin, K)), C = 4 * H;
  float* slabs = static_cast<float*>(workspace);
  CG_HIP(cg::launch_dw_slabs(h_planes, dpre, R, H * K, C, slabs, s, H, h_plane_stride, K, x_planes,
                             Fin, x_plane_stride));
  // the fixed-order slab sums straight into dWh | dWx | db (one launch, no copies)
  CG_HIP(cg::launch_reduce_slabs3(slabs, cg::dw_chunks(R), int64_t(rows) * C, dWh,
                                  int64_t(H) * K * C, dWx, int64_t(H + Fin) * K * C, db, s));
  return ok();
}

static int check_lstm(int64_t R, int32_t H, int32_t gates) {
  if (R < 1 || H < 1) return fail(CG_ERR_ARG, "lstm: bad shape R=%lld H=%d", (long long)R, H);
  if (R * int64_t(H) * 4 >= (int64_t(1) << 31))
    return fail(CG_ERR_ARG, "lstm: R*4H = %lld exceeds 2^31", (long long)(R * H * 4));
  if (gates != CG_LSTM_GATES_REFERENCE && gates != CG_LSTM_GATES_STANDARD)
    return fail(CG_ERR_ARG, "lstm: unknown gate set %d", gates);
  return CG_OK;
}

int cg_lstm_cell_forward(int64_t R, int32_t H, int32_t gates, const float* gx, const float* gh,
                         const float* bias, const float* c, float* c_out, float* h_out, float* act,
                         void* stream) {
  int rc = check_lstm(R, H, gates);
  if (rc) return rc;
  if (!gx || !c_out || !h_out) return fail(CG_ERR_ARG, "lstm_cell_forward: null gx/c_out/h_out");
  CG_HIP(cg::launch_lstm_fwd(gates, R, H, gx, gh, bias, c, c_out, h_out, act,
                             reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_lstm_cell_backward(int64_t R, int32_t H, int32_t gates, const float* dh,
                          const float* dh_rec, const float* dc,
                          const float* act, const float* c, const float* c_out, float* dpre,
                          float* dc_prev, void* stream) {
  int rc = check_lstm(R, H, gates);
  if (rc) return rc;
  if (!act || !c_out || !dpre) return fail(CG_ERR_ARG, "lstm_cell_backward: null act/c_out/dpre");
  CG_HIP(cg::launch_lstm_bwd(gates, R, H, dh, dh_rec, dc, act, c, c_out, dpre, dc_prev,
                             reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_lstm_hconv_supported(const cg_plan* plan, int32_t H, int32_t K, int32_t* supported) {
  if (!plan || !supported) return fail(CG_ERR_ARG, "lstm_hconv_supported: null argument");
  *supported = cg::lstm_hstep_ok(plan->M, H, K) ? 1 : 0;
  return ok();
}

int cg_lstm_hconv_step(cg_plan* plan, int32_t N, int32_t H, int32_t K, int32_t gates,
                       const float* h_prev, const float* c_prev, const float* gx, const float* Wh,
                       const float* bias, float* c_out, float* h_out, float* act, float* planes,
                       int64_t plane_stride, void* stream) {
  int rc = check_lstm(int64_t(N) * (plan ? plan->M : 1), H, gates);
  if (rc) return rc;
  if (!plan || N < 1 || K < 1) return fail(CG_ERR_ARG, "lstm_hconv_step: bad plan / N / K");
  if (!h_prev || !gx || !Wh || !c_out || !h_out)
    return fail(CG_ERR_ARG, "lstm_hconv_step: null h_prev / gx / Wh / c_out / h_out");
  if (!cg::lstm_hstep_ok(plan->M, H, K))
    return fail(CG_ERR_UNSUPPORTED, "lstm_hconv_step: needs H = 32, M <= 1024 and the LDS for K "
                                    "(M=%d H=%d K=%d)", plan->M, H, K);
  if (planes && K > 1 && plane_stride < int64_t(N) * plan->M * H)
    return fail(CG_ERR_ARG, "lstm_hconv_step: plane stride %lld < N*M*H", (long long)plane_stride);
  // the kernel moves h_prev and the planes as float4
  if (!al16(h_prev) || (planes && !al16(planes)) || (planes && K > 1 && (plane_stride & 3)))
    return fail(CG_ERR_ARG, "lstm_hconv_step: h_prev / planes must be 16-byte aligned and the "
                            "plane stride a multiple of 4 floats");
  if ((rc = cg::no_alias("lstm_hconv_step: outputs", {c_out, h_out, act, planes}, {h_prev, c_prev, gx})))
    return rc;
  if ((rc = check_device(plan))) return rc;
  CG_HIP(cg::launch_lstm_hstep(gates, N, plan->M, K, plan->rowptr, plan->col, plan->val, h_prev,
                               c_prev, gx, Wh, bias, c_out, h_out, act, planes, plane_stride,
                               reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_lstm_seq_supported(const cg_plan* plan, int32_t H, int32_t K, int32_t* supported) {
  if (!plan || !supported) return fail(CG_ERR_ARG, "lstm_seq_supported: null argument");
  *supported =
      (cg::lstm_seq_ok(plan->M, H, K, plan->nnz) && cg::lstm_bstep_ok(plan->M, H, K, plan->nnzT)) ? 1 : 0;
  return ok();
}

int cg_lstm_seq_x_supported(const cg_plan* plan, int32_t Fin, int32_t H, int32_t K, int32_t* supported) {
  if (!plan || !supported) return fail(CG_ERR_ARG, "lstm_seq_x_supported: null argument");
  *supported = (Fin >= 1 && Fin <= 8 && cg::lstm_seq_ok(plan->M, H, K, plan->nnz, Fin) &&
                cg::lstm_bstep_ok(plan->M, H, K, plan->nnzT)) ? 1 : 0;
  return ok();
}

int cg_lstm_seq_workspace_bytes(const cg_plan* plan, int32_t N, size_t* bytes) {
  if (!plan || !bytes || N < 1) return fail(CG_ERR_ARG, "lstm_seq_workspace_bytes: bad arguments");
  *bytes = al256(sizeof(int) * size_t(2) * cg::lstm_seq_pairs(N, plan->device));
  return ok();
}

static int lstm_seq_impl(cg_plan* plan, int32_t T, int32_t N, int32_t H, int32_t K, int32_t gates,
                         const float* gx, const float* xs, const float* Wx, int32_t Fin,
                         float* xplanes, int64_t xplane_stride, const float* Wh, const float* bias,
                         const float* h0, const float* c0, float* hs, float* cs, float* act,
                         float* planes, int64_t plane_stride, void* workspace, size_t ws_bytes,
                         void* stream) {
  int rc = check_lstm(int64_t(T) * N * (plan ? plan->M : 1), H, gates);
  if (rc) return rc;
  if (!plan || T < 1 || N < 1 || K < 1) return fail(CG_ERR_ARG, "lstm_seq_forward: bad plan / T / N / K");
  if ((!gx && !xs) || !Wh || !hs || !cs) return fail(CG_ERR_ARG, "lstm_seq_forward: null gx|xs / Wh / hs / cs");
  if (xs && (Fin < 1 || Fin > 8 || !Wx || !xplanes))
    return fail(CG_ERR_ARG, "lstm_seq_forward_x: needs 1 <= feat_in <= 8, Wx and the x planes");
  if (!cg::lstm_seq_ok(plan->M, H, K, plan->nnz, xs ? Fin : 0))
    return fail(CG_ERR_UNSUPPORTED, "lstm_seq_forward: needs H = 32, M <= 1024 and L~ plus the "
                                    "weights in LDS (M=%d nnz=%lld H=%d K=%d)",
                plan->M, (long long)plan->nnz, H, K);
  const int64_t R = int64_t(T) * N * plan->M;
  if (!planes && K > 1)
    return fail(CG_ERR_ARG, "lstm_seq_forward: planes are required for K > 1 (the pair hands "
                            "its quarters' Chebyshev orders to the partner through them)");
  if (planes && K > 1 && plane_stride < R * H)
    return fail(CG_ERR_ARG, "lstm_seq_forward: plane stride %lld < T*N*M*H", (long long)plane_stride);
  if (xs && xplane_stride < R * Fin)
    return fail(CG_ERR_ARG, "lstm_seq_forward_x: x plane stride %lld < T*N*M*feat_in",
                (long long)xplane_stride);
  if ((gx && !al16(gx)) || !al16(hs) || !al16(cs) || (act && !al16(act)) || (planes && !al16(planes)) ||
      (h0 && !al16(h0)) || (c0 && !al16(c0)) || (bias && !al16(bias)) ||
      (planes && K > 1 && (plane_stride & 3)))
    return fail(CG_ERR_ARG, "lstm_seq_forward: tensors must be 16-byte aligned (float4 access), "
                            "plane stride a multiple of 4");
  if ((rc = cg::no_alias("lstm_seq_forward: outputs", {hs, cs, act, planes, xplanes},
                         {gx, xs, Wx, Wh, bias, h0, c0})))
    return rc;
  size_t need = 0;
  if ((rc = cg_lstm_seq_workspace_bytes(plan, N, &need))) return rc;
  if ((rc = need_ws("lstm_seq_forward", workspace, ws_bytes, need))) return rc;
  if ((rc = check_device(plan))) return rc;
  const int P = cg::lstm_seq_pairs(N, plan->device);
  int* flags = static_cast<int*>(workspace);
  if (!plan->seq_fault) {
    void* hp = nullptr;
    CG_HIP(hipHostMalloc(&hp, 64, hipHostMallocMapped | hipHostMallocCoherent));
    plan->seq_fault = static_cast<int*>(hp);
    *plan->seq_fault = 0;
    void* dp = nullptr;
    CG_HIP(hipHostGetDevicePointer(&dp, hp, 0));
    plan->seq_fault_dev = static_cast<int*>(dp);
    CG_HIP(hipEventCreateWithFlags(&plan->seq_event, hipEventDisableTiming));
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  CG_HIP(cg::launch_lstm_seq(gates, T, N, plan->M, K, plan->nnz, plan->rowptr, plan->col, plan->val,
                             plan->lorder, xs, Wx, Fin, xplanes, xplane_stride, gx, Wh, bias, h0,
                             c0, hs, cs, act, planes, plane_stride, flags, plan->seq_fault_dev, P, s,
                             plan->seq_fault_test, plan->max_row_nnz));
  CG_HIP(hipEventRecord(plan->seq_event, s));
  plan->seq_launched = true;
  return ok();
}

int cg_lstm_seq_forward(cg_plan* plan, int32_t T, int32_t N, int32_t H, int32_t K, int32_t gates,
                        const float* gx, const float* Wh, const float* bias, const float* h0,
                        const float* c0, float* hs, float* cs, float* act, float* planes,
                        int64_t plane_stride, void* workspace, size_t ws_bytes, void* stream) {
  return lstm_seq_impl(plan, T, N, H, K, gates, gx, nullptr, nullptr, 0, nullptr, 0, Wh, bias, h0,
                       c0, hs, cs, act, planes, plane_stride, workspace, ws_bytes, stream);
}

int cg_lstm_seq_forward_x(cg_plan* plan, int32_t T, int32_t N, int32_t Fin, int32_t H, int32_t K,
                          int32_t gates, const float* xs, const float* Wx, float* xplanes,
                          int64_t xplane_stride, const float* Wh, const float* bias,
                          const float* h0, const float* c0, float* hs, float* cs, float* act,
                          float* planes, int64_t plane_stride, void* workspace, size_t ws_bytes,
                          void* stream) {
  if (!xs) return fail(CG_ERR_ARG, "lstm_seq_forward_x: null xs");
  return lstm_seq_impl(plan, T, N, H, K, gates, nullptr, xs, Wx, Fin, xplanes, xplane_stride, Wh,
                       bias, h0, c0, hs, cs, act, planes, plane_stride, workspace, ws_bytes, stream);
}

int cg_lstm_seq_fault(cg_plan* plan, int32_t wait, int32_t clear, int32_t* fault) {
  if (!plan || !fault) return fail(CG_ERR_ARG, "lstm_seq_fault: null argument");
  *fault = 0;
  if (!plan->seq_launched) return ok();
  if (wait) {
    CG_HIP(hipEventSynchronize(plan->seq_event));
  } else {
    const hipError_t q = hipEventQuery(plan->seq_event);
    if (q == hipErrorNotReady) {
      *fault = -1;  // the last sequence launch is still in flight
      return ok();
    }
    if (q != hipSuccess) return fail(CG_ERR_HIP, "lstm_seq_fault: %s", hipGetErrorString(q));
  }
  const int v = __atomic_load_n(plan->seq_fault, __ATOMIC_ACQUIRE);
  if (!v) return ok();
  *fault = 1;
  if (clear) __atomic_store_n(plan->seq_fault, 0, __ATOMIC_RELEASE);
  return fail(CG_ERR_HIP, "lstm_seq_forward: a workgroup pair hand-off timed out (a partner "
                          "workgroup was not co-resident); the launch's hs / cs / act hold NaN "
                          "from the lost step on");
}

int cg_lstm_seq_status(const cg_plan* plan, int32_t N, const void* workspace, int32_t* status,
                       void* stream) {
  if (!plan || !status || N < 1) return fail(CG_ERR_ARG, "lstm_seq_status: bad arguments");
  (void)workspace;  // the fault word lives in the plan (sticky), not in the workspace
  CG_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  return cg_lstm_seq_fault(const_cast<cg_plan*>(plan), 1, 0, status);
}

int cg_plan_set_seq_fault_test(cg_plan* plan, int32_t step) {
  if (!plan || step < -1) return fail(CG_ERR_ARG, "plan_set_seq_fault_test: bad arguments");
  plan->seq_fault_test = step;
  return ok();
}

int cg_lstm_bwd_step(cg_plan* plan, int32_t N, int32_t H, int32_t K, int32_t gates, const float* dh,
                     const float* dh_rec, const float* dc, const float* act,
                     int32_t act_unit_major, const float* c_prev, const float* c_out,
                     const float* Wh, float* dpre, float* dc_prev, float* dh_prev, void* stream) {
  int rc = check_lstm(int64_t(N) * (plan ? plan->M : 1), H, gates);
  if (rc) return rc;
  if (!plan || N < 1 || K < 1) return fail(CG_ERR_ARG, "lstm_bwd_step: bad plan / N / K");
  if (!act || !c_out || !Wh || !dpre)
    return fail(CG_ERR_ARG, "lstm_bwd_step: null act / c_out / Wh / dpre");
  if (!cg::lstm_bstep_ok(plan->M, H, K, plan->nnzT))
    return fail(CG_ERR_UNSUPPORTED, "lstm_bwd_step: needs H = 32, M <= 1024, K <= 4 (M=%d H=%d K=%d)",
                plan->M, H, K);
  const void* all[] = {dh, dh_rec, dc, act, c_prev, c_out, dpre, dc_prev, dh_prev};
  for (const void* p : all)
    if (p && !al16(p)) return fail(CG_ERR_ARG, "lstm_bwd_step: tensors must be 16-byte aligned");
  if ((rc = cg::no_alias("lstm_bwd_step: outputs", {dpre, dc_prev, dh_prev},
                         {dh, dh_rec, dc, act, c_prev, c_out, Wh})))
    return rc;
  if ((rc = check_device(plan))) return rc;
  if (!dh_prev) {  // no h-conv at this step (a zero-state layer's step 0): the pointwise part
    CG_HIP(cg::launch_lstm_bwd(gates, int64_t(N) * plan->M, H, dh, dh_rec, dc, act, c_prev, c_out,
                               dpre, dc_prev, reinterpret_cast<hipStream_t>(stream),
                               act_unit_major));
    return ok();
  }
  CG_HIP(cg::launch_lstm_bstep(gates, N, plan->M, K, plan->trowptr, plan->tcol, plan->tval,
                               plan->tlorder, plan->nnzT, dh, dh_rec,
                               dc, act, act_unit_major, c_prev, c_out, Wh, dpre, dc_prev, dh_prev,
                               reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

}  // extern "C"
