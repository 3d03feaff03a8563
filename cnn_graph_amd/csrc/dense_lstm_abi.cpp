// C ABI of the dense LSTM baseline (see include/cheb_mi355.h): cg_dlstm_* --
// argument validation and the two launches.
#include "../../include/cheb_mi355.h"

#include <hip/hip_runtime.h>

#include "abi_checks.h"
#include "cg_internal.h"

using cg::al16;
using cg::fail;
using cg::need_ws;
using cg::ok;

extern "C" {

static int dlstm_unsupported(const char* who, int32_t H) {
  return fail(CG_ERR_UNSUPPORTED, "%s: H = %d, needs H %% 16 == 0 and 16 <= H <= 128", who, H);
}

// sizes, then H; the [T][N][4H] tensors are indexed in 64 bits
static int dlstm_shape(const char* who, int32_t T, int32_t N, int32_t H) {
  if (T < 1 || N < 1 || H < 1) return fail(CG_ERR_ARG, "%s: bad sizes (T=%d N=%d H=%d)", who, T, N, H);
  return cg::dlstm_ok(H) ? CG_OK : dlstm_unsupported(who, H);
}

// a zero-byte workspace needs no buffer; anything else goes through need_ws
static int dlstm_ws(const char* who, const void* ws, size_t have, size_t need) {
  return need == 0 ? CG_OK : need_ws(who, ws, have, need);
}

int cg_dlstm_supported(int32_t H, int32_t* supported) {
  if (!supported) return fail(CG_ERR_ARG, "dlstm_supported: null argument");
  *supported = cg::dlstm_ok(H) ? 1 : 0;
  return ok();
}

int cg_dlstm_workspace_bytes(int32_t T, int32_t N, int32_t H, size_t* fwd_bytes, size_t* bwd_bytes) {
  if (!fwd_bytes || !bwd_bytes) return fail(CG_ERR_ARG, "dlstm_workspace_bytes: null argument");
  if (int rc = dlstm_shape("dlstm_workspace_bytes", T, N, H)) return rc;
  *fwd_bytes = *bwd_bytes = 0;  // rows are independent: nothing is handed between workgroups
  return ok();
}

int cg_dlstm_seq_forward(int32_t T, int32_t N, int32_t H, const float* gx, const float* Wh,
                         const float* bias, float forget_bias, float* hs, float* cs, float* act,
                         void* workspace, size_t ws_bytes, void* stream) {
  if (!gx || !Wh || !bias || !hs || !cs) return fail(CG_ERR_ARG, "dlstm_seq_forward: null pointer");
  if (int rc = dlstm_shape("dlstm_seq_forward", T, N, H)) return rc;
  if (!al16(gx) || !al16(hs) || !al16(cs) || !al16(act))
    return fail(CG_ERR_ARG, "dlstm_seq_forward: gx, hs, cs and act must be 16-byte aligned");
  if (int rc = cg::no_alias("dlstm_seq_forward: hs, cs, act", {hs, cs, act}, {gx, Wh, bias})) return rc;
  if (int rc = cg::all_distinct("dlstm_seq_forward: hs, cs, act", {hs, cs, act})) return rc;
  if (int rc = dlstm_ws("dlstm_seq_forward", workspace, ws_bytes, 0)) return rc;
  CG_HIP(cg::launch_dlstm_fwd(T, N, H, gx, Wh, bias, forget_bias, hs, cs, act,
                              reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

int cg_dlstm_seq_backward(int32_t T, int32_t N, int32_t H, const float* dhs, const float* act,
                          const float* cs, const float* Wh, float forget_bias, float* dpre,
                          void* workspace, size_t ws_bytes, void* stream) {
  (void)forget_bias;  // act holds sigmoid(a_f + forget_bias) already
  if (!dhs || !act || !cs || !Wh || !dpre) return fail(CG_ERR_ARG, "dlstm_seq_backward: null pointer");
  if (int rc = dlstm_shape("dlstm_seq_backward", T, N, H)) return rc;
  if (!al16(dhs) || !al16(act) || !al16(cs) || !al16(dpre))
    return fail(CG_ERR_ARG, "dlstm_seq_backward: dhs, act, cs and dpre must be 16-byte aligned");
  if (int rc = cg::no_alias("dlstm_seq_backward: dpre", {dpre}, {act, dhs, cs, Wh})) return rc;
  if (int rc = dlstm_ws("dlstm_seq_backward", workspace, ws_bytes, 0)) return rc;
  CG_HIP(cg::launch_dlstm_bwd(T, N, H, dhs, act, cs, Wh, dpre, reinterpret_cast<hipStream_t>(stream)));
  return ok();
}

}  // extern "C"
