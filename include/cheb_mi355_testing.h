/* Test hooks of libcheb_mi355 -- NOT part of the integration surface
 * (include/cheb_mi355.h is).  They exist so the library's own tests can
 * provoke failure paths that a healthy GPU never takes and ask which kernels
 * a shape is dispatched to; a caller of the drop-in path never needs them.  Same ABI conventions as cheb_mi355.h.
 */
#ifndef CHEB_MI355_TESTING_H
#define CHEB_MI355_TESTING_H

#include "cheb_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Failure-detection test hook of the one-launch gconv-LSTM layer forward
 * (cg_lstm_seq_forward[_x]): from time step `step` on, workgroup 0 of pair 0
 * of this plan's sequence launches stops publishing its step counter, so its
 * partner times out exactly as when it is not co-resident: the launch poisons
 * the outputs it owed with NaN and sets the plan's fault word
 * (cg_lstm_seq_fault).  -1 (the default) is off.  Plan-scoped; nothing else
 * reads it.  Used by tests/test_gpu_lstm.py::test_seq_handoff_timeout_raises_and_poisons. */
int cg_plan_set_seq_fault_test(cg_plan* plan, int32_t step);

/* Which kernels the streaming forward and backward WOULD launch for a shape
 * (host only: no launch, no device access), so a test can assert that a case
 * reaches the dispatch class it was written for.  A read-out of the route the
 * forward and the backward themselves act on.  CG_ERR_UNSUPPORTED when the forward or the
 * backward of the shape is not on the streaming path, or `layout` (CG_BASIS_*)
 * does not apply.  out[CG_SD_*]; a field that does not apply is 0
 * (CG_SD_LAST_STAGED: -1). */
enum {
  CG_SD_WIDE = 0,         /* 1: wide-column layout (cheb_wide.hip), both ways */
  CG_SD_G = 1,            /* wide: column groups */
  CG_SD_CB = 2,           /* wide: columns per group */
  CG_SD_PL = 3,           /* wide: floats per lane (1, 2, 4) */
  CG_SD_FUSED_LAST = 4,   /* wide: k_wide_last (last step fused with the assembly) */
  CG_SD_ASSEMBLE_TM = 5,  /* wide: rows per tile of k_wide_assemble (0: not launched) */
  CG_SD_DYPASS = 6,       /* wide backward: 0 row-GEMM planes, 1 k_wide_dypass_small, 2 k_wide_dypass */
  CG_SD_SORTED_FWD = 7,   /* the forward steps visit rows in degree-sorted order */
  CG_SD_SORTED_BWD = 8,   /* the backward steps do (order of L~^T) */
  CG_SD_GROUP_FWD = 9,    /* 1: channel-group forward (cheb_group.hip) instead of steps */
  CG_SD_GROUP_BWD = 10,   /* channel-group backward: 0 no, 1 from dBasis planes, 2 dBasis in-kernel */
  CG_SD_VEC = 11,         /* sample-major steps: floats per lane (1, 4) */
  CG_SD_LPR = 12,         /* sample-major steps: lanes per row */
  CG_SD_RPW = 13,         /* sample-major steps: rows per wave */
  CG_SD_XCD_MAP = 14,     /* sample-major steps: 1 sample-per-XCD block mapping */
  CG_SD_LAST_STAGED = 15, /* rows-layout last step: 1 k_cheb_last (LDS staged), 0
                             k_cheb_step<., true>, -1 no assembling step */
  CG_SD_COUNT = 16
};
int cg_plan_query_stream_dispatch(const cg_plan* plan, int32_t N, int32_t Fin, int32_t K,
                                  int32_t Fout, int layout, int32_t out[16]);

#ifdef __cplusplus
}
#endif

#endif /* CHEB_MI355_TESTING_H */
