// The plan behind the cg_plan_* / cg_cheb_* / cg_lstm_* entries, shared by
// cheb_abi.cpp (which creates and frees it) and lstm_abi.cpp.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/cheb_mi355.h"
#include "cg_internal.h"

struct cg_plan {
  int device = 0;
  int M = 0;
  int64_t nnz = 0, nnzT = 0;
  int max_row_nnz = 0, max_row_nnzT = 0;
  int path = CG_PATH_AUTO;
  int variant = CG_VARIANT_AUTO;
  int* rowptr = nullptr;
  int* col = nullptr;
  float* val = nullptr;
  int* trowptr = nullptr;
  int* tcol = nullptr;
  float* tval = nullptr;
  // degree-sorted row orders of L~ / L~^T (longest rows first), used by the
  // streaming steps on skewed (power-law) graphs so a wave's rows have similar
  // lengths; null when the row lengths are near-uniform
  int* rperm = nullptr;
  int* trperm = nullptr;
  // rows of L~ / L~^T by decreasing length, always present: the LDS-resident
  // kernels deal rows to lanes in this order so a wave's rows have (nearly)
  // equal lengths and its unrolled gather loop has no idle entries
  int* lorder = nullptr;
  int* tlorder = nullptr;
  // thread-slot images of L~ and L~^T for the resident kernels (M <= 2048)
  struct Slots {
    int* buf = nullptr;  // one allocation: row | len | beg | col | val | wlen
    cg::SlotLayout view{};
  } slots, tslots;
  // images of L~ and L~^T for the fast resident kernels (cheb_fast.hip)
  struct Fast {
    void* buf = nullptr;
    cg::FastImage view{};
    bool ok = false;  // max row length <= cg::kFastWidth and M <= 1024
    long gather_cycles = 0, gather_ideal = 0;  // modelled LDS cycles per step
  } fast, tfast;
  // the gconv-LSTM sequence launches' sticky fault word: host-mapped pinned
  // memory the kernel writes (system scope) when a pair hand-off times out,
  // read by cg_lstm_seq_fault without a device copy once seq_event (recorded
  // behind every sequence launch) has completed
  int* seq_fault = nullptr;      // host pointer
  int* seq_fault_dev = nullptr;  // its device alias
  hipEvent_t seq_event = nullptr;
  bool seq_launched = false;
  // test hook (cg_plan_set_seq_fault_test): >= 0 makes workgroup 0 of pair 0
  // of this plan's sequence launches stop publishing its step counter from
  // that step on; -1 (default) off
  int seq_fault_test = -1;
};

namespace cg {

inline int check_device(const cg_plan* p) {
  int d = -1;
  CG_HIP(hipGetDevice(&d));
  if (d != p->device)
    return cg::fail(CG_ERR_ARG, "current HIP device %d differs from the plan's device %d", d,
                p->device);
  return CG_OK;
}

}  // namespace cg
