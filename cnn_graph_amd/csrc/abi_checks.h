// Argument checks and workspace sizes shared by the C-ABI files (cheb_abi.cpp,
// fourier_abi.cpp, train_abi.cpp): host code only, no kernel includes this.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/cheb_mi355.h"
#include "cg_internal.h"

namespace cg {

// CG_OK, or the one text every entry uses for a missing / short workspace
inline int need_ws(const char* who, const void* workspace, size_t have, size_t need) {
  if (workspace && have >= need) return CG_OK;
  return fail(CG_ERR_ARG, "%s workspace too small: %zu < %zu", who, have, need);
}

// TF 1.x ApplyAdam's bias-corrected rate: double arithmetic, rounded once.  The
// three Adam paths (k_adam, the fused dW reduction, the forward that applies
// the update) are bitwise equal only while they share this.
inline float adam_lr_t(float lr, float beta1, float beta2, int32_t step) {
  return float(double(lr) * std::sqrt(1.0 - std::pow(double(beta2), step)) /
               (1.0 - std::pow(double(beta1), step)));
}

// No non-null output is an input.  `what` names the entry and its outputs.
inline int no_alias(const char* what, std::initializer_list<const void*> outs,
                    std::initializer_list<const void*> ins) {
  for (const void* o : outs)
    for (const void* i : ins)
      if (o && o == i) return fail(CG_ERR_ARG, "%s must not alias the inputs", what);
  return CG_OK;
}

// No two non-null buffers are the same.  `what` names the entry and the buffers.
inline int all_distinct(const char* what, std::initializer_list<const void*> bufs) {
  for (auto a = bufs.begin(); a != bufs.end(); ++a)
    for (auto b = a + 1; b != bufs.end(); ++b)
      if (*a && *a == *b) return fail(CG_ERR_ARG, "%s must be distinct buffers", what);
  return CG_OK;
}

// A tensor of a * b elements (a, b >= 1) that a kernel indexes in 32 bits:
// a * b < 2^31.  `what` names the entry and the tensor.
inline int below_2_31(const char* what, int64_t a, int64_t b) {
  if (a <= INT32_MAX / b) return CG_OK;
  return fail(CG_ERR_ARG, "%s has %lld x %lld elements, the kernel indexes below 2^31", what,
              (long long)a, (long long)b);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// dW partial slabs: dw_chunks(R) of them from k_dw_slabs, or one per sample
// from the fused backward.
// M > 0: the wide path's fused dy pass writes the slabs (one per block)
inline size_t dw_slab_bytes(int64_t R, int32_t N, int FinK, int Fout, int32_t M = 0) {
  size_t n = std::max<size_t>(size_t(dw_chunks(R)), size_t(N));
  if (M > 0) n = std::max<size_t>(n, size_t(wide_dypass_blocks(N, M)));
  return al256(n * size_t(FinK) * size_t(Fout) * 4);
}

// column-sum partial slabs [colsum_chunks(R)][C]
inline size_t colsum_ws_bytes(int64_t R, int32_t C) {
  return al256(size_t(colsum_chunks(R)) * size_t(C) * 4);
}

}  // namespace cg
