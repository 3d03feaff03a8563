// C ABI of libcheb_mi355.so (see include/cheb_mi355.h): plan management,
// options, argument validation, workspace layout and kernel-path dispatch of the
// cg_plan_* and cg_cheb_* entries.  (The gconv-LSTM entries are lstm_abi.cpp, the
// training ops train_abi.cpp, the Fourier filter family fourier_abi.cpp.)
#include "../../include/cheb_mi355.h"
#include "../../include/cheb_mi355_testing.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "abi_checks.h"
#include "abi_plan.h"
#include "cg_internal.h"

#ifdef CG_DEBUG
namespace cg {
int g_debug_flags = 0;
int g_debug_params[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
unsigned long long* g_debug_ts = nullptr;
}
#endif

namespace {
thread_local std::string g_err;  // the calling thread's last-error text
}

// fail / ok / al256: declared in cg_internal.h, shared with fourier_abi.cpp
int cg::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int cg::ok() {
  g_err.clear();
  return CG_OK;
}

size_t cg::al256(size_t b) { return (b + 255) & ~size_t(255); }

using cg::al256;
using cg::check_device;
using cg::dw_slab_bytes;
using cg::fail;
using cg::need_ws;
using cg::ok;

namespace {

// Validates a host CSR: rowptr[0] = 0, non-decreasing, rowptr[M] = nnz,
// columns in [0, M) strictly increasing inside each row (canonical order,
// what tf.sparse_reorder produces at lib/graph_conv.py:153).
int check_csr(const char* what, int32_t M, int64_t nnz, const int32_t* rowptr, const int32_t* col,
              const float* val) {
  if (!rowptr || (nnz > 0 && (!col || !val))) return fail(CG_ERR_ARG, "%s: null CSR array", what);
  if (rowptr[0] != 0 || rowptr[M] != nnz)
    return fail(CG_ERR_ARG, "%s: rowptr[0]=%d rowptr[M]=%d nnz=%lld", what, rowptr[0], rowptr[M],
                (long long)nnz);
  for (int32_t r = 0; r < M; ++r) {
    if (rowptr[r + 1] < rowptr[r]) return fail(CG_ERR_ARG, "%s: rowptr decreases at row %d", what, r);
    for (int32_t j = rowptr[r]; j < rowptr[r + 1]; ++j) {
      if (col[j] < 0 || col[j] >= M)
        return fail(CG_ERR_ARG, "%s: column %d out of range at nnz %d", what, col[j], j);
      if (j > rowptr[r] && col[j] <= col[j - 1])
        return fail(CG_ERR_ARG, "%s: columns not strictly increasing in row %d", what, r);
    }
  }
  return CG_OK;
}

// Exact transpose (counting sort by column; rows come out in increasing order,
// so columns of the transpose are sorted).
void transpose_csr(int32_t M, int64_t nnz, const int32_t* rp, const int32_t* ci, const float* v,
                   std::vector<int32_t>& trp, std::vector<int32_t>& tci, std::vector<float>& tv) {
  trp.assign(size_t(M) + 1, 0);
  tci.resize(size_t(nnz));
  tv.resize(size_t(nnz));
  for (int64_t j = 0; j < nnz; ++j) trp[size_t(ci[j]) + 1]++;
  for (int32_t r = 0; r < M; ++r) trp[size_t(r) + 1] += trp[size_t(r)];
  std::vector<int32_t> fill(trp.begin(), trp.end() - 1);
  for (int32_t r = 0; r < M; ++r)
    for (int32_t j = rp[r]; j < rp[r + 1]; ++j) {
      const int32_t dst = fill[size_t(ci[j])]++;
      tci[size_t(dst)] = r;
      tv[size_t(dst)] = v[j];
    }
}

// Thread-slot ELL image of a CSR operand for the resident kernels
// (cg_internal.h::SlotLayout).  Rows are dealt to thread slots in order of
// decreasing length (stable), so the 64 rows of a wave have nearly equal
// length and the kernel can skip whole gather instructions past the wave's
// maximum; the ELL arrays are column-major so each prologue load is one
// coalesced 256-byte wave access.
int build_slots(cg_plan::Slots* out, int32_t M, const int32_t* rp, const int32_t* ci,
                const float* v) {
  constexpr int kT = cg::kResidentThreads, kW = kT / 64;
  const int rpt = (M + kT - 1) / kT;
  if (rpt > 2) return CG_OK;  // resident path not available: no image
  int maxlen = 0;
  for (int32_t r = 0; r < M; ++r) maxlen = std::max(maxlen, rp[r + 1] - rp[r]);
  const int width = cg::resident_slot_width(M, maxlen);
  const int S = rpt * kT;
  std::vector<int32_t> order(static_cast<size_t>(M));
  for (int32_t r = 0; r < M; ++r) order[size_t(r)] = r;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    return (rp[a + 1] - rp[a]) > (rp[b + 1] - rp[b]);
  });
  // slot t = q*kT + tid: deal sorted rows tid-major inside each slot group
  std::vector<int32_t> row(size_t(S), -1), len(size_t(S), 0), beg(size_t(S), 0);
  std::vector<int32_t> col(size_t(width) * S, M), wlen(size_t(rpt) * kW, 0);
  std::vector<float> val(size_t(width) * S, 0.f);
  for (int32_t i = 0; i < M; ++i) {
    const int32_t r = order[size_t(i)];
    const int t = i;  // group q = i / kT, tid = i % kT
    row[size_t(t)] = r;
    len[size_t(t)] = rp[r + 1] - rp[r];
    beg[size_t(t)] = rp[r];
    for (int j = 0; j < std::min(width, len[size_t(t)]); ++j) {
      col[size_t(j) * S + t] = ci[rp[r] + j];
      val[size_t(j) * S + t] = v[rp[r] + j];
    }
    const int w = (t / kT) * kW + (t % kT) / 64;
    wlen[size_t(w)] = std::max(wlen[size_t(w)], len[size_t(t)]);
  }
  const size_t n_int = 3 * size_t(S) + size_t(width) * S + size_t(width) * S + wlen.size();
  int* d = nullptr;
  CG_HIP(hipMalloc(reinterpret_cast<void**>(&d), n_int * 4));
  size_t o = 0;
  auto put = [&](const void* src, size_t count) -> int {
    CG_HIP(hipMemcpy(d + o, src, count * 4, hipMemcpyHostToDevice));
    o += count;
    return CG_OK;
  };
  int rc = put(row.data(), row.size());
  if (!rc) rc = put(len.data(), len.size());
  if (!rc) rc = put(beg.data(), beg.size());
  if (!rc) rc = put(col.data(), col.size());
  if (!rc) rc = put(val.data(), val.size());
  if (!rc) rc = put(wlen.data(), wlen.size());
  if (rc) {
    (void)hipFree(d);
    return rc;
  }
  out->buf = d;
  cg::SlotLayout& e = out->view;
  e.S = S;
  e.width = width;
  e.row = d;
  e.len = d + S;
  e.beg = d + 2 * size_t(S);
  e.col = d + 3 * size_t(S);
  e.val = reinterpret_cast<const float*>(d + 3 * size_t(S) + size_t(width) * S);
  e.wlen = d + 3 * size_t(S) + 2 * size_t(width) * S;
  return CG_OK;
}

// Image of a CSR operand for the fast resident kernels (cg_internal.h::
// FastImage): thread->row assignment and bank-aware record layout from
// lds_layout.cpp, uploaded as one device allocation.
int build_fast_image(cg_plan::Fast* out, int32_t M, const int32_t* rp, const int32_t* ci,
                     const float* v, cg::FastLayout* keep = nullptr, const cg::FastLayout* reuse = nullptr) {
  constexpr int kT = 1024, kWd = cg::kFastWidth;
  if (M > kT) return CG_OK;
  int maxlen = 0;
  for (int32_t r = 0; r < M; ++r) maxlen = std::max(maxlen, rp[r + 1] - rp[r]);
  if (maxlen > kWd) return CG_OK;
  cg::FastLayout lay;
  if (reuse) lay = *reuse;  // the same sparsity pattern: the same layout
  else cg::plan_fast_layout(M, rp, ci, &lay);
  if (keep) *keep = lay;
  std::vector<float> val(size_t(kWd) * kT, 0.f);
  for (int t = 0; t < kT; ++t) {
    const int r = lay.row[size_t(t)];
    if (r < 0) continue;
    for (int j = 0; j < rp[r + 1] - rp[r]; ++j) val[size_t(j) * kT + t] = v[rp[r] + j];
  }
  // gather records packed two per word (record indices < 2^16): the per-thread
  // image the fast kernels load in their prologue is 8 words smaller
  if (lay.P >= 65536) return CG_OK;  // (never for M <= 1024: P ~ 2M + 66)
  std::vector<int> cpos2(size_t(kWd / 2) * kT);
  for (int j2 = 0; j2 < kWd / 2; ++j2)
    for (int t = 0; t < kT; ++t)
      cpos2[size_t(j2) * kT + t] = int(uint32_t(lay.cpos[size_t(2 * j2) * kT + t]) |
                                       (uint32_t(lay.cpos[size_t(2 * j2 + 1) * kT + t]) << 16));
  const std::vector<int>* ints[] = {&lay.row, &lay.rpos0, &lay.rpos1, &lay.rposr, &cpos2,
                                    &lay.wlen, &lay.mpos, &lay.pos0, &lay.pos1};
  size_t bytes = val.size() * 4;
  for (const auto* a : ints) bytes += a->size() * 4;
  char* d = nullptr;
  CG_HIP(hipMalloc(reinterpret_cast<void**>(&d), bytes));
  out->buf = d;
  size_t o = 0;
  bool okc = true;
  auto put = [&](const void* src, size_t count) -> const void* {
    const void* at = d + o;
    if (hipMemcpy(d + o, src, count * 4, hipMemcpyHostToDevice) != hipSuccess) okc = false;
    o += count * 4;
    return at;
  };
  cg::FastImage& e = out->view;
  e.row = static_cast<const int*>(put(lay.row.data(), lay.row.size()));
  e.rpos = static_cast<const int*>(put(lay.rpos0.data(), lay.rpos0.size()));
  e.rpos1 = static_cast<const int*>(put(lay.rpos1.data(), lay.rpos1.size()));
  e.rposr = static_cast<const int*>(put(lay.rposr.data(), lay.rposr.size()));
  e.cpos = static_cast<const int*>(put(cpos2.data(), cpos2.size()));
  e.val = static_cast<const float*>(put(val.data(), val.size()));
  e.wlen = static_cast<const int*>(put(lay.wlen.data(), lay.wlen.size()));
  e.mpos = static_cast<const int*>(put(lay.mpos.data(), lay.mpos.size()));
  e.pos0 = static_cast<const int*>(put(lay.pos0.data(), lay.pos0.size()));
  e.pos1 = static_cast<const int*>(put(lay.pos1.data(), lay.pos1.size()));
  e.zpos = lay.zero_base;
  e.P = lay.P;
  if (!okc) return fail(CG_ERR_HIP, "build_fast_image: hipMemcpy failed");
  out->gather_cycles = lay.gather_cycles;
  out->gather_ideal = lay.gather_ideal;
  out->ok = true;
  return CG_OK;
}

template <typename T>
int upload(T** dst, const T* src, size_t count) {
  *dst = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  CG_HIP(hipMalloc(reinterpret_cast<void**>(dst), bytes));
  if (count) CG_HIP(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice));
  return CG_OK;
}

void free_plan(cg_plan* p) {
  if (!p) return;
  void* ptrs[] = {p->rowptr, p->col, p->val, p->trowptr, p->tcol, p->tval, p->rperm, p->trperm,
                  p->lorder, p->tlorder};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (p->slots.buf) (void)hipFree(p->slots.buf);
  if (p->tslots.buf) (void)hipFree(p->tslots.buf);
  if (p->fast.buf) (void)hipFree(p->fast.buf);
  if (p->tfast.buf) (void)hipFree(p->tfast.buf);
  if (p->seq_event) (void)hipEventDestroy(p->seq_event);
  if (p->seq_fault) (void)hipHostFree(p->seq_fault);
  delete p;
}

int check_shape(const cg_plan* p, int32_t N, int32_t Fin, int32_t K, int32_t Fout) {
  if (!p) return fail(CG_ERR_ARG, "null plan");
  if (N < 1 || Fin < 1 || K < 1 || Fout < 1)
    return fail(CG_ERR_ARG, "bad shape N=%d Fin=%d K=%d Fout=%d", N, Fin, K, Fout);
  if (int64_t(N) * p->M >= (int64_t(1) << 31) || int64_t(N) * Fin >= (int64_t(1) << 31))
    return fail(CG_ERR_ARG, "N*M or N*Fin exceeds 2^31");
  return CG_OK;
}

// CG_VARIANT_CLASSIC runs the classic resident kernels (cheb_resident.hip)
// where the fast ones (cheb_fast.hip) would; CG_VARIANT_UNFUSED_DW keeps the
// fast kernels but computes dW with the separate streaming GEMM.
cg::FastGeom fast_geom(const cg_plan* p, int32_t Fin, int32_t K, int32_t Fout) {
  return cg::fast_geometry(p->M, p->fast.view.P, p->max_row_nnz, p->max_row_nnzT, Fin, K, Fout);
}

bool use_fast(const cg_plan* p, int32_t Fin, int32_t K, int32_t Fout, bool backward) {
  if (p->variant == CG_VARIANT_CLASSIC) return false;
  if (!(backward ? p->tfast.ok : p->fast.ok)) return false;
  const cg::FastGeom g = fast_geom(p, Fin, K, Fout);
  return backward ? g.bwd_ok : g.fwd_ok;
}

bool fused_dw(const cg_plan* p, int32_t Fin, int32_t K, int32_t Fout) {
  return use_fast(p, Fin, K, Fout, true) && fast_geom(p, Fin, K, Fout).dw_fused &&
         p->variant != CG_VARIANT_UNFUSED_DW;
}

int choose_path(const cg_plan* p, int32_t Fin, int32_t K, int32_t Fout, bool backward,
                int* path) {
  const cg::ResidentGeom g = cg::resident_geometry(p->M, int(p->nnz), p->max_row_nnz, p->max_row_nnzT, Fin, K, Fout);
  const bool fits = use_fast(p, Fin, K, Fout, backward) || (backward ? g.bwd_ok : g.fwd_ok);
  if (p->path == CG_PATH_STREAM) {
    *path = CG_PATH_STREAM;
  } else if (p->path == CG_PATH_RESIDENT) {
    if (!fits)
      return fail(CG_ERR_UNSUPPORTED,
                  "resident path does not fit: M=%d nnz=%lld Fin=%d K=%d Fout=%d (lds fwd %zu / "
                  "bwd %zu bytes)",
                  p->M, (long long)p->nnz, Fin, K, Fout, g.fwd_lds, g.bwd_lds);
    *path = CG_PATH_RESIDENT;
  } else {
    *path = fits ? CG_PATH_RESIDENT : CG_PATH_STREAM;
  }
  return CG_OK;
}

// Basis layouts (cheb_mi355.h): CG_BASIS_ROWS [N*M][Fin*K] (lib/graph_conv.py:172)
// on every path; CG_BASIS_ORDERS [N][Fin*K][Mb] (Mb = M rounded up to 32) where
// the fast forward stores it during the recurrence and the fused-dW fast
// backward reads it back.
inline int32_t basis_mb(int32_t M) { return (M + 31) & ~31; }

int check_layout(const cg_plan* p, int32_t Fin, int32_t K, int32_t Fout, int layout) {
  if (layout == CG_BASIS_ROWS) return CG_OK;
  if (layout == CG_BASIS_PLANES) {
    // the sample-major streaming path both ways (Fin >= 16 never takes the
    // wide-column layout), planes whose 16-float chunks the row GEMM loads
    int pf = 0, pb = 0;
    const bool ok = Fin % 16 == 0 && K >= 2 && !choose_path(p, Fin, K, Fout, false, &pf) &&
                    !choose_path(p, Fin, K, Fout, true, &pb) && pf == CG_PATH_STREAM &&
                    pb == CG_PATH_STREAM && cg::rowgemm_ok(Fin * K, Fin * K, Fout);
    if (!ok)
      return fail(CG_ERR_UNSUPPORTED,
                  "planes basis layout needs the sample-major streaming path forward and "
                  "backward, Fin a multiple of 16 and K >= 2 (M=%d Fin=%d K=%d Fout=%d)",
                  p->M, Fin, K, Fout);
    return CG_OK;
  }
  if (layout != CG_BASIS_ORDERS) return fail(CG_ERR_ARG, "unknown basis layout %d", layout);
  // the fast forward without the basis staging (so it also serves shapes whose
  // staged basis would not fit in LDS) and the fused-dW fast backward
  if (Fin > 2 || p->path == CG_PATH_STREAM || p->variant == CG_VARIANT_CLASSIC || !p->fast.ok ||
      !fast_geom(p, Fin, K, Fout).fwd_ok_ob || !fused_dw(p, Fin, K, Fout))
    return fail(CG_ERR_UNSUPPORTED,
                "orders basis layout needs Fin <= 2, the fast resident forward and the "
                "fused-dW fast backward (M=%d Fin=%d K=%d Fout=%d)",
                p->M, Fin, K, Fout);
  return CG_OK;
}

// What a Chebyshev convolution launches and where its buffers lie, decided once
// per call by cheb_route.  The forward, the backward, cg_cheb_workspace_bytes and
// the test hook cg_plan_query_stream_dispatch all read it, so they cannot
// disagree.  A field that does not apply is zero (last_staged: -1).  What depends
// on the call's pointers or the ablation build stays with backward_impl /
// forward_impl: dw_small_aligned(basis, dy), the cg::debug_flags() bits, x != basis.
enum class FwdKind { Fast, Resident, Copy, WideSteps, Group, PlanesSteps, Steps };
enum class BwdKind { Fast, Resident, WideDypass, GroupDy, WidePlanes, GroupPlanes, Clenshaw };
// dBasis = dy W^T of the backwards that read dBasis planes
enum class DaGemm { None, RowAllPlanes, RowPerPlane, Gemm };
// y = act(basis W + res) after the forward recurrence
enum class YGemm { InKernel, RowPlanes, Row, GemmThenAct };

struct ChebRoute {
  int path_fwd, path_bwd;  // CG_PATH_RESIDENT / CG_PATH_STREAM
  FwdKind fwd;             // the forward recurrence
  BwdKind bwd;             // the backward dx pass
  bool wide;               // streaming path in the wide-column layout (cheb_wide.hip)
  bool fused_last;         // WideSteps: k_wide_last (last step fused with the assembly)
  int assemble_tm;         // WideSteps: rows per tile of k_wide_assemble (0: not launched)
  int dypass;              // WideDypass: 1 k_wide_dypass_small, 2 k_wide_dypass
  int last_staged;         // Steps: 1 k_cheb_last (LDS staged), 0 k_cheb_step<., true>
  const int* rperm_fwd;    // row order of the forward / backward steps (NULL: natural,
  const int* rperm_bwd;    // or no stepping kernel)
  DaGemm da_gemm;
  YGemm y_gemm;
  bool dw_fused;  // Fast backward forms the dW slabs (when the call wants dx and dW)
  bool dw_small;  // dW in one block (rows layout, aligned pointers)
  int vec;        // sample-major steps: floats per lane
  cg::StepGeom step;
  cg::WideGeom wg;
  cg::FastGeom fast;
  cg::ResidentGeom res;
  // Workspace.  forward: T_1 .. T_{K-2} (sample-major), the K planes T_0 .. T_{K-1}
  // (wide) or the per-group partial y; the size holds for every layout the shape
  // admits.  backward: [dW slabs][dBasis][wide D planes] (streaming path; G_k
  // overwrites plane k, so no ring).  The forward's workspace is dead once it has
  // returned, so one buffer of max(fwd, bwd) bytes may serve both.
  size_t fwd_bytes, bwd_bytes;
  size_t off_dA, off_D;  // byte offsets inside the backward workspace (the dW slabs: 0)
};

// The only place where the dispatch predicates are combined.  `layout` has
// passed check_layout.  with_bwd = false (the forward) leaves the backward half
// unset, so a forward still runs where only the backward fails to fit a forced
// resident path.
int cheb_route(const cg_plan* p, int32_t N, int32_t Fin, int32_t K, int32_t Fout, int layout,
               bool with_bwd, ChebRoute* out) {
  ChebRoute& r = *out = ChebRoute{};
  r.last_staged = -1;
  int rc;
  if ((rc = choose_path(p, Fin, K, Fout, false, &r.path_fwd))) return rc;
  if (with_bwd && (rc = choose_path(p, Fin, K, Fout, true, &r.path_bwd))) return rc;
  const int M = p->M, FinK = Fin * K;
  const int64_t R = int64_t(N) * M;
  const bool stream_f = r.path_fwd == CG_PATH_STREAM;
  const bool stream_b = with_bwd && r.path_bwd == CG_PATH_STREAM;
  bool group = false;
  if (stream_f || stream_b) {
    // The wide-column layout serves the streaming path when Fin < 8 (sample-major
    // gathers of Fin*4 < 32 bytes) and its column split fits (cheb_wide.hip).
    const cg::WideGeom wg = cg::wide_geometry(N, Fin, M);
    r.wide = p->variant != CG_VARIANT_NARROW && int64_t(Fin) * K <= 256 && wg.ok;
    if (r.wide) {
      r.wg = wg;
    } else {
      r.vec = cg::step_vec(Fin);
      r.step = cg::step_geom(N, M, Fin, r.vec);
      // Channel-group resident kernels (cheb_group.hip) serve the sample-major
      // streaming path for M <= 1024, Fin % 8 == 0 (forward: planes layout only).
      group = p->variant != CG_VARIANT_STEPS && p->variant != CG_VARIANT_NARROW &&
              cg::grp_ok(M, std::max(p->nnz, p->nnzT), Fin, K, Fout);
    }
  }
  const bool fast_f = layout == CG_BASIS_ORDERS ||
                      (r.path_fwd == CG_PATH_RESIDENT && use_fast(p, Fin, K, Fout, false));
  const bool fast_b = with_bwd && r.path_bwd == CG_PATH_RESIDENT && use_fast(p, Fin, K, Fout, true);
  if (fast_f || fast_b) r.fast = fast_geom(p, Fin, K, Fout);
  if ((!fast_f && !stream_f) || (with_bwd && !fast_b && !stream_b))
    r.res = cg::resident_geometry(M, int(p->nnz), p->max_row_nnz, p->max_row_nnzT, Fin, K, Fout);

  if (fast_f) {
    r.fwd = FwdKind::Fast;
  } else if (!stream_f) {
    r.fwd = FwdKind::Resident;
  } else if (K == 1) {
    r.fwd = FwdKind::Copy;
  } else if (r.wide) {
    r.fwd = FwdKind::WideSteps;
    r.rperm_fwd = p->rperm;
    r.fused_last = cg::wide_last_ok(r.wg, Fin, K, p->rperm != nullptr);
    r.assemble_tm = r.fused_last ? 0 : cg::wide_tm(FinK);
  } else if (layout == CG_BASIS_PLANES && group) {
    r.fwd = FwdKind::Group;
  } else {
    r.fwd = layout == CG_BASIS_PLANES ? FwdKind::PlanesSteps : FwdKind::Steps;
    r.rperm_fwd = cg::step_rperm(p->rperm, Fin);
    if (r.fwd == FwdKind::Steps)  // (planes: every step writes its own plane)
      r.last_staged = cg::cheb_last_stage_bytes(r.step, Fin, K) <= size_t(cg::kLdsBytes) ? 1 : 0;
  }
  if (fast_f || !stream_f || r.fwd == FwdKind::Group) r.y_gemm = YGemm::InKernel;
  else if (layout == CG_BASIS_PLANES) r.y_gemm = YGemm::RowPlanes;
  else r.y_gemm = cg::rowgemm_ok(FinK, FinK, Fout) ? YGemm::Row : YGemm::GemmThenAct;
  const size_t plane = size_t(M) * size_t(int64_t(N) * Fin) * 4;
  if (stream_f) {
    r.fwd_bytes = al256(r.wide ? size_t(K) * plane : size_t(K > 2 ? K - 2 : 0) * plane);
    if (group) r.fwd_bytes = std::max(r.fwd_bytes, al256(cg::grp_partial_bytes(N, M, Fin, Fout)));
  }
  if (!with_bwd) return CG_OK;

  if (fast_b) {
    r.bwd = BwdKind::Fast;
    r.dw_fused = fused_dw(p, Fin, K, Fout);
  } else if (!stream_b) {
    r.bwd = BwdKind::Resident;
  } else if (r.wide && cg::wide_dypass_ok(FinK, Fout)) {
    r.bwd = BwdKind::WideDypass;
    r.dypass = cg::wide_dypass_small(FinK) ? 1 : 2;
  } else if (group && cg::grp_clen_dy_ok(M, p->nnzT, K, Fout)) {
    r.bwd = BwdKind::GroupDy;
  } else {
    r.bwd = r.wide ? BwdKind::WidePlanes : group ? BwdKind::GroupPlanes : BwdKind::Clenshaw;
    // all K planes in one pass over dy when the FinK columns fit one row-GEMM block
    r.da_gemm = cg::rowgemm_ok(Fout, Fout, FinK)  ? DaGemm::RowAllPlanes
                : cg::rowgemm_ok(Fout, Fout, Fin) ? DaGemm::RowPerPlane
                                                  : DaGemm::Gemm;
    if (r.bwd == BwdKind::Clenshaw) r.rperm_bwd = cg::step_rperm(p->trperm, Fin);
  }
  if (stream_b && r.wide && K >= 2) r.rperm_bwd = p->trperm;  // (K == 1: no step)
  r.dw_small = cg::dw_small_ok(R, FinK, Fout);
  // the fused dy pass writes the slabs itself, one per block
  r.bwd_bytes = dw_slab_bytes(R, N, FinK, Fout, r.bwd == BwdKind::WideDypass ? M : 0);
  r.off_dA = r.off_D = r.bwd_bytes;
  if (stream_b) {
    // dBasis, N*M*FinK floats (k-major); reported for GroupDy too, which forms it in LDS
    if (r.bwd != BwdKind::WideDypass) r.bwd_bytes += al256(size_t(R) * size_t(FinK) * 4);
    r.off_D = r.bwd_bytes;
    if (r.wide) r.bwd_bytes += al256(size_t(K) * plane);  // the [K][M][B] planes D_k / G_k
  }
  return CG_OK;
}

// The route of a shape whose forward and backward are both on the streaming
// path, read out for the test hook cg_plan_query_stream_dispatch.
// out: CG_SD_* of include/cheb_mi355_testing.h.
void stream_dispatch(const ChebRoute& r, int32_t* out) {
  out[CG_SD_WIDE] = r.wide;
  out[CG_SD_G] = r.wg.G;
  out[CG_SD_CB] = r.wg.CB;
  out[CG_SD_PL] = r.wg.pl;
  out[CG_SD_FUSED_LAST] = r.fused_last;
  out[CG_SD_ASSEMBLE_TM] = r.assemble_tm;
  out[CG_SD_DYPASS] = r.dypass;
  out[CG_SD_SORTED_FWD] = r.rperm_fwd != nullptr;
  out[CG_SD_SORTED_BWD] = r.rperm_bwd != nullptr;
  out[CG_SD_GROUP_FWD] = r.fwd == FwdKind::Group;
  out[CG_SD_GROUP_BWD] = r.bwd == BwdKind::GroupDy ? 2 : r.bwd == BwdKind::GroupPlanes ? 1 : 0;
  out[CG_SD_VEC] = r.vec;
  out[CG_SD_LPR] = r.step.lpr;
  out[CG_SD_RPW] = r.step.rpw;
  out[CG_SD_XCD_MAP] = r.step.xcd_map;
  out[CG_SD_LAST_STAGED] = r.last_staged;
}

}  // namespace

namespace cg {
namespace {
// CG_OPT_* values (defaults: the measured-faster kernels) and their ranges
std::atomic<int> g_opts[kOptCount] = {{1}, {1}, {8}, {1}, {1}, {1}, {1}, {1}, {1}, {1}, {2}};
// The release library accepts only the values a user would choose between;
// the alternatives that lost every A/B exist in the ablation
// build only (`make debug`): CG_OPT_DW_DIRECT 2 / 3 (forced direct dW), CG_OPT_DW_W2
// 0 (one-wave dW builds), CG_OPT_SPMM_PW 0, CG_OPT_GRP_PC 0, CG_OPT_CLEN_DY 0 / 2.
bool option_valid(int o, int v) {
#ifndef CG_DEBUG
  switch (o) {
    case kOptDwDirect: return v == 0 || v == 1;
    case kOptDwW2:
    case kOptSpmmPw:
    case kOptGrpPc:
    case kOptClenDy: return v == 1;
    default: break;
  }
#endif
  switch (o) {
    case kOptDwDirect: return v >= 0 && v <= 3;
    case kOptDwWaves: return v == 4 || v == 8;
    case kOptClenDy: return v >= 0 && v <= 2;
    case kOptSeqXpre: return v >= 0 && v <= 2;
    case kOptMfmaStagger: return v >= 0 && v <= 2;
    default: return v == 0 || v == 1;
  }
}
}  // namespace
int option(Opt o) { return g_opts[o].load(std::memory_order_relaxed); }
}  // namespace cg

extern "C" {

int cg_version(void) { return 301; }


int cg_set_option(int32_t option, int32_t value) {
  if (option < 0 || option >= cg::kOptCount) return fail(CG_ERR_ARG, "unknown option %d", option);
  if (!cg::option_valid(option, value))
    return fail(CG_ERR_ARG, "value %d out of range for option %d", value, option);
  cg::g_opts[option].store(value, std::memory_order_relaxed);
  return ok();
}

int cg_get_option(int32_t option, int32_t* value) {
  if (option < 0 || option >= cg::kOptCount || !value)
    return fail(CG_ERR_ARG, "unknown option %d or null value", option);
  *value = cg::g_opts[option].load(std::memory_order_relaxed);
  return ok();
}

#ifdef CG_DEBUG
// Timing-ablation hook of the debug build only (`make debug`; not in the
// public header, not in the release library; outputs are WRONG when set).
int cg_debug_set_flags(int flags) {
  cg::g_debug_flags = flags;
  return ok();
}
// Tuning override (ablation build only): launch code reads key k < 8 with
// cg::debug_param(k, default); value -1 restores the default.
// Phase timestamps of the fast kernels (ablation build only): a device buffer
// of N * 8 uint64 or NULL.
int cg_debug_set_ts(void* dev_buf) {
  cg::g_debug_ts = static_cast<unsigned long long*>(dev_buf);
  return ok();
}
int cg_debug_set_param(int key, int value) {
  if (key < 0 || key >= 8) return fail(CG_ERR_ARG, "bad debug param %d", key);
  cg::g_debug_params[key] = value;
  return ok();
}
#endif

// Not in the public header: lets comm.cpp report through cg_last_error().
int cg_internal_set_error(int code, const char* msg) {
  if (code == CG_OK) return ok();
  return fail(code, "%s", msg ? msg : "");
}

const char* cg_last_error(void) { return g_err.c_str(); }

// Not in the public header (tests / diagnostics): plan the fast-path LDS layout
// of a host CSR operand without a GPU, check its invariants, and report the
// modelled LDS cycles of one step's gathers (with the layout and conflict-free).
int cg_debug_layout_stats(int32_t M, const int32_t* rowptr, const int32_t* col,
                          long* gather_cycles, long* gather_ideal, int* records) {
  if (M < 1 || M > 1024 || !rowptr || !col) return fail(CG_ERR_ARG, "layout_stats: bad args");
  for (int r = 0; r < M; ++r)
    if (rowptr[r + 1] - rowptr[r] > cg::kFastWidth)
      return fail(CG_ERR_UNSUPPORTED, "layout_stats: row %d longer than %d", r, cg::kFastWidth);
  cg::FastLayout lay;
  cg::plan_fast_layout(M, rowptr, col, &lay);
  std::vector<int> seen(size_t(lay.P), 0);
  for (int v = 0; v < M; ++v) {
    for (int p : {lay.pos0[size_t(v)], lay.pos1[size_t(v)]}) {
      if (p < 64 || p >= lay.P || seen[size_t(p)]++)
        return fail(CG_ERR_ARG, "layout: bad/duplicate record %d of vertex %d", p, v);
    }
  }
  for (int t = 0; t < 1024; ++t) {
    const int r = lay.row[size_t(t)];
    for (int j = 0; j < cg::kFastWidth; ++j) {
      const int p = lay.cpos[size_t(j) * 1024 + t];
      if (r >= 0 && j < rowptr[r + 1] - rowptr[r]) {
        const int c = col[rowptr[r] + j];
        if (p != lay.pos0[size_t(c)] && p != lay.pos1[size_t(c)])
          return fail(CG_ERR_ARG, "layout: thread %d slot %d reads record %d, not vertex %d", t, j, p, c);
      } else if (p >= 32) {
        return fail(CG_ERR_ARG, "layout: padding of thread %d slot %d is not a zero record", t, j);
      }
    }
    if (r >= 0 && (lay.rpos0[size_t(t)] != lay.pos0[size_t(r)] || lay.rpos1[size_t(t)] != lay.pos1[size_t(r)] ||
                   (lay.rposr[size_t(t)] != lay.pos0[size_t(r)] && lay.rposr[size_t(t)] != lay.pos1[size_t(r)])))
      return fail(CG_ERR_ARG, "layout: own records of thread %d", t);
    if (r < 0 && (lay.rpos0[size_t(t)] < 32 || lay.rpos0[size_t(t)] >= 64))
      return fail(CG_ERR_ARG, "layout: idle thread %d does not write a dummy record", t);
  }
  for (int m = 0; m < M; ++m)
    if (lay.mpos[size_t(m)] != lay.pos0[size_t(m)] && lay.mpos[size_t(m)] != lay.pos1[size_t(m)])
      return fail(CG_ERR_ARG, "layout: tile read of vertex %d", m);
  if (gather_cycles) *gather_cycles = lay.gather_cycles;
  if (gather_ideal) *gather_ideal = lay.gather_ideal;
  if (records) *records = lay.P;
  return ok();
}

int cg_plan_create(cg_plan** plan, int device, int32_t M, int64_t nnz, const int32_t* rowptr,
                   const int32_t* col, const float* val, const int32_t* t_rowptr,
                   const int32_t* t_col, const float* t_val) {
  if (!plan) return fail(CG_ERR_ARG, "null plan out-pointer");
  *plan = nullptr;
  if (M < 1 || nnz < 0 || nnz >= (int64_t(1) << 31))
    return fail(CG_ERR_ARG, "bad M=%d nnz=%lld", M, (long long)nnz);
  int rc = check_csr("L", M, nnz, rowptr, col, val);
  if (rc) return rc;
  std::vector<int32_t> trp, tci;
  std::vector<float> tv;
  if (t_rowptr) {
    const int64_t nnzT = t_rowptr[M];
    if (nnzT != nnz) return fail(CG_ERR_ARG, "transpose nnz %lld != nnz %lld", (long long)nnzT,
                                 (long long)nnz);
    if ((rc = check_csr("L^T", M, nnz, t_rowptr, t_col, t_val))) return rc;
    trp.assign(t_rowptr, t_rowptr + M + 1);
    tci.assign(t_col, t_col + nnz);
    tv.assign(t_val, t_val + nnz);
  } else {
    transpose_csr(M, nnz, rowptr, col, val, trp, tci, tv);
  }

  int prev = 0;
  CG_HIP(hipGetDevice(&prev));
  CG_HIP(hipSetDevice(device));
  cg_plan* p = new (std::nothrow) cg_plan();
  if (!p) return fail(CG_ERR_ALLOC, "out of host memory");
  p->device = device;
  p->M = M;
  p->nnz = nnz;
  p->nnzT = nnz;
  for (int32_t r = 0; r < M; ++r) {
    p->max_row_nnz = std::max(p->max_row_nnz, rowptr[r + 1] - rowptr[r]);
    p->max_row_nnzT = std::max(p->max_row_nnzT, trp[size_t(r) + 1] - trp[size_t(r)]);
  }
  rc = upload(&p->rowptr, rowptr, size_t(M) + 1);
  if (!rc) rc = upload(&p->col, col, size_t(nnz));
  if (!rc) rc = upload(&p->val, val, size_t(nnz));
  if (!rc) rc = upload(&p->trowptr, trp.data(), trp.size());
  if (!rc) rc = upload(&p->tcol, tci.data(), tci.size());
  if (!rc) rc = upload(&p->tval, tv.data(), tv.size());
  auto order = [M](const int32_t* rp) {
    std::vector<int32_t> o(size_t(M), 0);
    for (int32_t r = 0; r < M; ++r) o[size_t(r)] = r;
    std::stable_sort(o.begin(), o.end(), [rp](int32_t a, int32_t b) {
      return rp[a + 1] - rp[a] > rp[b + 1] - rp[b];
    });
    return o;
  };
  if (!rc && M > 0) {
    const std::vector<int32_t> o = order(rowptr), ot = order(trp.data());
    rc = upload(&p->lorder, o.data(), o.size());
    if (!rc) rc = upload(&p->tlorder, ot.data(), ot.size());
    if (!rc && nnz > 0 && p->max_row_nnz > 2 * (nnz / M) + 8) {
      rc = upload(&p->rperm, o.data(), o.size());
      if (!rc) rc = upload(&p->trperm, ot.data(), ot.size());
    }
  }
  if (!rc && nnz > 0) rc = build_slots(&p->slots, M, rowptr, col, val);
  if (!rc && nnz > 0) rc = build_slots(&p->tslots, M, trp.data(), tci.data(), tv.data());
  // a symmetric pattern (every Laplacian here) shares one layout between L~
  // and L~^T: the annealing (lds_layout.cpp) runs once
  const bool sym = nnz > 0 && std::equal(rowptr, rowptr + M + 1, trp.begin()) &&
                   std::equal(col, col + nnz, tci.begin());
  cg::FastLayout lay;
  if (!rc && nnz > 0) rc = build_fast_image(&p->fast, M, rowptr, col, val, sym ? &lay : nullptr);
  if (!rc && nnz > 0)
    rc = build_fast_image(&p->tfast, M, trp.data(), tci.data(), tv.data(), nullptr,
                          sym && p->fast.ok ? &lay : nullptr);
  (void)hipSetDevice(prev);
  if (rc) {
    free_plan(p);
    return rc;
  }
  *plan = p;
  return ok();
}

int cg_plan_destroy(cg_plan* plan) {
  free_plan(plan);
  return ok();
}

int cg_plan_set_path(cg_plan* plan, int path) {
  if (!plan) return fail(CG_ERR_ARG, "null plan");
  if (path != CG_PATH_AUTO && path != CG_PATH_RESIDENT && path != CG_PATH_STREAM)
    return fail(CG_ERR_ARG, "bad path %d", path);
  plan->path = path;
  return ok();
}

int cg_plan_set_variant(cg_plan* plan, int variant) {
  if (!plan) return fail(CG_ERR_ARG, "null plan");
  if (variant != CG_VARIANT_AUTO && variant != CG_VARIANT_CLASSIC &&
      variant != CG_VARIANT_UNFUSED_DW && variant != CG_VARIANT_NARROW && variant != CG_VARIANT_STEPS)
    return fail(CG_ERR_ARG, "bad kernel variant %d", variant);
  plan->variant = variant;
  return ok();
}

int cg_plan_query_path(const cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                       int* path) {
  int rc = check_shape(plan, N, Fin, K, Fout);
  if (rc) return rc;
  if (!path) return fail(CG_ERR_ARG, "null path out-pointer");
  if ((rc = choose_path(plan, Fin, K, Fout, false, path))) return rc;
  return ok();
}

int cg_cheb_workspace_bytes(const cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                            size_t* fwd_bytes, size_t* bwd_bytes) {
  int rc = check_shape(plan, N, Fin, K, Fout);
  if (rc) return rc;
  ChebRoute r;
  if ((rc = cheb_route(plan, N, Fin, K, Fout, CG_BASIS_ROWS, true, &r))) return rc;
  if (fwd_bytes) *fwd_bytes = r.fwd_bytes;
  if (bwd_bytes) *bwd_bytes = r.bwd_bytes;
  return ok();
}

}  // extern "C"

namespace {
// Adam applied to W by the forward that consumes it (cg_cheb_forward_adam)
struct FwdAdam {
  const float* grad;
  const float* m;
  const float* v;
  float* W_out;
  float* m_out;
  float* v_out;
  float lr_t, beta1, beta2, eps, grad_scale;
};

// forward with the residual / activation epilogue y = act(basis W + res)
int forward_impl(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout, const float* x,
                 const float* W, const float* res, int act, float* basis, float* y, void* workspace,
                 size_t ws_bytes, void* stream, int layout = CG_BASIS_ROWS,
                 const FwdAdam* fa = nullptr) {
  int rc = check_shape(plan, N, Fin, K, Fout);
  if (rc) return rc;
  if ((rc = check_layout(plan, Fin, K, Fout, layout))) return rc;
  if (!x) return fail(CG_ERR_ARG, "null x");
  if (act < CG_ACT_NONE || act > CG_ACT_TANH) return fail(CG_ERR_ARG, "unknown activation %d", act);
  if (!y && (res || act)) return fail(CG_ERR_ARG, "an epilogue needs y");
  if (y && !W) return fail(CG_ERR_ARG, "null W with non-null y");
  if (!y && !basis) return fail(CG_ERR_ARG, "nothing to compute (basis and y both null)");
  if ((rc = check_device(plan))) return rc;
  ChebRoute r;
  if ((rc = cheb_route(plan, N, Fin, K, Fout, layout, false, &r))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int M = plan->M;
  if (fa && r.fwd != FwdKind::Fast) {
    // other kernels: the same update out of place by k_adam, then the forward on W'
    const size_t nb = size_t(Fin) * K * Fout * sizeof(float);
    CG_HIP(hipMemcpyAsync(fa->W_out, W, nb, hipMemcpyDeviceToDevice, s));
    CG_HIP(hipMemcpyAsync(fa->m_out, fa->m, nb, hipMemcpyDeviceToDevice, s));
    CG_HIP(hipMemcpyAsync(fa->v_out, fa->v, nb, hipMemcpyDeviceToDevice, s));
    CG_HIP(cg::launch_adam(fa->W_out, fa->grad, fa->m_out, fa->v_out, int64_t(Fin) * K * Fout,
                           fa->lr_t, fa->beta1, fa->beta2, fa->eps, fa->grad_scale, s));
    W = fa->W_out;
    fa = nullptr;
  }

  if (r.fwd == FwdKind::Fast) {
    // (M, Fin, K, Fout, dbg, res, act, E, x, W, basis, y, bord)
    cg::FastFwdArgs a{M, Fin, K, Fout, cg::debug_flags() & 0xff, res, act, plan->fast.view, x,
                      y ? W : nullptr, basis, y, layout == CG_BASIS_ORDERS ? basis_mb(M) : 0};
#ifdef CG_DEBUG
    a.ts = cg::g_debug_ts;
#endif
    if (fa) {
      a.W = W;
      a.ad_grad = fa->grad;
      a.ad_m = fa->m;
      a.ad_v = fa->v;
      a.ad_W = fa->W_out;
      a.ad_mo = fa->m_out;
      a.ad_vo = fa->v_out;
      a.ad_lr_t = fa->lr_t;
      a.ad_b1 = fa->beta1;
      a.ad_b2 = fa->beta2;
      a.ad_eps = fa->eps;
      a.ad_scale = fa->grad_scale;
    }
    CG_HIP(cg::launch_fast_forward(r.fast, N, a, s));
    return ok();
  }
  if (r.fwd == FwdKind::Resident) {
    // (M, Fin, K, Fout, Mp, dbg, res, act, E, col, val, x, W, basis, y)
    const cg::ResidentFwdArgs a{M, Fin, K, Fout, cg::lds_vertex_stride(M), cg::debug_flags() & 0xff,
                                res, act, plan->slots.view, plan->col, plan->val, x,
                                y ? W : nullptr, basis, y};
    CG_HIP(cg::launch_resident_forward(r.res, N, a, s));
    return ok();
  }
  // streaming path
  if (!basis) return fail(CG_ERR_ARG, "streaming path needs a basis buffer (the GEMM reads it)");
  if (r.fwd_bytes && (rc = need_ws("forward", workspace, ws_bytes, r.fwd_bytes))) return rc;
  float* slots = static_cast<float*>(workspace);
  const size_t slot = size_t(M) * size_t(N) * size_t(Fin);
  switch (r.fwd) {
    default:  // (Fast, Resident: returned above)
      break;
    case FwdKind::Copy:
      if (x != basis) CG_HIP(hipMemcpyAsync(basis, x, slot * sizeof(float), hipMemcpyDeviceToDevice, s));
      break;
    case FwdKind::WideSteps: {
      // wide columns: T_0 = x re-laid [M][Fin*N] into plane 0, the K-1 steps
      // plane to plane, then the basis (lib/graph_conv.py:155-172)
      const int B = N * Fin;
      CG_HIP(cg::launch_sm_to_vm(x, 1, N, int64_t(M) * Fin, slots, s));
      for (int k = 1; k < (r.fused_last ? K - 1 : K); ++k)
        CG_HIP(cg::launch_wide_step(r.wg, plan->rowptr, plan->col, plan->val, r.rperm_fwd,
                                    slots + size_t(k - 1) * slot,
                                    k >= 2 ? slots + size_t(k - 2) * slot : nullptr, nullptr,
                                    slots + size_t(k) * slot, M, B, k == 1 ? 0 : 1, 2.f, s));
      if (r.fused_last)  // T_{K-1} and the basis assembly in one launch
        CG_HIP(cg::launch_wide_last(r.wg, plan->rowptr, plan->col, plan->val, slots, int64_t(slot),
                                    basis, M, N, K, s));
      else
        CG_HIP(cg::launch_wide_assemble(slots, int64_t(slot), N, M, Fin, K, basis, s));
      break;
    }
    case FwdKind::Group:
      // channel-group resident kernel: the whole recurrence in LDS per (sample,
      // 8 channels), planes written once, y from per-group MFMA partials
      CG_HIP(cg::launch_grp_fwd(plan->rowptr, plan->col, plan->val, plan->lorder, plan->nnz, N, M,
                                Fin, K, Fout, x, W, basis, slots, res, act, y, s));
      break;
    case FwdKind::PlanesSteps: {
      // planes layout: T_k IS plane k of the basis (plane 0 = x: copied unless
      // the caller placed x there), every step writes its own plane, no assembly
      // step (lib/graph_conv.py:159-169)
      auto P = [&](int k) { return basis + size_t(k) * slot; };
      if (x != basis) CG_HIP(hipMemcpyAsync(basis, x, slot * sizeof(float), hipMemcpyDeviceToDevice, s));
      for (int k = 1; k < K; ++k)
        CG_HIP(cg::launch_cheb_step(plan->rowptr, plan->col, plan->val, r.rperm_fwd,
                                    k == 1 ? x : P(k - 1), k == 2 ? x : (k > 2 ? P(k - 2) : nullptr),
                                    P(k), x, nullptr, nullptr, N, M, Fin, K, k, false, s));
      break;
    }
    case FwdKind::Steps: {
      // sample-major steps: T_0 = x, T_j (1 <= j <= K-2) in slots[j-1], the last
      // step writes the whole basis (lib/graph_conv.py:159-172)
      auto T = [&](int k) -> const float* { return k == 0 ? x : slots + size_t(k - 1) * slot; };
      for (int k = 1; k < K; ++k) {
        const bool last = (k == K - 1);
        CG_HIP(cg::launch_cheb_step(plan->rowptr, plan->col, plan->val, r.rperm_fwd, T(k - 1),
                                    k >= 2 ? T(k - 2) : nullptr,
                                    last ? nullptr : slots + size_t(k - 1) * slot, x, slots, basis, N,
                                    M, Fin, K, k, last, s));
      }
      break;
    }
  }
  const int FinK = Fin * K;
  if (!y || r.y_gemm == YGemm::InKernel) return ok();
  if (r.y_gemm == YGemm::RowPlanes) {
    // y = sum_k T_k W_k straight from the planes (row GEMM, A addressed per plane)
    CG_HIP(cg::launch_rowgemm(basis, int64_t(N) * M, FinK, FinK, W, Fout, 1, 0, 1, Fout, y, Fout, 0,
                              s, res, act, 0, Fin, int64_t(slot), K));
  } else if (r.y_gemm == YGemm::Row) {
    CG_HIP(cg::launch_rowgemm(basis, int64_t(N) * M, FinK, FinK, W, Fout, 1, 0, 1, Fout, y, Fout, 0,
                              s, res, act));
  } else {
    CG_HIP(cg::launch_gemm_f32(false, false, N * M, Fout, FinK, basis, FinK, W, Fout, y, Fout, 1, s));
    if (res || act) CG_HIP(cg::launch_act_fwd(y, res, act, int64_t(N) * M * Fout, s));
  }
  return ok();
}

// Wide-column reverse recurrence over the [K][M][Fin*N] planes D: G_k in place
// of D_k, one launch per step (G_{K-1} = D_{K-1}: the last order's step would
// rewrite its plane in place), then G_0 re-laid into dx (dx += when accumulating)
int wide_reverse(const cg_plan* plan, const ChebRoute& r, float* D, int32_t N, int32_t Fin,
                 int32_t K, float* dx, int dx_acc, hipStream_t s) {
  const int M = plan->M, B = N * Fin;
  auto G = [&](int k) { return D + size_t(k) * size_t(M) * size_t(B); };
  for (int k = K - 2; k >= 0; --k)
    CG_HIP(cg::launch_wide_step(r.wg, plan->trowptr, plan->tcol, plan->tval, r.rperm_bwd, G(k + 1),
                                (k + 2 <= K - 1) ? G(k + 2) : nullptr, G(k), G(k), M, B, 2,
                                k >= 1 ? 2.f : 1.f, s));
  CG_HIP(cg::launch_vm_to_sm(G(0), N, int64_t(M) * Fin, dx, dx_acc, s));
  return CG_OK;
}

int backward_impl(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout, const float* dy,
                  const float* basis, const float* W, float* dx, int dx_acc, float* dW,
                  void* workspace, size_t ws_bytes, void* stream,
                  const cg::AdamStep* adam = nullptr, int layout = CG_BASIS_ROWS) {
  int rc = check_shape(plan, N, Fin, K, Fout);
  if (rc) return rc;
  if ((rc = check_layout(plan, Fin, K, Fout, layout))) return rc;
  if (layout == CG_BASIS_ORDERS && dW && !dx)
    return fail(CG_ERR_UNSUPPORTED, "orders basis layout: dW is fused into the dx pass (dx needed)");
  if (!dy || !W) return fail(CG_ERR_ARG, "null dy/W");
  if (!basis && dW) return fail(CG_ERR_ARG, "null basis: dW needs the forward's basis");
  if (!dx && !dW) return fail(CG_ERR_ARG, "dx and dW are both NULL: nothing to compute");
  if ((rc = check_device(plan))) return rc;
  ChebRoute r;
  if ((rc = cheb_route(plan, N, Fin, K, Fout, layout, true, &r))) return rc;
  if ((rc = need_ws("backward", workspace, ws_bytes, r.bwd_bytes))) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int M = plan->M;
  const int FinK = Fin * K;
  const int64_t R = int64_t(N) * M;

  // Everything runs on the caller's stream.  (Forking the streaming dW GEMM onto a side stream to
  // overlap the dx recurrence was measured on MI355X in round 1: the event
  // fork + join costs ~20 us per call, more than the overlap gains there.)
  char* base = static_cast<char*>(workspace);
  float* slabs = reinterpret_cast<float*>(base);
  float* dA = reinterpret_cast<float*>(base + r.off_dA);  // dBasis, k-major [K][N*M][Fin]
  float* D = reinterpret_cast<float*>(base + r.off_D);    // wide: the [K][M][Fin*N] planes D_k / G_k
  const size_t slot = size_t(M) * size_t(N) * size_t(Fin);
  const bool fused = dx != nullptr && dW != nullptr && r.dw_fused;
  int nslab_ready = 0;  // dW slabs a kernel of the dx pass already wrote
  if (dx) {
    // dBasis = dy W^T written k-major ([K][N*M][Fin]): plane k is
    // dA_k[r][fin] = sum_f dy[r][f] W[fin*K+k][f]
    const int NM = N * M;
    if (r.da_gemm == DaGemm::RowAllPlanes)
      CG_HIP(cg::launch_rowgemm(dy, NM, Fout, Fout, W, 1, int64_t(K) * Fout, Fout, 1, FinK, dA, Fin,
                                int64_t(slot), s, nullptr, 0, Fin));
    else if (r.da_gemm == DaGemm::RowPerPlane)
      CG_HIP(cg::launch_rowgemm(dy, NM, Fout, Fout, W, 1, int64_t(K) * Fout, Fout, K, Fin, dA, Fin,
                                int64_t(slot), s));
    else if (r.da_gemm == DaGemm::Gemm)
      CG_HIP(cg::launch_gemm_f32(false, true, NM, FinK, Fout, dy, Fout, W, Fout, dA, FinK, 1, s, K));
    switch (r.bwd) {
      case BwdKind::Fast: {
        // (M, Fin, K, Fout, Mp, dbg, dx_acc, dscratch_bytes, E, dy, basis, W, dx, dw_slab, bord)
        cg::FastBwdArgs a{M, Fin, K, Fout, cg::lds_vertex_stride(M), (cg::debug_flags() >> 8) & 0xff,
                          dx_acc, r.fast.dscratch, plan->tfast.view, dy, basis, W, dx,
                          fused ? slabs : nullptr, layout == CG_BASIS_ORDERS ? basis_mb(M) : 0};
        a.x3 = cg::option(cg::kOptGemmX3) != 0 ? 1 : 0;
        a.stg = cg::option(cg::kOptMfmaStagger);
#ifdef CG_DEBUG
        a.ts = cg::g_debug_ts;
#endif
        CG_HIP(cg::launch_fast_backward(r.fast, N, a, s));
        break;
      }
      case BwdKind::Resident: {
        // (M, Fin, K, Fout, Mp, dbg, dx_acc, E, col, val, dy, W, dx)
        const cg::ResidentBwdArgs a{M, Fin, K, Fout, cg::lds_vertex_stride(M),
                                    (cg::debug_flags() >> 8) & 0xff, dx_acc, plan->tslots.view,
                                    plan->tcol, plan->tval, dy, W, dx};
        CG_HIP(cg::launch_resident_backward(r.res, N, a, s));
        break;
      }
      case BwdKind::WideDypass:
        // wide columns: ONE pass over dy writes the D_k planes straight in the
        // [M][Fin*N] layout and the dW slabs
        CG_HIP(cg::launch_wide_dypass(dy, basis, W, N, M, Fin, K, Fout, D, int64_t(slot),
                                      dW ? slabs : nullptr, s));
        if (dW) nslab_ready = cg::wide_dypass_blocks(N, M);
        if ((rc = wide_reverse(plan, r, D, N, Fin, K, dx, dx_acc, s))) return rc;
        break;
      case BwdKind::WidePlanes:
        // wide columns: the k-planes of dBasis re-laid [M][Fin*N]
        CG_HIP(cg::launch_sm_to_vm(dA, K, N, int64_t(M) * Fin, D, s));
        if ((rc = wide_reverse(plan, r, D, N, Fin, K, dx, dx_acc, s))) return rc;
        break;
      case BwdKind::GroupDy:
        // the whole reverse recurrence in LDS per (sample, 8 channels), dBasis
        // formed in the kernel from dy and W (no dBasis planes)
        CG_HIP(cg::launch_grp_clen_dy(plan->trowptr, plan->tcol, plan->tval, plan->tlorder,
                                      plan->nnzT, N, M, Fin, K, Fout, dy, W, dx, dx_acc, s));
        break;
      case BwdKind::GroupPlanes:
        // the whole reverse recurrence in LDS per (sample, 8 channels)
        CG_HIP(cg::launch_grp_clen(plan->trowptr, plan->tcol, plan->tval, plan->tlorder, plan->nnzT,
                                   N, M, Fin, K, dA, dx, dx_acc, s));
        break;
      case BwdKind::Clenshaw: {
        // the reverse recurrence one launch per step in the sample-major
        // layout.  Step k reads D_k[r] and writes G_k[r] at the same address
        // (same lane), and the steps below k gather G_{k+1} / read G_{k+2} from
        // planes k+1 / k+2, so G lives in place of dBasis: no separate ring (for
        // config D at N = 256 that is 3 x 17.2 GB less workspace).
        auto G = [&](int k) { return dA + size_t(k) * slot; };
        // G_{K-1} = D_{K-1} already sits in its plane: the last order's step
        // would only rewrite it (D's 17 GB at N = 256); with K = 1 the one step
        // is dx = D_0
        for (int k = K >= 2 ? K - 2 : 0; k >= 0; --k)
          CG_HIP(cg::launch_clenshaw(plan->trowptr, plan->tcol, plan->tval, r.rperm_bwd,
                                     (k + 1 <= K - 1) ? G(k + 1) : nullptr,
                                     (k + 2 <= K - 1) ? G(k + 2) : nullptr, k == 0 ? dx : G(k),
                                     G(k), N, M, Fin, K, k, dx_acc, s));
        break;
      }
    }
  }
  if (!dW) return ok();
  if (fused) nslab_ready = N;
  // small problems (config A): dW in one block, no slabs and no reduction
  // launch (with Adam: the one result is the single slab of the fused reduction)
  if (!nslab_ready && layout == CG_BASIS_ROWS && r.dw_small && cg::dw_small_aligned(basis, dy) &&
      !(cg::debug_flags() & (1 << 22))) {
    CG_HIP(cg::launch_dw_small(basis, dy, R, FinK, Fout, adam ? slabs : dW, s));
    if (!adam) return ok();
    nslab_ready = 1;
  }
  if (!nslab_ready && !(cg::debug_flags() & (1 << 22)))  // ablation hook (debug build): skip dW
    CG_HIP(cg::launch_dw_slabs(basis, dy, R, FinK, Fout, slabs, s,
                               layout == CG_BASIS_PLANES ? Fin : 0,
                               layout == CG_BASIS_PLANES ? int64_t(R) * Fin : 0, K));
  const int nslab = nslab_ready ? nslab_ready : cg::dw_chunks(R);
  if (adam)  // reduction + optimizer step in one launch (no exchange in between)
    CG_HIP(cg::launch_reduce_slabs_adam(slabs, nslab, int64_t(FinK) * Fout, dW, *adam, s));
  else if (!(cg::debug_flags() & (1 << 23)))  // ablation hook (debug build): skip the reduction
    CG_HIP(cg::launch_reduce_slabs(slabs, nslab, int64_t(FinK) * Fout, dW, s));
  return ok();
}

}  // namespace

extern "C" {

int cg_cheb_forward(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                    const float* x, const float* W, float* basis, float* y, void* workspace,
                    size_t ws_bytes, void* stream) {
  return forward_impl(plan, N, Fin, K, Fout, x, W, nullptr, CG_ACT_NONE, basis, y, workspace,
                      ws_bytes, stream);
}

int cg_cheb_forward_ex(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                       const float* x, const float* W, const float* residual, int32_t act,
                       float* basis, float* y, void* workspace, size_t ws_bytes, void* stream) {
  return forward_impl(plan, N, Fin, K, Fout, x, W, residual, act, basis, y, workspace, ws_bytes,
                      stream);
}

int cg_cheb_backward(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                     const float* dy, const float* basis, const float* W, float* dx, float* dW,
                     void* workspace, size_t ws_bytes, void* stream) {
  return backward_impl(plan, N, Fin, K, Fout, dy, basis, W, dx, 0, dW, workspace, ws_bytes, stream);
}

namespace {
int backward_adam_impl(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                       int layout, const float* dy, const float* basis, float* W, float* dx,
                       float* dW, float* m, float* v, float lr, float beta1, float beta2,
                       float eps, int32_t step, float grad_scale, void* workspace,
                       size_t ws_bytes, void* stream) {
  if (!dW || !W || !m || !v || step < 1)
    return fail(CG_ERR_ARG, "cheb_backward_adam: dW, W, m, v required and step >= 1");
  // the reduction stores grad[i] and then updates param/m/v[i] in place:
  // any two of them sharing memory would corrupt the update
  if (int rc = cg::all_distinct("cheb_backward_adam: dW, W, m and v", {dW, W, m, v})) return rc;
  if (cg::debug_flags() & ((1 << 22) | (1 << 23)))
    return fail(CG_ERR_UNSUPPORTED, "cheb_backward_adam: dW ablation bits would corrupt W");
  cg::AdamStep a{};
  a.param = W;
  a.m = m;
  a.v = v;
  a.lr_t = cg::adam_lr_t(lr, beta1, beta2, step);
  a.beta1 = beta1;
  a.beta2 = beta2;
  a.eps = eps;
  a.grad_scale = grad_scale;
  return backward_impl(plan, N, Fin, K, Fout, dy, basis, W, dx, 0, dW, workspace, ws_bytes, stream,
                       &a, layout);
}

int backward_ex_impl(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                     const float* dy, const float* y, int32_t act, int layout, const float* basis,
                     const float* W, float* dx, int32_t dx_accumulate, float* dW, float* dz,
                     void* workspace, size_t ws_bytes, void* stream) {
  if (act < CG_ACT_NONE || act > CG_ACT_TANH) return fail(CG_ERR_ARG, "unknown activation %d", act);
  if (!plan || !dy) return fail(CG_ERR_ARG, "null plan / dy");
  int rc = check_shape(plan, N, Fin, K, Fout);
  if (rc) return rc;
  if ((rc = check_layout(plan, Fin, K, Fout, layout))) return rc;
  const float* dy_eff = dy;
  if (act != CG_ACT_NONE) {
    if (!y || !dz)
      return fail(CG_ERR_ARG, "%s backward needs y (its output) and dz",
                  act == CG_ACT_RELU ? "ReLU" : "tanh");
    CG_HIP(cg::launch_act_bwd(dy, y, act, dz, int64_t(N) * plan->M * Fout,
                              reinterpret_cast<hipStream_t>(stream)));
    dy_eff = dz;
  } else if (dz) {
    CG_HIP(hipMemcpyAsync(dz, dy, size_t(N) * plan->M * Fout * sizeof(float),
                          hipMemcpyDeviceToDevice, reinterpret_cast<hipStream_t>(stream)));
  }
  if (!dx && !dW) return ok();
  return backward_impl(plan, N, Fin, K, Fout, dy_eff, basis, W, dx, dx_accumulate != 0, dW,
                       workspace, ws_bytes, stream, nullptr, layout);
}
}  // namespace

int cg_cheb_backward_adam(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                          const float* dy, const float* basis, float* W, float* dx, float* dW,
                          float* m, float* v, float lr, float beta1, float beta2, float eps,
                          int32_t step, float grad_scale, void* workspace, size_t ws_bytes,
                          void* stream) {
  return backward_adam_impl(plan, N, Fin, K, Fout, CG_BASIS_ROWS, dy, basis, W, dx, dW, m, v, lr,
                            beta1, beta2, eps, step, grad_scale, workspace, ws_bytes, stream);
}

int cg_cheb_backward_ex(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                        const float* dy, const float* y, int32_t act, const float* basis,
                        const float* W, float* dx, int32_t dx_accumulate, float* dW, float* dz,
                        void* workspace, size_t ws_bytes, void* stream) {
  return backward_ex_impl(plan, N, Fin, K, Fout, dy, y, act, CG_BASIS_ROWS, basis, W, dx,
                          dx_accumulate, dW, dz, workspace, ws_bytes, stream);
}

int cg_cheb_basis_elems(const cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                        int32_t layout, int64_t* elems) {
  int rc = check_shape(plan, N, Fin, K, Fout);
  if (rc) return rc;
  if (!elems) return fail(CG_ERR_ARG, "null elems out-pointer");
  if ((rc = check_layout(plan, Fin, K, Fout, layout))) return rc;
  const int64_t rows = layout == CG_BASIS_ORDERS ? basis_mb(plan->M) : plan->M;
  *elems = int64_t(N) * rows * Fin * K;
  return ok();
}

int cg_cheb_forward_layout(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                           const float* x, const float* W, const float* residual, int32_t act,
                           int32_t layout, float* basis, float* y, void* workspace,
                           size_t ws_bytes, void* stream) {
  return forward_impl(plan, N, Fin, K, Fout, x, W, residual, act, basis, y, workspace, ws_bytes,
                      stream, layout);
}

int cg_cheb_forward_adam(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                         const float* x, const float* W, const float* grad, const float* m,
                         const float* v, float lr, float beta1, float beta2, float eps,
                         int32_t step, float grad_scale, float* W_out, float* m_out, float* v_out,
                         int32_t layout, float* basis, float* y, void* workspace,
                         size_t ws_bytes, void* stream) {
  if (!W || !grad || !m || !v || !W_out || !m_out || !v_out || step < 1 || !y)
    return fail(CG_ERR_ARG, "cheb_forward_adam: W, grad, m, v, W_out, m_out, v_out, y required "
                            "and step >= 1");
  // every workgroup reads W, m, v while workgroup 0 writes W', m', v': the
  // outputs must not alias any input
  const char* outs = "cheb_forward_adam: W_out, m_out, v_out";
  int rc = cg::no_alias(outs, {W_out, m_out, v_out}, {W, grad, m, v});
  if (!rc) rc = cg::all_distinct(outs, {W_out, m_out, v_out});
  if (rc) return rc;
  FwdAdam fa{grad, m, v, W_out, m_out, v_out, cg::adam_lr_t(lr, beta1, beta2, step),
             beta1, beta2, eps, grad_scale};
  return forward_impl(plan, N, Fin, K, Fout, x, W, nullptr, CG_ACT_NONE, basis, y, workspace,
                      ws_bytes, stream, layout, &fa);
}

int cg_cheb_backward_layout(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                            const float* dy, const float* y, int32_t act, int32_t layout,
                            const float* basis, const float* W, float* dx, int32_t dx_accumulate,
                            float* dW, float* dz, void* workspace, size_t ws_bytes, void* stream) {
  return backward_ex_impl(plan, N, Fin, K, Fout, dy, y, act, layout, basis, W, dx, dx_accumulate,
                          dW, dz, workspace, ws_bytes, stream);
}

int cg_cheb_backward_adam_layout(cg_plan* plan, int32_t N, int32_t Fin, int32_t K, int32_t Fout,
                                 int32_t layout, const float* dy, const float* basis, float* W,
                                 float* dx, float* dW, float* m, float* v, float lr, float beta1,
                                 float beta2, float eps, int32_t step, float grad_scale,
                                 void* workspace, size_t ws_bytes, void* stream) {
  return backward_adam_impl(plan, N, Fin, K, Fout, layout, dy, basis, W, dx, dW, m, v, lr, beta1,
                            beta2, eps, step, grad_scale, workspace, ws_bytes, stream);
}

int cg_plan_query_stream_dispatch(const cg_plan* plan, int32_t N, int32_t Fin, int32_t K,
                                  int32_t Fout, int layout, int32_t out[16]) {
  int rc = check_shape(plan, N, Fin, K, Fout);
  if (rc) return rc;
  if (!out) return fail(CG_ERR_ARG, "null dispatch out-pointer");
  if ((rc = check_layout(plan, Fin, K, Fout, layout))) return rc;
  ChebRoute r;
  if ((rc = cheb_route(plan, N, Fin, K, Fout, layout, true, &r))) return rc;
  if (r.path_fwd != CG_PATH_STREAM || r.path_bwd != CG_PATH_STREAM)
    return fail(CG_ERR_UNSUPPORTED, "not on the streaming path: M=%d Fin=%d K=%d Fout=%d", plan->M,
                Fin, K, Fout);
  stream_dispatch(r, out);
  return ok();
}

}  // extern "C"
