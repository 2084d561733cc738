// cave_hip.hip — the C ABI declared in include/cave_hip.h (host code only).
//
// The kernels live in kernels.h; each shape is instantiated in its own k_*.hip next to its launch
// function.  The argument checks and the parameter blocks are plain host code shared with the emulation
// drivers (cone_entry.h for the cone entries, solver_entry.h and the *_plan functions for the exact
// solvers); every entry here is a plan call followed by a launch.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kernels.h"
#include "apgd.h"
#include "cone_entry.h"
#include "sp_grid.h"
#include "tight_cones.h"
#include "tsp_hk.h"
#include "tsp_hk_wide.h"
#include "vrp_dp.h"
#include "vrp_dp_wide.h"

namespace cave {

// --------------------------------------------------------------- host helpers

static thread_local char g_err[512] = "";

static int32_t fail(int32_t code, const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess) snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  else snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}

// compute units of the current device (queried once per device; 256 on MI355X)
static int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

// Launch the `waves` shape of an LDS-path operator on GRID workgroups, and return from the entry.
#define CAVE_LAUNCH(OP, W1, WAVES, GRID, STREAM, PARAMS, WHAT)                                                 \
  do {                                                                                                         \
    if ((GRID) >= (int64_t)1 << 31) return fail(CAVE_E_INVALID, WHAT ": batch too large (B < 2^31)");          \
    const unsigned grid_ = (unsigned)(GRID);                                                                   \
    hipError_t e_;                                                                                             \
    if ((WAVES) == 1) e_ = W1(grid_, (PARAMS).lds_bytes, (hipStream_t)(STREAM), PARAMS);                       \
    else if ((WAVES) == 8) e_ = launch_##OP##_w8(grid_, (PARAMS).lds_bytes, (hipStream_t)(STREAM), PARAMS);    \
    else if ((WAVES) == 2) e_ = launch_##OP##_w2(grid_, (PARAMS).lds_bytes, (hipStream_t)(STREAM), PARAMS);    \
    else e_ = launch_##OP##_w4(grid_, (PARAMS).lds_bytes, (hipStream_t)(STREAM), PARAMS);                      \
    return e_ == hipSuccess ? CAVE_OK : fail(CAVE_E_LAUNCH, "launch " WHAT, e_);                               \
  } while (0)
// W1: the operator's one-wave launch function; no_one_wave for the sparse pack pass, which has none (its plan refuses waves == 1)
static hipError_t no_one_wave(unsigned, uint32_t, hipStream_t, const SparsePackParams&) { return hipErrorInvalidValue; }

// ... of a large-path operator: GRID persistent workgroups, one workspace slice each
#define CAVE_LAUNCH_LARGE(FN, GRID, STREAM, PARAMS, WORKSPACE, SLICE, WHAT)                                    \
  do {                                                                                                         \
    const LargeWs ws_{(unsigned char*)(WORKSPACE), (uint64_t)(SLICE)};                                         \
    hipError_t e_ = FN((unsigned)(GRID), (PARAMS).lds_bytes, (hipStream_t)(STREAM), PARAMS, ws_);              \
    return e_ == hipSuccess ? CAVE_OK : fail(CAVE_E_LAUNCH, "launch " WHAT, e_);                               \
  } while (0)

// The five fused-step entries (cone_entry.h step_plan): sparse_entry -- the NEXT batch arrives as `next_cones`, else as
// next_ctrs [B_next, m_max, d]; ipm -- the interior-point kernels (mode is CAVE_MODE_INNER_IPM, no cache).
static int32_t step_entry(bool sparse_entry, bool ipm, const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B,
                          int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t flags, const OutPtrs& o,
                          const float* next_ctrs, int64_t B_next, int64_t m_max, int64_t d, const cave_sparse_cones* next_cones,
                          const cave_lite_store* next, int32_t* pack_status, const cave_warm_cache* warm, const int64_t* keys,
                          uint8_t* warm_hit, uint32_t* cu_tickets, void* stream) {
  StepPlan L;
  const int32_t rc = step_plan(sparse_entry, ipm, solve, ids, pred, B, mode, sign, inner_ratio, max_iter, flags, o, next_ctrs, B_next,
                               m_max, d, next_cones, next, pack_status, warm, keys, warm_hit, cu_tickets, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = L.launch != kStepWarm && warm_hit && B > 0 ? hipMemsetAsync(warm_hit, 0, (size_t)B, s) : hipSuccess;
  if (e != hipSuccess) {
    snprintf(L.msg, sizeof(L.msg), "%s: warm_hit", L.who);
    return fail(CAVE_E_LAUNCH, L.msg, e);
  }
  const unsigned grid = (unsigned)L.grid;
  if (L.sparse) {
    e = L.launch == kStepWarm  ? launch_step_sparse_warm(grid, L.X.lds_bytes, s, L.X)
        : L.launch == kStepIpm ? launch_step_sparse_ipm(grid, L.X.lds_bytes, s, L.X)
                               : launch_step_sparse(grid, L.X.lds_bytes, s, L.X);
  } else {
    e = L.launch == kStepWarm  ? launch_step_warm(grid, L.D.lds_bytes, s, L.D)
        : L.launch == kStepIpm ? launch_step_ipm(grid, L.D.lds_bytes, s, L.D)
                               : launch_step(grid, L.D.lds_bytes, s, L.D);
  }
  if (e == hipSuccess) return CAVE_OK;
  snprintf(L.msg, sizeof(L.msg), "launch %s_kernel%s", L.who, L.launch == kStepWarm ? " (warm)" : L.launch == kStepIpm ? " (ipm)" : "");
  return fail(CAVE_E_LAUNCH, L.msg, e);
}

}  // namespace cave

using namespace cave;

extern "C" {

int32_t cave_hip_version(void) { return CAVE_HIP_ABI_VERSION; }

#ifdef CAVE_STAMPS
// diagnostic build only: read and clear the per-phase cycle accumulators
int32_t cave_hip_debug_stamps(unsigned long long* out, int n_inst) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out, HIP_SYMBOL(cave::g_stamp_buf), sizeof(unsigned long long) * 16 * (size_t)n_inst);
  return 0;
}
#endif

const char* cave_hip_last_error(void) { return g_err; }

int32_t cave_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t cave_hip_default_limits(int64_t m_max, int64_t d, int32_t* nnz_cap, int32_t* lds_bytes) {
  if (m_max < 0 || d <= 0) return fail(CAVE_E_INVALID, "default_limits: bad shape");
  default_limits(m_max, d, nnz_cap, lds_bytes);
  return CAVE_OK;
}

int32_t cave_hip_cone_dense(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d, int32_t mode,
                            float sign, float inner_ratio, int32_t max_iter, int32_t nnz_cap, int32_t lds_bytes,
                            int32_t waves, float* proj, float* rnorm, float* target, float* loss, float* grad,
                            int32_t* status, int32_t* iters, void* stream) {
  ConePlan<DenseParams> L;
  const int32_t rc = dense_plan("cone_dense", false, ctrs, pred, B, m_max, d, mode, sign, inner_ratio, max_iter, nnz_cap, lds_bytes, &waves,
                                nullptr, 0, 0, OutPtrs{proj, rnorm, target, loss, grad, status, iters}, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH(dense, launch_dense_w1, waves, L.grid, stream, L.params, "cone_dense_kernel");
}

int32_t cave_hip_pack_count(const float* ctrs, int64_t B, int64_t m_max, int64_t d, int32_t nnz_cap, int32_t lds_bytes,
                            int32_t waves, int32_t* n_rows, int32_t* n_nnz, int32_t* status, void* stream) {
  ConePlan<PackParams> L;
  const int32_t rc = pack_plan("pack_count", kPackCount, ctrs, nullptr, B, m_max, d, nnz_cap, lds_bytes, &waves, nullptr, 0, 0, n_rows, n_nnz,
                               status, nullptr, 0, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH(pack, launch_pack_w1, waves, L.grid, stream, L.params, "cone_pack_kernel(count)");
}

int32_t cave_hip_pack_fill(const float* ctrs, int64_t B, int64_t m_max, int64_t d, int32_t nnz_cap, int32_t lds_bytes,
                           int32_t waves, const cave_cone_store* store, int64_t slot0, int32_t* status, void* stream) {
  ConePlan<PackParams> L;
  const int32_t rc = pack_plan("pack_fill", kPackFill, ctrs, nullptr, B, m_max, d, nnz_cap, lds_bytes, &waves, nullptr, 0, 0, nullptr, nullptr,
                               status, store, slot0, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH(pack, launch_pack_w1, waves, L.grid, stream, L.params, "cone_pack_kernel(fill)");
}

int32_t cave_hip_packed_lds_bytes(int64_t d, int32_t max_rows, int32_t max_nnz, int32_t all_pm1) {
  if (d <= 0 || max_rows < 0 || max_nnz < 0) return CAVE_E_INVALID;
  int32_t s = all_pm1 == 3 ? packed_lds_bytes(d, max_rows, max_nnz, true, false, true)
                           : packed_lds_bytes(d, max_rows, max_nnz, all_pm1 != 0, all_pm1 != 2);
  return s < 0 ? CAVE_E_INVALID : s;
}

int32_t cave_hip_cone_packed(const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B,
                             int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t lds_bytes,
                             int32_t waves, float* proj, float* rnorm, float* target, float* loss, float* grad,
                             int32_t* status, int32_t* iters, void* stream) {
  ConePlan<PackedParams> L;
  const int32_t rc = packed_plan("cone_packed", false, store, ids, pred, B, mode, sign, inner_ratio, max_iter, lds_bytes, &waves, nullptr,
                                 0, 0, OutPtrs{proj, rnorm, target, loss, grad, status, iters}, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH(packed, launch_packed_w1, waves, L.grid, stream, L.params, "cone_packed_kernel");
}

// ------------------------------------------------------------------ large-cone path

int64_t cave_hip_large_slice_bytes(int64_t m_max, int64_t d, int64_t nnz_cap, int64_t band_entries) {
  if (m_max < 0 || d <= 0 || nnz_cap <= 0 || band_entries < 0) return CAVE_E_INVALID;
  return (int64_t)large_slice_bytes(m_max, d, nnz_cap, band_entries);
}

int64_t cave_hip_packed_large_slice_bytes(int64_t d, int64_t max_rows, int64_t band_entries) {
  if (d <= 0 || max_rows < 0 || band_entries < 0) return CAVE_E_INVALID;
  return (int64_t)packed_large_slice_bytes(d, max_rows, band_entries);
}

int32_t cave_hip_packed_large_lds_bytes(int32_t max_rows, int32_t max_bw) {
  if (max_rows < 0 || max_bw < 0) return CAVE_E_INVALID;
  return (int32_t)packed_large_lds_bytes(max_rows, max_bw);
}

int64_t cave_hip_packed_large_rb_bytes(int64_t max_rows) { return (int64_t)rb_cache_bytes(max_rows); }

int32_t cave_hip_cone_dense_large(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d,
                                  int32_t mode, float sign, float inner_ratio, int32_t max_iter, int64_t nnz_cap,
                                  int32_t lds_bytes, void* workspace, int64_t slice_bytes, int32_t n_slots, float* proj,
                                  float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                                  int32_t* iters, void* stream) {
  ConePlan<DenseParams> L;
  const int32_t rc = dense_plan("cone_dense_large", true, ctrs, pred, B, m_max, d, mode, sign, inner_ratio, max_iter, nnz_cap, lds_bytes,
                                nullptr, workspace, slice_bytes, n_slots, OutPtrs{proj, rnorm, target, loss, grad, status, iters}, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH_LARGE(launch_dense_large, L.grid, stream, L.params, workspace, slice_bytes, "cone_dense_large_kernel");
}

int32_t cave_hip_pack_large(const float* ctrs, int64_t B, int64_t m_max, int64_t d, int64_t nnz_cap, void* workspace,
                            int64_t slice_bytes, int32_t n_slots, int32_t* n_rows, int32_t* n_nnz,
                            const cave_cone_store* store, int64_t slot0, int32_t* status, void* stream) {
  ConePlan<PackParams> L;
  const int32_t rc = pack_plan("pack_large", kPackLarge, ctrs, nullptr, B, m_max, d, nnz_cap, 0, nullptr, workspace, slice_bytes, n_slots,
                               n_rows, n_nnz, status, store, slot0, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH_LARGE(launch_pack_large, L.grid, stream, L.params, workspace, slice_bytes, "cone_pack_large_kernel");
}

int32_t cave_hip_cone_packed_large(const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B,
                                   int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t lds_bytes,
                                   int32_t waves, void* workspace, int64_t slice_bytes, int32_t n_slots, float* proj,
                                   float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                                   int32_t* iters, void* stream) {
  ConePlan<PackedParams> L;
  const int32_t rc = packed_plan("cone_packed_large", true, store, ids, pred, B, mode, sign, inner_ratio, max_iter, lds_bytes, &waves,
                                 workspace, slice_bytes, n_slots, OutPtrs{proj, rnorm, target, loss, grad, status, iters}, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  // workgroup shape (waves = 0): 4 waves (two workgroups per CU) unless the batch needs more than two workgroups
  // per CU and four fit the LDS; then 2 waves.
  if (waves == 0) waves = (L.grid > 2 * (int64_t)device_cus() && (int64_t)L.params.lds_bytes * 4 <= (int64_t)kMaxLds) ? 2 : 4;
  if (waves == 1) CAVE_LAUNCH_LARGE(launch_packed_large_w1, L.grid, stream, L.params, workspace, slice_bytes, "cone_packed_large_kernel<1>");
  if (waves == 2) CAVE_LAUNCH_LARGE(launch_packed_large_w2, L.grid, stream, L.params, workspace, slice_bytes, "cone_packed_large_kernel<2>");
  CAVE_LAUNCH_LARGE(launch_packed_large_w4, L.grid, stream, L.params, workspace, slice_bytes, "cone_packed_large_kernel<4>");
}

// ------------------------------------------------------------------ sparse wire format

int32_t cave_hip_pack_count_sparse(const cave_sparse_cones* cones, int32_t nnz_cap, int32_t lds_bytes, int32_t waves,
                                   int32_t* n_rows, int32_t* n_nnz, int32_t* status, void* stream) {
  ConePlan<SparsePackParams> L;
  const int32_t rc = pack_plan("pack_count_sparse", kPackCount, nullptr, cones, 0, 0, 0, nnz_cap, lds_bytes, &waves, nullptr, 0, 0, n_rows,
                               n_nnz, status, nullptr, 0, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH(pack_sparse, no_one_wave, waves, L.grid, stream, L.params, "cone_pack_sparse_kernel(count)");
}

int32_t cave_hip_pack_fill_sparse(const cave_sparse_cones* cones, int32_t nnz_cap, int32_t lds_bytes, int32_t waves,
                                  const cave_cone_store* store, int64_t slot0, int32_t* status, void* stream) {
  ConePlan<SparsePackParams> L;
  const int32_t rc = pack_plan("pack_fill_sparse", kPackFill, nullptr, cones, 0, 0, 0, nnz_cap, lds_bytes, &waves, nullptr, 0, 0, nullptr,
                               nullptr, status, store, slot0, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH(pack_sparse, no_one_wave, waves, L.grid, stream, L.params, "cone_pack_sparse_kernel(fill)");
}

int32_t cave_hip_pack_large_sparse(const cave_sparse_cones* cones, int64_t nnz_cap, void* workspace, int64_t slice_bytes,
                                   int32_t n_slots, int32_t* n_rows, int32_t* n_nnz, const cave_cone_store* store,
                                   int64_t slot0, int32_t* status, void* stream) {
  ConePlan<SparsePackParams> L;
  const int32_t rc = pack_plan("pack_large_sparse", kPackLarge, nullptr, cones, 0, 0, 0, nnz_cap, 0, nullptr, workspace, slice_bytes, n_slots,
                               n_rows, n_nnz, status, store, slot0, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  CAVE_LAUNCH_LARGE(launch_pack_sparse_large, L.grid, stream, L.params, workspace, slice_bytes, "cone_pack_sparse_large_kernel");
}

// ------------------------------------------------------------------ fused step

// (step_limits, the launch limits of a shape: cone_step.h)
int32_t cave_hip_step_lds_bytes(int64_t m_max, int64_t d) {
  int32_t cap = 0, lds = 0;
  const int32_t rc = step_limits(m_max, d, cap, lds);
  return rc == CAVE_OK ? lds : rc;
}

int32_t cave_hip_cone_step(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode, float sign,
                           float inner_ratio, int32_t max_iter, int32_t flags, float* proj, float* rnorm, float* target, float* loss,
                           float* grad, int32_t* status, int32_t* iters, const float* next_ctrs, int64_t B_next,
                           int64_t m_max, int64_t d, const cave_lite_store* next, int32_t* pack_status,
                           uint32_t* cu_tickets, void* stream) {
  return step_entry(false, false, solve, ids, pred, B, mode, sign, inner_ratio, max_iter, flags,
                    OutPtrs{proj, rnorm, target, loss, grad, status, iters}, next_ctrs, B_next, m_max, d, nullptr, next, pack_status,
                    nullptr, nullptr, nullptr, cu_tickets, stream);
}

int32_t cave_hip_cone_step_warm(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode,
                                float sign, float inner_ratio, int32_t max_iter, int32_t flags, float* proj, float* rnorm,
                                float* target, float* loss, float* grad, int32_t* status, int32_t* iters,
                                const float* next_ctrs, int64_t B_next, int64_t m_max, int64_t d, const cave_lite_store* next,
                                int32_t* pack_status, const cave_warm_cache* warm, const int64_t* keys, uint8_t* warm_hit,
                                uint32_t* cu_tickets, void* stream) {
  return step_entry(false, false, solve, ids, pred, B, mode, sign, inner_ratio, max_iter, flags,
                    OutPtrs{proj, rnorm, target, loss, grad, status, iters}, next_ctrs, B_next, m_max, d, nullptr, next, pack_status,
                    warm, keys, warm_hit, cu_tickets, stream);
}

// the fused step with the NEXT batch on the sparse wire format (kernels.h cone_step_sparse_kernel): the solve half and
// its arguments are those of cave_hip_cone_step_warm, the pack half reads `next_cones`
int32_t cave_hip_cone_step_sparse(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode,
                                  float sign, float inner_ratio, int32_t max_iter, int32_t flags, float* proj, float* rnorm,
                                  float* target, float* loss, float* grad, int32_t* status, int32_t* iters,
                                  const cave_sparse_cones* next_cones, const cave_lite_store* next, int32_t* pack_status,
                                  const cave_warm_cache* warm, const int64_t* keys, uint8_t* warm_hit, uint32_t* cu_tickets,
                                  void* stream) {
  return step_entry(true, false, solve, ids, pred, B, mode, sign, inner_ratio, max_iter, flags,
                    OutPtrs{proj, rnorm, target, loss, grad, status, iters}, nullptr, 0, 0, 0, next_cones, next, pack_status, warm, keys,
                    warm_hit, cu_tickets, stream);
}

// ---- the interior-point variant of the fused step (CAVE_MODE_INNER_IPM): kernels of their own (k_step_ipm.hip,
// k_step_sparse_ipm.hip), validated as their siblings; always cold
int32_t cave_hip_cone_step_ipm(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, float sign,
                               int32_t max_iter, int32_t flags, float* proj, float* rnorm, float* target, float* loss,
                               float* grad, int32_t* status, int32_t* iters, const float* next_ctrs, int64_t B_next,
                               int64_t m_max, int64_t d, const cave_lite_store* next, int32_t* pack_status,
                               uint32_t* cu_tickets, void* stream) {
  return step_entry(false, true, solve, ids, pred, B, CAVE_MODE_INNER_IPM, sign, 0.0f, max_iter, flags,
                    OutPtrs{proj, rnorm, target, loss, grad, status, iters}, next_ctrs, B_next, m_max, d, nullptr, next, pack_status,
                    nullptr, nullptr, nullptr, cu_tickets, stream);
}

int32_t cave_hip_cone_step_sparse_ipm(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, float sign,
                                      int32_t max_iter, int32_t flags, float* proj, float* rnorm, float* target, float* loss,
                                      float* grad, int32_t* status, int32_t* iters, const cave_sparse_cones* next_cones,
                                      const cave_lite_store* next, int32_t* pack_status, uint32_t* cu_tickets, void* stream) {
  return step_entry(true, true, solve, ids, pred, B, CAVE_MODE_INNER_IPM, sign, 0.0f, max_iter, flags,
                    OutPtrs{proj, rnorm, target, loss, grad, status, iters}, nullptr, 0, 0, 0, next_cones, next, pack_status, nullptr,
                    nullptr, nullptr, cu_tickets, stream);
}

int32_t cave_hip_lite_from_packed(const cave_cone_store* src, const cave_lite_store* dst, int32_t* status, void* stream) {
  ConePlan<LiteFromPackedParams> L;
  const int32_t rc = lite_from_packed_plan(src, dst, status, &L);
  if (rc != CAVE_OK) return fail(rc, L.msg);
  if (L.grid == 0) return CAVE_OK;
  hipError_t e = launch_lite_from_packed((unsigned)L.grid, L.params.lds_bytes, (hipStream_t)stream, L.params);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch lite_from_packed_kernel", e);
  return CAVE_OK;
}

// ------------------------------------------------------------------ grid shortest path (sp_grid.h)

int32_t cave_hip_sp_grid_lds_bytes(int64_t h, int64_t w) {
  const uint32_t lds = sp_grid_wave_lds_bytes(h, w);
  if (lds == 0u) return fail(CAVE_E_INVALID, "sp_grid_lds_bytes: need h, w >= 1, h*w >= 2 and an instance that fits the LDS");
  return (int32_t)lds;
}

int32_t cave_hip_sp_grid_solve(const float* costs, const float* eval_costs, int64_t N, int64_t h, int64_t w, float* sol,
                               double* obj, double* eval, int32_t* status, uint32_t* key, float* val, void* stream) {
  SpGridParams P;
  int64_t grid;
  int waves;
  char msg[kSolverMsg];
  const int32_t rc = sp_grid_plan(costs, eval_costs, N, h, w, sol, obj, eval, status, key, val, &P, &grid, &waves, msg);
  if (rc != CAVE_OK) return fail(rc, msg);
  if (grid == 0) return CAVE_OK;
  hipError_t e = launch_sp_grid((unsigned)grid, waves, (hipStream_t)stream, P);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch sp_grid_kernel", e);
  return CAVE_OK;
}

// ------------------------------------------------------------------ Held-Karp TSP (tsp_hk.h)

int64_t cave_hip_tsp_hk_slot_bytes(int64_t n) {
  if (!tsp_hk_valid_n(n)) return fail(CAVE_E_INVALID, "tsp_hk_slot_bytes: need 3 <= n <= 14");
  return tsp_hk_slot_bytes(n);
}

int64_t cave_hip_tsp_hk_workspace_bytes(int64_t n, int64_t N) {
  if (!tsp_hk_valid_n(n) || N < 0) return fail(CAVE_E_INVALID, "tsp_hk_workspace_bytes: need 3 <= n <= 14 and N >= 0");
  return solver_workspace_bytes(0, tsp_hk_slot_bytes(n), N, kTspHkDefaultSlots);
}

int32_t cave_hip_tsp_hk_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                              double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  TspHkParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = tsp_hk_plan(costs, eval_costs, N, n, sol, obj, eval, tour, status, workspace, workspace_bytes, &P, &grid, msg);
  if (rc != CAVE_OK) return fail(rc, msg);
  if (grid == 0) return CAVE_OK;
  hipError_t e = launch_tsp_hk((unsigned)grid, (hipStream_t)stream, P);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch tsp_hk kernel", e);
  return CAVE_OK;
}

// ------------------------------------------------------------------ CVRP dynamic program (vrp_dp.h)

int64_t cave_hip_vrp_dp_slot_bytes(int64_t n, int64_t K) {
  if (!vrp_dp_valid(n, K)) return fail(CAVE_E_INVALID, "vrp_dp_slot_bytes: need 3 <= n <= 14 and 1 <= K <= 8");
  return vrp_dp_slot_bytes(n, K);
}

int64_t cave_hip_vrp_dp_workspace_bytes(int64_t n, int64_t K, int64_t N) {
  if (!vrp_dp_valid(n, K) || N < 0) return fail(CAVE_E_INVALID, "vrp_dp_workspace_bytes: need 3 <= n <= 14, 1 <= K <= 8 and N >= 0");
  return solver_workspace_bytes(0, vrp_dp_slot_bytes(n, K), N, kTspHkDefaultSlots);
}

int32_t cave_hip_vrp_dp_solve(const float* costs, const float* eval_costs, const float* demands, double capacity, int64_t K,
                              int64_t N, int64_t n, float* sol, double* obj, double* eval, int32_t* routes, int32_t* status,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  VrpDpParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = vrp_dp_plan(costs, eval_costs, demands, capacity, K, N, n, sol, obj, eval, routes, status, workspace,
                                 workspace_bytes, &P, &grid, msg);
  if (rc != CAVE_OK) return fail(rc, msg);
  if (grid == 0) return CAVE_OK;
  hipError_t e = launch_vrp_dp((unsigned)grid, (hipStream_t)stream, P);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch vrp_dp kernel", e);
  return CAVE_OK;
}

// ------------------------------------------------------------------ Held-Karp TSP, 13 <= n <= 20 (tsp_hk_wide.h)

int64_t cave_hip_tsp_hk_wide_slot_bytes(int64_t n) {
  if (!tsp_hk_wide_valid_n(n)) return fail(CAVE_E_INVALID, "tsp_hk_wide_slot_bytes: need 13 <= n <= 20");
  return tsp_hk_wide_slot_bytes(n);
}

int64_t cave_hip_tsp_hk_wide_workspace_bytes(int64_t n, int64_t N) {
  if (!tsp_hk_wide_valid_n(n) || N < 0) return fail(CAVE_E_INVALID, "tsp_hk_wide_workspace_bytes: need 13 <= n <= 20 and N >= 0");
  return solver_workspace_bytes(tsp_hk_wide_header_bytes(n), tsp_hk_wide_slot_bytes(n), N, tsp_hk_wide_default_slots(n));
}

int32_t cave_hip_tsp_hk_wide_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                                   double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  TspHkParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = tsp_hk_wide_plan(costs, eval_costs, N, n, sol, obj, eval, tour, status, workspace, workspace_bytes, &P, &grid, msg);
  if (rc != CAVE_OK) return fail(rc, msg);
  if (grid == 0) return CAVE_OK;
  hipError_t e = launch_tsp_hk_wide((unsigned)grid, (hipStream_t)stream, P);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch tsp_hk_wide kernels", e);
  return CAVE_OK;
}

// ------------------------------------------------------------------ CVRP dynamic program, 13 <= n <= 20 (vrp_dp_wide.h)

int64_t cave_hip_vrp_dp_wide_slot_bytes(int64_t n, int64_t K) {
  if (!vrp_dp_wide_valid(n, K)) return fail(CAVE_E_INVALID, "vrp_dp_wide_slot_bytes: need 13 <= n <= 20 and 1 <= K <= 8");
  return vrp_dp_wide_slot_bytes(n, K);
}

int64_t cave_hip_vrp_dp_wide_workspace_bytes(int64_t n, int64_t K, int64_t N) {
  if (!vrp_dp_wide_valid(n, K) || N < 0)
    return fail(CAVE_E_INVALID, "vrp_dp_wide_workspace_bytes: need 13 <= n <= 20, 1 <= K <= 8 and N >= 0");
  return solver_workspace_bytes(tsp_hk_wide_header_bytes(n), vrp_dp_wide_slot_bytes(n, K), N, vrp_dp_wide_default_slots(n, K));
}

int32_t cave_hip_vrp_dp_wide_solve(const float* costs, const float* eval_costs, const float* demands, double capacity, int64_t K,
                                   int64_t N, int64_t n, float* sol, double* obj, double* eval, int32_t* routes, int32_t* status,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  VrpDpWideParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = vrp_dp_wide_plan(costs, eval_costs, demands, capacity, K, N, n, sol, obj, eval, routes, status, workspace,
                                      workspace_bytes, &P, &grid, msg);
  if (rc != CAVE_OK) return fail(rc, msg);
  if (grid == 0) return CAVE_OK;
  hipError_t e = launch_vrp_dp_wide((unsigned)grid, (hipStream_t)stream, P);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch vrp_dp_wide kernels", e);
  return CAVE_OK;
}

// ------------------------------------------------------------------ tight cones of any binary LP (tight_cones.h)

static int32_t tight_cones_entry(bool fill, const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off,
                                 const float* sol, int64_t N, double tol, int32_t* n_rows, int64_t* n_ent, const int64_t* ent_off,
                                 int64_t ent_cap, uint32_t* key, float* val, int32_t* status, void* stream) {
  TightConesParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = tight_cones_plan(fill, sys, lazy, lazy_off, sol, N, tol, n_rows, n_ent, ent_off, ent_cap, key, val, status, &P,
                                      &grid, msg);
  if (rc != CAVE_OK) return fail(rc, msg);
  if (grid == 0) return CAVE_OK;
  hipError_t e = launch_tight_cones(fill, (unsigned)grid, (hipStream_t)stream, P);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch tight_cones_kernel", e);
  return CAVE_OK;
}

int32_t cave_hip_tight_cones_count(const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off, const float* sol,
                                   int64_t N, double tol, int32_t* n_rows, int64_t* n_ent, int32_t* status, void* stream) {
  return tight_cones_entry(false, sys, lazy, lazy_off, sol, N, tol, n_rows, n_ent, nullptr, 0, nullptr, nullptr, status, stream);
}

int32_t cave_hip_tight_cones_fill(const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off, const float* sol,
                                  int64_t N, double tol, const int64_t* ent_off, int64_t ent_cap, uint32_t* key, float* val,
                                  int32_t* status, void* stream) {
  return tight_cones_entry(true, sys, lazy, lazy_off, sol, N, tol, nullptr, nullptr, ent_off, ent_cap, key, val, status, stream);
}

// ------------------------------------------------------------------ APGD projector (apgd.h)

int32_t cave_hip_apgd_lds_bytes(int64_t m_max, int64_t d, int64_t nnz_cap) { return (int32_t)apgd_lds_bytes(m_max, d, nnz_cap); }

static int32_t apgd_entry(bool sparse, const float* ctrs, const cave_sparse_cones* cones, const float* pred, int64_t B, int64_t m_max,
                          int64_t d, int32_t mode, float sign, int32_t k_start, int32_t n_iter, int32_t power_iter, int32_t nnz_cap,
                          double* x_curr, double* x_prev, double* step, float* proj, float* rnorm, float* target, float* loss,
                          float* grad, int32_t* status, int32_t* iters, double* pgrad, void* stream) {
  ApgdParams P;
  int64_t grid;
  int waves;
  char msg[kSolverMsg];
  const int32_t rc = apgd_plan(sparse, ctrs, cones, pred, B, m_max, d, mode, sign, k_start, n_iter, power_iter, nnz_cap, x_curr, x_prev,
                               step, proj, rnorm, target, loss, grad, status, iters, pgrad, &P, &grid, &waves, msg);
  if (rc != CAVE_OK) return fail(rc, msg);
  if (grid == 0) return CAVE_OK;
  hipError_t e = waves == 1 ? launch_apgd_w1(sparse, (unsigned)grid, (hipStream_t)stream, P)
                            : launch_apgd_w4(sparse, (unsigned)grid, (hipStream_t)stream, P);
  if (e != hipSuccess) return fail(CAVE_E_LAUNCH, "launch apgd kernel", e);
  return CAVE_OK;
}

int32_t cave_hip_cone_apgd(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d, int32_t mode, float sign,
                           int32_t k_start, int32_t n_iter, int32_t power_iter, int32_t nnz_cap, double* x_curr, double* x_prev,
                           double* step, float* proj, float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                           int32_t* iters, double* pgrad, void* stream) {
  return apgd_entry(false, ctrs, nullptr, pred, B, m_max, d, mode, sign, k_start, n_iter, power_iter, nnz_cap, x_curr, x_prev, step, proj,
                    rnorm, target, loss, grad, status, iters, pgrad, stream);
}

int32_t cave_hip_cone_apgd_sparse(const cave_sparse_cones* cones, const float* pred, int32_t mode, float sign, int32_t k_start,
                                  int32_t n_iter, int32_t power_iter, int32_t nnz_cap, double* x_curr, double* x_prev, double* step,
                                  float* proj, float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                                  int32_t* iters, double* pgrad, void* stream) {
  return apgd_entry(true, nullptr, cones, pred, 0, 0, 0, mode, sign, k_start, n_iter, power_iter, nnz_cap, x_curr, x_prev, step, proj,
                    rnorm, target, loss, grad, status, iters, pgrad, stream);
}

}  // extern "C"
