// cone_entry.h — the host side of the cone entry points (cave_hip_cone_dense ... cave_hip_lite_from_packed): their
// argument checks, in the order and with the texts the C ABI has always had, and the fill of every parameter block, once
// each.  Plain host code, as solver_entry.h is for the exact solvers: the C ABI (cave_hip.hip) calls a *_plan function
// and launches; the emulation drivers (tests/emul, g++) call the same fills and checks, so the CPU tier runs the code the
// library runs.  A plan returns CAVE_OK, the kernel argument and the grid (0: nothing to do), or CAVE_E_INVALID and
// "<entry>: <what>" as the message; it makes no HIP call and never touches the library's last-error text.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "../../include/cave_hip.h"
#include "cone_instance.h"
#include "cone_step.h"

namespace cave {

static constexpr int kConeMsg = 256;  // bytes of a plan function's message buffer

inline int32_t cone_bad(char* msg, const char* who, const char* what) {
  snprintf(msg, kConeMsg, "%s: %s", who, what);
  return CAVE_E_INVALID;
}

// ------------------------------------------------------------------------------------------------ shared checks
inline bool dims_ok(int64_t B, int64_t m_max, int64_t d) { return B >= 0 && m_max >= 0 && d > 0 && d <= 65535; }
inline bool shape_ok(int64_t B, int64_t m_max, int64_t d, bool large) {
  return dims_ok(B, m_max, d) && (!large || m_max <= 65535) && m_max * d < (int64_t)1 << 32;
}
inline bool mode_ok(int32_t mode) { return mode >= CAVE_MODE_PROJECT && mode <= CAVE_MODE_INNER_IPM; }

inline bool waves_ok(int32_t& waves) {
  if (waves == 0) waves = 2;  // measured best at the benchmark size, no register spills, 64-row systems
  return waves == 1 || waves == 2 || waves == 4 || waves == 8;  // 8 = four waves, wide register budget
}

inline bool lite_store_ok(const cave_lite_store* s, int64_t need, int64_t d) {
  return s && s->n >= need && s->d == d && s->hdr && s->usign && s->avg && s->rowptr && s->ell && s->csr16 && s->rl &&
         (((uintptr_t)s->ell | (uintptr_t)s->csr16) & 15u) == 0 && ((4 * d) & 3) == 0;
}

// what is wrong with a multiplier cache (null: nothing)
inline const char* warm_cache_bad(const cave_warm_cache* warm) {
  const int64_t n = warm->n_entries;
  if (n <= 0 || n >= (int64_t)1 << 40 || (n & (n - 1)) != 0) return "n_entries must be a power of two";
  if (!warm->key || !warm->theta) return "null key / theta array";
  if (((uintptr_t)warm->theta & 15u) != 0) return "theta must be 16-byte aligned";
  return nullptr;
}

// slots [slot0, slot0 + B) of a packed store of dimension d
inline bool store_slot_ok(const cave_cone_store* store, int64_t d, int64_t slot0, int64_t B) {
  return store->d == d && slot0 >= 0 && slot0 + B <= store->n;
}

// workspace and LDS of a large-path launch (lds_bytes <= 0: 64 KiB)
inline int32_t check_large(const char* who, const void* workspace, int64_t slice_bytes, int32_t n_slots, int32_t& lds_bytes, char* msg) {
  if (!workspace || slice_bytes < 1024 || slice_bytes >= ((int64_t)1 << 32) || (slice_bytes & 7) || n_slots <= 0 ||
      ((uintptr_t)workspace & 15u))
    return cone_bad(msg, who, "bad workspace (16-byte aligned, 1 KiB <= slice_bytes < 4 GiB, multiple of 8, n_slots > 0)");
  if (lds_bytes <= 0) lds_bytes = 64 * 1024;
  if (lds_bytes < 1024 || (uint32_t)lds_bytes > kMaxLds) return cone_bad(msg, who, "bad lds_bytes");
  return CAVE_OK;
}

inline int32_t check_sparse(const char* who, const cave_sparse_cones* s, char* msg) {
  if (!s || s->B < 0 || s->m_max < 0 || s->m_max > 65535 || s->d <= 0 || s->d > 65535)
    return cone_bad(msg, who, "bad batch (need 0 <= m_max <= 65535, 0 < d <= 65535)");
  if (s->B > 0 && (!s->ent_off || !s->key || !s->val || (((uintptr_t)s->key | (uintptr_t)s->val) & 3u) || ((uintptr_t)s->ent_off & 7u)))
    return cone_bad(msg, who, "null or misaligned ent_off / key / val");
  return CAVE_OK;
}

inline int64_t large_grid(int64_t B, int32_t n_slots) { return B < n_slots ? B : (int64_t)n_slots; }

// ------------------------------------------------------------------------------------------------ fills
// max_iter <= 0: the default of the solver that runs (the interior-point steps: 3; the Newton loop: 100)
inline int32_t max_iter_or_default(int32_t max_iter, bool ipm) { return max_iter > 0 ? max_iter : (ipm ? 3 : 100); }

inline DenseParams dense_fill(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d, int32_t mode, float sign,
                              float inner_ratio, int32_t max_iter, int64_t nnz_cap, int32_t lds_bytes, const OutPtrs& o) {
  return DenseParams{ctrs, pred, B, (int32_t)m_max, (int32_t)d, mode, sign, inner_ratio,
                     max_iter_or_default(max_iter, mode == CAVE_MODE_INNER_IPM), (uint32_t)nnz_cap, (uint32_t)lds_bytes, o};
}

inline PackedParams packed_fill(const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B, int32_t mode, float sign,
                                float inner_ratio, int32_t max_iter, int32_t lds_bytes, const OutPtrs& o) {
  return PackedParams{*store, ids, pred, B, mode, sign, inner_ratio, max_iter_or_default(max_iter, mode == CAVE_MODE_INNER_IPM),
                      (uint32_t)lds_bytes, o};
}

// what PackParams and SparsePackParams share.  store null: the count pass (n_rows / n_nnz receive the sizes); else the
// fill pass into slots slot0 .. of `store`; the large path's one entry does either
template <class P>
inline void pack_fill_common(P& p, int64_t B, int64_t m_max, int64_t d, int64_t nnz_cap, int32_t lds_bytes, int32_t* n_rows,
                             int32_t* n_nnz, int32_t* status, const cave_cone_store* store, int64_t slot0) {
  p.B = B; p.m = (int32_t)m_max; p.d = (int32_t)d; p.nnz_cap = (uint32_t)nnz_cap; p.lds_bytes = (uint32_t)lds_bytes;
  p.n_rows = n_rows; p.n_nnz = n_nnz; p.status = status;
  if (store) { p.store = *store; p.slot0 = slot0; p.fill = 1; }
}
inline PackParams pack_fill_params(const float* ctrs, int64_t B, int64_t m_max, int64_t d, int64_t nnz_cap, int32_t lds_bytes,
                                   int32_t* n_rows, int32_t* n_nnz, int32_t* status, const cave_cone_store* store, int64_t slot0) {
  PackParams P;
  memset(&P, 0, sizeof(P));
  P.ctrs = ctrs;
  pack_fill_common(P, B, m_max, d, nnz_cap, lds_bytes, n_rows, n_nnz, status, store, slot0);
  return P;
}
inline SparsePackParams sparse_pack_fill(const cave_sparse_cones* s, int64_t nnz_cap, int32_t lds_bytes, int32_t* n_rows, int32_t* n_nnz,
                                         int32_t* status, const cave_cone_store* store, int64_t slot0) {
  SparsePackParams P;
  memset(&P, 0, sizeof(P));
  P.ent_off = s->ent_off; P.key = s->key; P.val = s->val;
  pack_fill_common(P, s->B, s->m_max, s->d, nnz_cap, lds_bytes, n_rows, n_nnz, status, store, slot0);
  return P;
}

inline StepSolveParams step_solve_fill(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode,
                                       float sign, float inner_ratio, int32_t max_iter, int32_t flags, const OutPtrs& o, bool ipm) {
  return StepSolveParams{*solve, ids, pred, B, mode, sign, inner_ratio, max_iter_or_default(max_iter, ipm), flags, o};
}

// nnz_cap: step_limits' figure for the shape
inline StepPackParams step_pack_fill(const float* ctrs, int64_t B, int64_t m_max, int64_t d, int32_t nnz_cap, const cave_lite_store* dst,
                                     int32_t* status) {
  return StepPackParams{ctrs, B, (int32_t)m_max, (int32_t)d, (uint32_t)nnz_cap, *dst, status, lite_pmax_table((int)d)};
}
inline StepSparsePackParams step_sparse_pack_fill(const cave_sparse_cones* s, int32_t nnz_cap, const cave_lite_store* dst, int32_t* status) {
  return StepSparsePackParams{s->ent_off, s->key, s->val, s->B, s->m_max, s->d, (uint32_t)nnz_cap, *dst, status, lite_pmax_table((int)s->d)};
}

// lds_extra: the LDS copy of a hit's multipliers beyond both arenas (step_warm_lds_extra of the launch's LDS)
inline StepWarm step_warm_fill(const cave_warm_cache* warm, const int64_t* keys, uint8_t* warm_hit, uint32_t lds_extra) {
  return StepWarm{warm->key, warm->theta, warm->n_entries, keys, warm_hit, lds_extra};
}

inline LiteFromPackedParams lite_from_packed_fill(const cave_cone_store* src, const cave_lite_store* dst, int32_t* status) {
  return LiteFromPackedParams{*src, *dst, src->n, lite_from_packed_lds_bytes(src->d), status, lite_pmax_table((int)src->d)};
}

// ------------------------------------------------------------------------------------------------ plans
// what a plan hands back: the kernel argument, the grid (0: nothing to do) and, on failure, the message
template <class P>
struct ConePlan {
  P params;
  int64_t grid;
  char msg[kConeMsg];
};

// cone_dense and cone_dense_large (`large`: nnz_cap and the workspace are the caller's, no `waves`)
inline int32_t dense_plan(const char* who, bool large, const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d,
                          int32_t mode, float sign, float inner_ratio, int32_t max_iter, int64_t nnz_cap, int32_t lds_bytes,
                          int32_t* waves, const void* workspace, int64_t slice_bytes, int32_t n_slots, const OutPtrs& o,
                          ConePlan<DenseParams>* L) {
  L->grid = 0;
  if (large) {
    if (!shape_ok(B, m_max, d, true)) return cone_bad(L->msg, who, "bad shape (need m_max, d <= 65535, m_max*d < 2^32)");
  } else {
    if (!dims_ok(B, m_max, d)) return cone_bad(L->msg, who, "bad shape (need 0 < d <= 65535)");
    if (!shape_ok(B, m_max, d, false)) return cone_bad(L->msg, who, "m_max*d must be < 2^32");
  }
  if (!mode_ok(mode)) return cone_bad(L->msg, who, "bad mode");
  if (B == 0) return CAVE_OK;
  if (!ctrs && m_max > 0) return cone_bad(L->msg, who, "ctrs is null");
  if (!pred && mode != CAVE_MODE_AVG) return cone_bad(L->msg, who, "pred is null");
  if (large) {
    if (nnz_cap <= 0 || nnz_cap >= (int64_t)1 << 31) return cone_bad(L->msg, who, "bad nnz_cap");
    if (check_large(who, workspace, slice_bytes, n_slots, lds_bytes, L->msg) != CAVE_OK) return CAVE_E_INVALID;
  } else {
    if (!waves_ok(*waves)) return cone_bad(L->msg, who, "waves must be 0, 1, 2, 4 or 8");
    // the one-wave lite solver only exists in the one- / two-wave shapes and only runs for grids of up to 2048
    int32_t cap = (int32_t)nnz_cap;
    if (!resolve_limits(m_max, d, cap, lds_bytes, *waves <= 2 && B <= 2048)) return cone_bad(L->msg, who, "bad nnz_cap / lds_bytes");
    nnz_cap = cap;
  }
  L->params = dense_fill(ctrs, pred, B, m_max, d, mode, sign, inner_ratio, max_iter, nnz_cap, lds_bytes, o);
  L->grid = large ? large_grid(B, n_slots) : B;
  return CAVE_OK;
}

// cone_packed and cone_packed_large (`large`: waves stays 0 where the caller leaves the shape to the entry)
inline int32_t packed_plan(const char* who, bool large, const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B,
                           int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t lds_bytes, int32_t* waves,
                           const void* workspace, int64_t slice_bytes, int32_t n_slots, const OutPtrs& o, ConePlan<PackedParams>* L) {
  L->grid = 0;
  if (!store || B < 0) return cone_bad(L->msg, who, "null store / bad B");
  if (!mode_ok(mode)) return cone_bad(L->msg, who, "bad mode");
  if (B == 0) return CAVE_OK;
  if (!pred && mode != CAVE_MODE_AVG) return cone_bad(L->msg, who, "pred is null");
  if (large) {
    if (check_large(who, workspace, slice_bytes, n_slots, lds_bytes, L->msg) != CAVE_OK) return CAVE_E_INVALID;
    if (*waves != 0 && *waves != 1 && *waves != 2 && *waves != 4) return cone_bad(L->msg, who, "waves must be 0, 1, 2 or 4");
  } else {
    if (lds_bytes <= 0 || (uint32_t)lds_bytes > kMaxLds) return cone_bad(L->msg, who, "bad lds_bytes");
    if (!waves_ok(*waves)) return cone_bad(L->msg, who, "waves must be 0, 1, 2, 4 or 8");
  }
  L->params = packed_fill(store, ids, pred, B, mode, sign, inner_ratio, max_iter, lds_bytes, o);
  L->grid = large ? large_grid(B, n_slots) : B;
  return CAVE_OK;
}

// The six pack entries: P = PackParams reads the dense block `ctrs` [B, m_max, d], P = SparsePackParams the batch `cones`
// (shape and size are the batch's; no one-wave shape).  kPackCount / kPackFill: the LDS path's two passes (nnz_cap,
// lds_bytes <= 0: the defaults); kPackLarge: the large path's one entry for both (store null: the count pass), 1 KiB of LDS.
enum PackPass { kPackCount, kPackFill, kPackLarge };
template <class P>
inline int32_t pack_plan(const char* who, PackPass pass, const float* ctrs, const cave_sparse_cones* cones, int64_t B, int64_t m_max,
                         int64_t d, int64_t nnz_cap, int32_t lds_bytes, int32_t* waves, const void* workspace, int64_t slice_bytes,
                         int32_t n_slots, int32_t* n_rows, int32_t* n_nnz, int32_t* status, const cave_cone_store* store, int64_t slot0,
                         ConePlan<P>* L) {
  constexpr bool sparse = std::is_same<P, SparsePackParams>::value;
  const bool large = pass == kPackLarge, fill = pass == kPackFill;
  L->grid = 0;
  if (sparse) {
    if (check_sparse(who, cones, L->msg) != CAVE_OK) return CAVE_E_INVALID;
    B = cones->B; m_max = cones->m_max; d = cones->d;
  } else if (!shape_ok(B, m_max, d, large)) return cone_bad(L->msg, who, "bad shape");
  if (B == 0) return CAVE_OK;
  if (large) {
    if (!sparse && !ctrs) return cone_bad(L->msg, who, "ctrs is null");
    if (!store && (!n_rows || !n_nnz)) return cone_bad(L->msg, who, "count pass needs n_rows and n_nnz");
    if (store && !store_slot_ok(store, d, slot0, B)) return cone_bad(L->msg, who, "store mismatch");
    if (nnz_cap <= 0 || nnz_cap >= (int64_t)1 << 31) return cone_bad(L->msg, who, "bad nnz_cap");
    lds_bytes = 1024;
    if (check_large(who, workspace, slice_bytes, n_slots, lds_bytes, L->msg) != CAVE_OK) return CAVE_E_INVALID;
  } else {
    if ((!sparse && !ctrs) || (fill ? !store : (!n_rows || !n_nnz))) return cone_bad(L->msg, who, "null pointer");
    if (fill && !store_slot_ok(store, d, slot0, B)) return cone_bad(L->msg, who, "store mismatch");
    int32_t cap = (int32_t)nnz_cap;
    if (!resolve_limits(m_max, d, cap, lds_bytes, false)) return cone_bad(L->msg, who, "bad limits");
    nnz_cap = cap;
    if (!waves_ok(*waves) || (sparse && *waves == 1))
      return cone_bad(L->msg, who, sparse ? "waves must be 0, 2, 4 or 8" : "waves must be 0, 1, 2, 4 or 8");
    if (fill && (store->n_rows == nullptr) != (store->n_nnz == nullptr)) return cone_bad(L->msg, who, "n_rows and n_nnz go together");
    if (!fill) store = nullptr;
  }
  if constexpr (sparse) L->params = sparse_pack_fill(cones, nnz_cap, lds_bytes, n_rows, n_nnz, status, store, slot0);
  else L->params = pack_fill_params(ctrs, B, m_max, d, nnz_cap, lds_bytes, n_rows, n_nnz, status, store, slot0);
  L->grid = large ? large_grid(B, n_slots) : B;
  return CAVE_OK;
}

inline int32_t lite_from_packed_plan(const cave_cone_store* src, const cave_lite_store* dst, int32_t* status, ConePlan<LiteFromPackedParams>* L) {
  const char* who = "lite_from_packed";
  L->grid = 0;
  if (!src || !dst) return cone_bad(L->msg, who, "null store");
  if (src->n == 0) return CAVE_OK;
  if (src->n < 0 || src->n >= (int64_t)1 << 31 || src->d <= 0 || src->d > kLiteMaxD) return cone_bad(L->msg, who, "need 0 < d <= 256, n < 2^31");
  if (!lite_store_ok(dst, src->n, src->d)) return cone_bad(L->msg, who, "bad lite store (size, d, null or unaligned array)");
  L->params = lite_from_packed_fill(src, dst, status);
  L->grid = src->n;
  return CAVE_OK;
}

// ------------------------------------------------------------------------------------------------ the fused step
// The five step entries in one plan.  The pack half is the NEXT batch as a dense block (next_ctrs, B_next, m_max, d;
// next_cones null) or on the sparse wire format (next_cones: shape and size are the batch's); a sparse entry without a
// next batch (null or empty) is the dense entry's solve-only call, under the dense entry's name, at the solve store's d.
enum StepLaunch { kStepCold, kStepIpm, kStepWarm };  // the kernel the call launches

struct StepPlan {
  const char* who;          // the entry the messages name: "cone_step" or "cone_step_sparse"
  bool sparse;              // X holds the launch's argument (else D)
  StepLaunch launch;
  int64_t grid;             // B + B_next (0: nothing to do)
  StepParamsWarm D;         // the cold and interior-point kernels take its StepParams part
  StepSparseParamsWarm X;
  char msg[kConeMsg];
};

// what is wrong with the solve half of a step call (null: nothing)
inline const char* step_solve_bad(bool ipm, const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode,
                                  int64_t d) {
  if (!ipm && (mode < CAVE_MODE_PROJECT || mode > CAVE_MODE_AVG)) return "bad mode (PROJECT .. AVG)";
  if (!pred && mode != CAVE_MODE_AVG) return "pred is null";
  if (!lite_store_ok(solve, ids ? 1 : B, d)) return "bad solve store (size, d, null or unaligned array)";
  return nullptr;
}

// sparse_entry: called for cave_hip_cone_step_sparse(_ipm).  ipm: mode is CAVE_MODE_INNER_IPM, no cache, max_iter <= 0 = 3
inline int32_t step_plan(bool sparse_entry, bool ipm, const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B,
                         int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t flags, const OutPtrs& o,
                         const float* next_ctrs, int64_t B_next, int64_t m_max, int64_t d, const cave_sparse_cones* next_cones,
                         const cave_lite_store* next, int32_t* pack_status, const cave_warm_cache* warm, const int64_t* keys,
                         uint8_t* warm_hit, uint32_t* cu_tickets, StepPlan* L) {
  memset(L, 0, sizeof(*L));
  char* msg = L->msg;
  if (sparse_entry && (!next_cones || next_cones->B == 0)) {
    // solve only: the dense entry point's launch (the same kernel, the same bits); d is the store's
    if (B > 0 && !solve) return cone_bad(msg, "cone_step_sparse", "solve store is null");
    next_cones = nullptr; next_ctrs = nullptr; B_next = 0; m_max = 0; d = solve ? solve->d : 1; next = nullptr; pack_status = nullptr;
  }
  const bool sparse = next_cones != nullptr;
  const char* who = sparse ? "cone_step_sparse" : "cone_step";
  L->who = who;
  L->sparse = sparse;
  const char* what = warm ? warm_cache_bad(warm) : nullptr;
  if (what) return cone_bad(msg, sparse ? who : "cone_step_warm", what);
  if (sparse) {
    if (check_sparse(who, next_cones, msg) != CAVE_OK) return CAVE_E_INVALID;
    B_next = next_cones->B; m_max = next_cones->m_max; d = next_cones->d;
  }
  if (B < 0 || B_next < 0 || B + B_next >= (int64_t)1 << 31) return cone_bad(msg, who, "bad batch sizes");
  if (B == 0 && B_next == 0) return CAVE_OK;
  if (!sparse && (d <= 0 || d > kLiteMaxD)) return cone_bad(msg, who, "need 0 < d <= 256");
  if (!cu_tickets) return cone_bad(msg, who, "cu_tickets is null");
  // the dense entries check the solve half, then the shape, then the pack half; the sparse ones the shape and the pack
  // half, then the solve half
  int32_t cap = 0, lds = 0;
  if (sparse) {
    if (m_max <= 0 || step_limits(m_max, d, cap, lds) != CAVE_OK) return cone_bad(msg, who, "shape does not qualify (cave_hip_step_lds_bytes)");
    if (!next) return cone_bad(msg, who, "next store is null");
    if (next->d != d || (B > 0 && solve && solve->d != d)) return cone_bad(msg, who, "d of the batch differs from the store's d");
    if (!lite_store_ok(next, B_next, d)) return cone_bad(msg, who, "bad next store (size, d, null or unaligned array)");
  }
  if (B > 0 && (what = step_solve_bad(ipm, solve, ids, pred, B, mode, d)) != nullptr) return cone_bad(msg, who, what);
  if (!sparse) {
    if (step_limits(B_next > 0 ? m_max : 0, d, cap, lds) != CAVE_OK) return cone_bad(msg, who, "shape does not qualify (cave_hip_step_lds_bytes)");
    if (B_next > 0) {
      if (m_max <= 0 || m_max * d >= (int64_t)1 << 32) return cone_bad(msg, who, "bad m_max");
      if (!next_ctrs) return cone_bad(msg, who, "next_ctrs is null");
      if (!lite_store_ok(next, B_next, d)) return cone_bad(msg, who, "bad next store (size, d, null or unaligned array)");
    }
  }
  if (B > 0 && B_next > 0 && next->hdr == solve->hdr) return cone_bad(msg, who, "solve and next must be different stores");
  // (a pack-only launch has nothing to warm, and its pack half is the cold kernel's code: the cold kernel)
  L->launch = B == 0 ? kStepCold : warm ? kStepWarm : ipm ? kStepIpm : kStepCold;
  StepSolveParams& S = sparse ? L->X.S : L->D.S;  // (a half that has nothing to do stays zero: S.B or Q.B = 0)
  StepWarm& W = sparse ? L->X.W : L->D.W;
  if (B > 0) S = step_solve_fill(solve, ids, pred, B, mode, sign, inner_ratio, max_iter, flags, o, ipm);
  if (L->launch == kStepWarm) W = step_warm_fill(warm, keys, warm_hit, step_warm_lds_extra((uint32_t)lds, B_next > 0));
  if (sparse) L->X.Q = step_sparse_pack_fill(next_cones, cap, next, pack_status);
  else if (B_next > 0) L->D.Q = step_pack_fill(next_ctrs, B_next, m_max, d, cap, next, pack_status);
  (sparse ? L->X.lds_bytes : L->D.lds_bytes) = (uint32_t)lds + W.lds_extra;
  (sparse ? L->X.tickets : L->D.tickets) = cu_tickets;
  L->grid = B + B_next;
  return CAVE_OK;
}

}  // namespace cave
