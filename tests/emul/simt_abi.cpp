// simt_abi.cpp — SIMT emulation build of the GPU code paths (TEST INFRASTRUCTURE ONLY).
//
// Compiles cave_amd/csrc exactly as the HIP build sees it -- wave contexts, DPP / readlane / ballot primitives,
// the one-wave lite solver, the one-/two-wave band elimination, the blocked dense LDL^T -- with g++ against the
// shim in tests/emul/simt/hip/hip_runtime.h: every lane of a workgroup is a fiber, every cross-lane primitive and
// barrier a rendezvous.  Runs under -fsanitize=address,undefined in the CPU test tier.  Exports cave_simt_* with the
// signatures of include/cave_hip.h (host pointers, no stream, + a schedule seed: 0 = round robin, else the lanes
// between two rendezvous run in a seeded random order).  Never loaded by cave_amd.
//
// The fused step kernel (cone_step.h) is here too: its pack half (run_pack_lite_instance on the two-wave context the
// product instantiates), its solve half (run_lite_instance<SoloCtx<32, 4>, WARM>, cold and with the multiplier cache)
// and run_lite_from_packed, with the LDS figures of the product's own step_limits / lite_from_packed_lds_bytes.  NOT
// emulated: the wave election of a solve block (kernels.h step_elect_wave reads hardware registers) and the wave
// priorities; the solve entry calls run_lite_instance behind the election words exactly as the kernel wrapper does.
#define CAVE_SIMT_EMUL 1
#define CAVE_EMUL_COUNTERS 1
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/cave_hip.h"
#include "../../cave_amd/csrc/cone_common.h"
#include "../../cave_amd/csrc/cone_core.h"
#include "../../cave_amd/csrc/ctx_wave.h"
#include "../../cave_amd/csrc/ctx_block.h"
#include "../../cave_amd/csrc/cone_instance.h"
#include "../../cave_amd/csrc/cone_entry.h"
#include "simt_solver.h"
#include "../prims/prim_entries.h"
#ifdef CAVE_SIMT_OPS  // the plain build only: the sanitizer and variant builds keep their compile time
#include "../prims/op_entries.h"
#endif

using namespace cave;

namespace {

using Ctx1 = WaveCtx;
using Ctx2 = BlockCtx<2>;
using Ctx4 = BlockCtx<4>;
using CtxW = BlockCtx<4, true>;
using CtxL = BlockCtx<4, true>;
using CtxL2 = BlockCtx<2, true>;
using CtxStep = BlockCtx<2, true>;  // pack half of the step kernel (k_step.hip)
using CtxSolo = SoloCtx<32, 4>;      // its solve half: one wave

// LDS is not cleared between workgroups: a block starts on whatever the last one left there.  The step entries poison
// the block before every workgroup (0xFF bytes: NaN as a double or float, 65535 as an index), so that a read of LDS the
// workgroup has not written shows up as a wrong result instead of a convenient zero
using simt_solver::Lds;

template <class C, class F>
void launch(int64_t B, unsigned grid, uint64_t seed, F&& body) {  // one workgroup per instance
  for (int64_t b = 0; b < B; ++b) {
    simt::run_block(C::NT, (unsigned)b, grid, [&]() { body(b); }, seed ? seed + (uint64_t)b : 0);
  }
}

template <class C>
int32_t packed_impl(const PackedParams& P, uint64_t seed) {
  Lds lds(P.lds_bytes);
  launch<C>(P.B, (unsigned)P.B, seed, [&](int64_t b) {
    C c;
    c.init(lds.p);
    run_packed_instance(c, lds.p, P, b);
  });
  return CAVE_OK;
}

template <class C>
int32_t dense_impl(const DenseParams& P, uint64_t seed) {
  Lds lds(P.lds_bytes);
  launch<C>(P.B, (unsigned)P.B, seed, [&](int64_t b) {
    C c;
    c.init(lds.p);
    run_dense_instance(c, lds.p, P, b);
  });
  return CAVE_OK;
}

template <class C>
int32_t pack_impl(const PackParams& P, uint64_t seed) {
  Lds lds(P.lds_bytes);
  launch<C>(P.B, (unsigned)P.B, seed, [&](int64_t b) {
    C c;
    c.init(lds.p);
    run_pack_instance(c, lds.p, P, b);
  });
  return CAVE_OK;
}

template <class C>
int32_t packed_large_impl(const PackedParams& P, int64_t slice_bytes, uint64_t seed) {
  Lds lds(P.lds_bytes);
  std::vector<unsigned char> ws((size_t)slice_bytes + 16);
  unsigned char* wsp = ws.data() + ((16 - ((uintptr_t)ws.data() & 15)) & 15);
  launch<C>(P.B, (unsigned)P.B, seed, [&](int64_t b) {
    C c;
    c.init(lds.p);
    run_packed_large_instance<C>(c, lds.p, P, b, wsp, (uint32_t)slice_bytes);
  });
  return CAVE_OK;
}

// solve half of the step kernel: one 64-lane wave per instance.  `lds` is the launch's LDS without the warm variant's
// extra block, `extra` that block (kernels.h cone_step_kernel: lds_bytes -= W.lds_extra; smem + kStepElectBytes)
template <bool WARM>
void step_solve_impl(const StepSolveParams& P, const StepWarm& W, uint32_t lds, uint32_t extra, uint64_t seed) {
  Lds mem((size_t)lds + extra);
  launch<CtxSolo>(P.B, (unsigned)P.B, seed, [&](int64_t b) {
    if (simt::tid() == 0) mem.poison();
    simt::block_sync();
    CtxSolo sc;
    sc.lane = simt::lane();
    run_lite_instance<CtxSolo, WARM>(sc, mem.p + kStepElectBytes, lds - kStepElectBytes, P, b, W);
  });
}

// one solver alone (tests/prims/prim_entries.h): the workgroup's LDS is an exact-size block, poisoned before every system
template <int KIND>
int32_t prim_impl(const cave_prims::PrimBatch& a, uint64_t seed) {
  using C = typename cave_prims::PrimCtx<KIND>::type;
  Lds mem(cave_prims::kind_lds_bytes(KIND, a.p, a.nF, a.bw));
  launch<C>(a.B, (unsigned)a.B, seed, [&](int64_t b) {
    if (simt::tid() == 0) mem.poison();
    simt::block_sync();
    cave_prims::prim_body<KIND>(mem.p, a, b);
  });
  return CAVE_OK;
}

#ifdef CAVE_SIMT_OPS
// one operator alone (tests/prims/op_entries.h): an exact-size LDS block per case, poisoned before it runs
template <int OP, int CX, bool PM1>
int32_t op_impl(const cave_ops::OpCase* cases, int64_t B, uint64_t seed) {
  using C = typename cave_ops::OpCtx<CX>::type;
  for (int64_t b = 0; b < B; ++b) {
    if (!cave_ops::op_case_valid(OP, PM1, cases[b])) return CAVE_E_INVALID;
    Lds mem(cave_ops::op_lds_bytes(OP, PM1, cases[b]));
    mem.poison();
    simt::run_block(C::NT, (unsigned)b, (unsigned)B, [&]() { cave_ops::op_body<OP, CX, PM1>(mem.p, cases[b]); },
                    seed ? seed + (uint64_t)b : 0);
  }
  return CAVE_OK;
}

#endif  // CAVE_SIMT_OPS

}  // namespace

extern "C" {

// ---- the linear solvers alone (tests/prims/prim_entries.h); seed as everywhere here
int32_t cave_simt_prim_run(int32_t kind, const cave_prims::PrimBatch* a, uint64_t seed) {
  if (!a || a->B < 0 || !cave_prims::kind_valid(kind, a->p, a->nF, a->bw, a->n_ex)) return CAVE_E_INVALID;
  switch (kind) {
#define CAVE_PRIM_CASE(K) case K: return prim_impl<K>(*a, seed);
    CAVE_PRIM_KINDS(CAVE_PRIM_CASE)
#undef CAVE_PRIM_CASE
  }
  return CAVE_E_INVALID;
}
int64_t cave_simt_prim_info(int32_t kind, int32_t what, int32_t p, int32_t nF, int32_t bw) {  // sizes the caller allocates by
  using namespace cave_prims;
  if (!kind_valid(kind, p, nF, bw, 0)) return -1;
  switch (what) {
    case 0: return kind_h_entries(kind, p, bw);
    case 1: return kind_ws_entries(kind, p, bw);
    case 2: return kind_lds_bytes(kind, p, nF, bw);
  }
  return -1;
}

#ifdef CAVE_SIMT_OPS
// ---- the operators alone (tests/prims/op_entries.h)
int32_t cave_simt_op_run(int32_t kind, const cave_ops::OpCase* cases, int64_t B, uint64_t seed) {
  using namespace cave_ops;
  if (!cases || B < 0) return CAVE_E_INVALID;
  switch (kind) {
#define CAVE_OP_CASE(OP, CX, PM1) case op_kind(OP, CX, PM1): return op_impl<OP, CX, PM1>(cases, B, seed);
    CAVE_OP_KINDS(CAVE_OP_CASE)
#undef CAVE_OP_CASE
  }
  return CAVE_E_INVALID;
}
int32_t cave_simt_op_case_bytes(void) { return (int32_t)sizeof(cave_ops::OpCase); }
double cave_simt_exact_step(const double* x, const double* y, int32_t n, double psi0, double amax, int32_t* n_eval) {
  int ne = 0;
  const double a = cave_ops::exact_step_driver(x, y, n, psi0, amax, &ne);
  if (n_eval) *n_eval = ne;
  return a;
}
double cave_simt_psitol(void) { return CAVE_PSITOL; }
#endif  // CAVE_SIMT_OPS

// ---- fused step (cone_step.h)
int32_t cave_simt_step_lds_bytes(int64_t m_max, int64_t d) {  // what cave_hip_step_lds_bytes returns
  int32_t cap = 0, lds = 0;
  const int32_t rc = step_limits(m_max, d, cap, lds);
  return rc == CAVE_OK ? lds : rc;
}
int32_t cave_simt_step_solve_lds_bytes(int64_t d) { return (int32_t)step_solve_lds_bytes(d); }
int32_t cave_simt_step_warm_lds_extra(int32_t lds, int32_t has_pack) { return (int32_t)step_warm_lds_extra((uint32_t)lds, has_pack != 0); }
// the rule by which write_lite_slot accepts a cone of p reduced rows, nI of them with bounds (cone_step.h)
int32_t cave_simt_lite_scratch_fits(int32_t d, int32_t p, int32_t nI) {
  return (lite_scratch_fits(d, p, nI) ? 1 : 0) | (lite_pmax_allows(lite_pmax_table(d), p, nI) ? 2 : 0);  // bit 0: the rule, bit 1: as the kernels read it
}
int32_t cave_simt_lite_from_packed_lds_bytes(int64_t d) { return (int32_t)lite_from_packed_lds_bytes(d); }
uint64_t cave_simt_lite_content_key(uint32_t fp, int32_t p, int32_t nF, uint32_t nnz) { return lite_content_key(fp, p, nF, nnz); }

// pack half: instances [0, B) of ctrs [B, m_max, d] into slots [0, B) of `dst`; LDS and non-zero cap of the product
int32_t cave_simt_step_pack(const float* ctrs, int64_t B, int64_t m_max, int64_t d, uint64_t seed,
                            const cave_lite_store* dst, int32_t* status) {
  int32_t cap = 0, lds = 0;
  if (B < 0 || m_max <= 0 || step_limits(m_max, d, cap, lds) != CAVE_OK || !lite_store_ok(dst, B, d)) return CAVE_E_INVALID;
  const StepPackParams Q = step_pack_fill(ctrs, B, m_max, d, cap, dst, status);
  Lds mem((size_t)lds);
  launch<CtxStep>(B, (unsigned)B, seed, [&](int64_t b) {
    if (simt::tid() == 0) mem.poison();
    simt::block_sync();
    CtxStep c;
    c.init(mem.p);
    run_pack_lite_instance(c, mem.p, (uint32_t)lds, Q, b);
  });
  return CAVE_OK;
}

// solve half.  lds_bytes: LDS of the launch (a value of cave_simt_step_lds_bytes); lds_extra: the warm variant's block
// behind it (cone_step.h step_warm_lds_extra: 256 when the residency allows it, else 0).  warm == NULL: the cold kernel.
int32_t cave_simt_step_solve(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode,
                             float sign, float inner_ratio, int32_t max_iter, int32_t flags, int32_t lds_bytes,
                             int32_t lds_extra, const cave_warm_cache* warm, const int64_t* keys, uint8_t* warm_hit,
                             uint64_t seed, float* proj, float* rnorm, float* target, float* loss, float* grad,
                             int32_t* status, int32_t* iters) {
  if (B < 0 || mode < CAVE_MODE_PROJECT || mode > CAVE_MODE_AVG || (!pred && mode != CAVE_MODE_AVG)) return CAVE_E_INVALID;
  if (!solve || !lite_store_ok(solve, ids ? 1 : B, solve->d)) return CAVE_E_INVALID;
  if (lds_bytes <= (int32_t)kStepElectBytes || lds_extra < 0) return CAVE_E_INVALID;
  const StepSolveParams P = step_solve_fill(solve, ids, pred, B, mode, sign, inner_ratio, max_iter, flags,
                                            OutPtrs{proj, rnorm, target, loss, grad, status, iters}, false);
  if (warm) {
    if (warm_cache_bad(warm)) return CAVE_E_INVALID;
    step_solve_impl<true>(P, step_warm_fill(warm, keys, warm_hit, (uint32_t)lds_extra), (uint32_t)lds_bytes, (uint32_t)lds_extra, seed);
  } else {
    if (warm_hit) memset(warm_hit, 0, (size_t)B);
    step_solve_impl<false>(P, StepWarm{}, (uint32_t)lds_bytes, 0u, seed);
  }
  return CAVE_OK;
}

// slot i of `dst` from slot i of the packed store `src` (lite_from_packed_kernel<Ctx2>)
int32_t cave_simt_lite_from_packed(const cave_cone_store* src, const cave_lite_store* dst, int32_t* status, uint64_t seed) {
  ConePlan<LiteFromPackedParams> L;  // the library's own checks
  if (lite_from_packed_plan(src, dst, status, &L) != CAVE_OK) return CAVE_E_INVALID;
  const LiteFromPackedParams& P = L.params;
  if (L.grid == 0) return CAVE_OK;
  Lds mem((size_t)P.lds_bytes);
  launch<Ctx2>(P.n, (unsigned)P.n, seed, [&](int64_t b) {
    if (simt::tid() == 0) mem.poison();
    simt::block_sync();
    Ctx2 c;
    c.init(mem.p);
    run_lite_from_packed(c, mem.p, P, b);
  });
  return CAVE_OK;
}


void cave_simt_path_counters(long* out) {
  for (int i = 0; i < 8; ++i) { out[i] = emul_counters()[i]; emul_counters()[i] = 0; }
}
void cave_simt_stats(unsigned long* out) {  // context switches, rendezvous since the start
  out[0] = simt::S().switches;
  out[1] = simt::S().rendezvous;
}

int32_t cave_simt_packed_lds_bytes(int64_t d, int32_t max_rows, int32_t max_nnz, int32_t all_pm1) {
  int32_t s = all_pm1 == 3 ? packed_lds_bytes(d, max_rows, max_nnz, true, false, true)   // the diet layout
                           : packed_lds_bytes(d, max_rows, max_nnz, all_pm1 != 0, all_pm1 != 2);
  return s < 0 ? CAVE_E_INVALID : s;
}
int32_t cave_simt_packed_large_lds_bytes(int32_t max_rows, int32_t max_bw) {
  return (int32_t)packed_large_lds_bytes(max_rows, max_bw);
}
int64_t cave_simt_packed_large_slice_bytes(int64_t d, int64_t max_rows, int64_t band_entries) {
  return (int64_t)packed_large_slice_bytes(d, max_rows, band_entries);
}

int32_t cave_simt_cone_dense(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d, int32_t mode,
                             float sign, float inner_ratio, int32_t max_iter, int32_t nnz_cap, int32_t lds_bytes,
                             int32_t waves, uint64_t seed, float* proj, float* rnorm, float* target, float* loss,
                             float* grad, int32_t* status, int32_t* iters) {
  if (!resolve_limits(m_max, d, nnz_cap, lds_bytes, waves <= 2 && B <= 2048)) return CAVE_E_INVALID;
  const DenseParams P = dense_fill(ctrs, pred, B, m_max, d, mode, sign, inner_ratio, max_iter, nnz_cap, lds_bytes,
                                   OutPtrs{proj, rnorm, target, loss, grad, status, iters});
  switch (waves) {
    case 1: return dense_impl<Ctx1>(P, seed);
    case 2: return dense_impl<Ctx2>(P, seed);
    case 4: return dense_impl<Ctx4>(P, seed);
    case 8: return dense_impl<CtxW>(P, seed);
  }
  return CAVE_E_INVALID;
}

int32_t cave_simt_pack_fill(const float* ctrs, int64_t B, int64_t m_max, int64_t d, int32_t nnz_cap, int32_t lds_bytes,
                            int32_t waves, uint64_t seed, const cave_cone_store* store, int64_t slot0, int32_t* n_rows,
                            int32_t* n_nnz, int32_t* status) {
  if (!resolve_limits(m_max, d, nnz_cap, lds_bytes, false)) return CAVE_E_INVALID;
  const PackParams P = pack_fill_params(ctrs, B, m_max, d, nnz_cap, lds_bytes, n_rows, n_nnz, status, store, slot0);
  switch (waves) {
    case 1: return pack_impl<Ctx1>(P, seed);
    case 2: return pack_impl<Ctx2>(P, seed);
    case 4: return pack_impl<Ctx4>(P, seed);
    case 8: return pack_impl<CtxW>(P, seed);
  }
  return CAVE_E_INVALID;
}

int32_t cave_simt_cone_packed(const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B,
                              int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t lds_bytes,
                              int32_t waves, uint64_t seed, float* proj, float* rnorm, float* target, float* loss,
                              float* grad, int32_t* status, int32_t* iters) {
  if (!store || lds_bytes <= 0) return CAVE_E_INVALID;
  const PackedParams P = packed_fill(store, ids, pred, B, mode, sign, inner_ratio, max_iter, lds_bytes,
                                     OutPtrs{proj, rnorm, target, loss, grad, status, iters});
  switch (waves) {
    case 1: return packed_impl<Ctx1>(P, seed);
    case 2: return packed_impl<Ctx2>(P, seed);
    case 4: return packed_impl<Ctx4>(P, seed);
    case 8: return packed_impl<CtxW>(P, seed);
  }
  return CAVE_E_INVALID;
}

int32_t cave_simt_cone_packed_large(const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B,
                                    int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t lds_bytes,
                                    int32_t waves, int64_t slice_bytes, uint64_t seed, float* proj, float* rnorm,
                                    float* target, float* loss, float* grad, int32_t* status, int32_t* iters) {
  if (!store || lds_bytes <= 0 || slice_bytes <= 0 || slice_bytes >= ((int64_t)1 << 32)) return CAVE_E_INVALID;
  const PackedParams P = packed_fill(store, ids, pred, B, mode, sign, inner_ratio, max_iter, lds_bytes,
                                     OutPtrs{proj, rnorm, target, loss, grad, status, iters});
  switch (waves) {
    case 1: return packed_large_impl<Ctx1>(P, slice_bytes, seed);
    case 2: return packed_large_impl<CtxL2>(P, slice_bytes, seed);
    case 4: return packed_large_impl<CtxL>(P, slice_bytes, seed);
  }
  return CAVE_E_INVALID;
}

}  // extern "C"
