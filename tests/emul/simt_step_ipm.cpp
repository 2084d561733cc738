// simt_step_ipm.cpp — SIMT emulation of the step kernel's INTERIOR-POINT solve half (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_abi.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin, else
// the lanes between two rendezvous run in a seeded random order), as simt_step_sparse.cpp is.  It holds ONE code path:
// run_lite_instance<SoloCtx<32, 4>, false, /*IPM*/ true> (cone_step.h; cone_core.h lite_solve_ipm), one 64-lane wave per
// instance, behind the election words exactly as the kernel wrapper calls it, on an exact-size LDS block that is
// poisoned before every instance.  The tests load it beside the library of simt_abi.cpp, whose cave_simt_step_pack and
// cave_simt_lite_from_packed fill the host stores it reads.  Never loaded by cave_amd.
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

using namespace cave;

namespace {

using CtxSolo = SoloCtx<32, 4>;  // the solve half: one wave

using simt_solver::Lds;  // exact-size block standing in for the workgroup's LDS, poisoned before every instance

}  // namespace

extern "C" {

// the solve half of cave_hip_cone_step_ipm: max_iter <= 0 means 3.  lds_bytes: LDS of the launch (a value of
// cave_hip_step_lds_bytes; step_solve_lds_bytes(d) for the solve-only launch of a device-resident store)
int32_t cave_simt_step_solve_ipm(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, float sign,
                                 int32_t max_iter, int32_t flags, int32_t lds_bytes, uint64_t seed, float* proj, float* rnorm,
                                 float* target, float* loss, float* grad, int32_t* status, int32_t* iters) {
  if (B < 0 || !pred) return CAVE_E_INVALID;
  if (!solve || !lite_store_ok(solve, ids ? 1 : B, solve->d)) return CAVE_E_INVALID;
  if (lds_bytes <= (int32_t)kStepElectBytes) return CAVE_E_INVALID;
  const StepSolveParams P = step_solve_fill(solve, ids, pred, B, CAVE_MODE_INNER_IPM, sign, 0.0f, max_iter, flags,
                                            OutPtrs{proj, rnorm, target, loss, grad, status, iters}, true);
  const StepWarm W{};
  Lds mem((size_t)lds_bytes);
  for (int64_t b = 0; b < B; ++b) {  // one wave per instance
    simt::run_block(CtxSolo::NT, (unsigned)b, (unsigned)B, [&]() {
      if (simt::tid() == 0) mem.poison();
      simt::block_sync();
      CtxSolo sc;
      sc.lane = simt::lane();
      run_lite_instance<CtxSolo, false, true>(sc, mem.p + kStepElectBytes, (uint32_t)lds_bytes - kStepElectBytes, P, b, W);
    }, seed ? seed + (uint64_t)b : 0);
  }
  return CAVE_OK;
}

int32_t cave_simt_step_ipm_solve_lds_bytes(int64_t d) { return (int32_t)step_solve_lds_bytes(d); }

}  // extern "C"
