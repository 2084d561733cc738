// simt_step_sparse.cpp — SIMT emulation of the step kernel's SPARSE pack half (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_abi.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin, else
// the lanes between two rendezvous run in a seeded random order).  It holds ONE code path, so that it builds in a
// fraction of the time simt_abi.cpp takes: run_pack_sparse_lite_instance (cone_step.h) on the two-wave context the
// product instantiates (BlockCtx<2, true>), with the LDS of the product's own step_limits as an exact-size block,
// poisoned before every workgroup, and the product's non-zero capacity.  The tests load it beside the library of
// simt_abi.cpp, whose cave_simt_step_pack (the dense pack half) and cave_simt_step_solve work on the same host stores.
// Never loaded by cave_amd.
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

using CtxStep = BlockCtx<2, true>;  // pack half of the step kernels (k_step_sparse.hip)

using simt_solver::Lds;  // exact-size block standing in for the workgroup's LDS, poisoned before every workgroup

}  // namespace

extern "C" {

// pack half from the sparse wire format: the instances of `cones` (host arrays) into slots [0, B) of `dst`
int32_t cave_simt_step_pack_sparse(const cave_sparse_cones* cones, uint64_t seed, const cave_lite_store* dst, int32_t* status) {
  if (!cones || cones->B < 0 || cones->m_max <= 0 || cones->d <= 0) return CAVE_E_INVALID;
  if (cones->B > 0 && (!cones->ent_off || !cones->key || !cones->val)) return CAVE_E_INVALID;
  int32_t cap = 0, lds = 0;
  if (step_limits(cones->m_max, cones->d, cap, lds) != CAVE_OK || !lite_store_ok(dst, cones->B, cones->d)) return CAVE_E_INVALID;
  const StepSparsePackParams Q = step_sparse_pack_fill(cones, cap, dst, status);
  Lds mem((size_t)lds);
  for (int64_t b = 0; b < Q.B; ++b) {  // one workgroup per instance
    simt::run_block(CtxStep::NT, (unsigned)b, (unsigned)Q.B, [&]() {
      if (simt::tid() == 0) mem.poison();
      simt::block_sync();
      CtxStep c;
      c.init(mem.p);
      run_pack_sparse_lite_instance(c, mem.p, (uint32_t)lds, Q, b);
    }, seed ? seed + (uint64_t)b : 0);
  }
  return CAVE_OK;
}

// the non-zero capacity of the pack half for a shape (step_limits): what the tests size an over-full instance by
int32_t cave_simt_step_nnz_cap(int64_t m_max, int64_t d) {
  int32_t cap = 0, lds = 0;
  return step_limits(m_max, d, cap, lds) == CAVE_OK ? cap : CAVE_E_INVALID;
}

}  // extern "C"
