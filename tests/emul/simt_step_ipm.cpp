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
#include "../../cave_amd/csrc/cone_step.h"

using namespace cave;

namespace {

using CtxSolo = SoloCtx<32, 4>;  // the solve half: one wave

struct Lds {  // exact-size, 16-byte aligned heap block standing in for the workgroup's LDS (as simt_abi.cpp): ASan sees overruns
  std::vector<unsigned char> raw;
  unsigned char* p;
  size_t len;
  explicit Lds(size_t n) : raw(n + 16), len(n) {
    const size_t off = (16 - ((uintptr_t)raw.data() & 15)) & 15;
    raw.resize(off + n);  // no slack behind the arena (shrinking keeps the buffer where it is)
    p = raw.data() + off;
  }
  void poison() { memset(p, 0xFF, len); }  // LDS is not cleared between workgroups: NaN as a float, 65535 as an index
};

bool lite_store_ok(const cave_lite_store* s, int64_t need, int64_t d) {  // (as cave_hip.hip)
  return s && s->n >= need && s->d == d && s->hdr && s->usign && s->avg && s->rowptr && s->ell && s->csr16 && s->rl &&
         (((uintptr_t)s->ell | (uintptr_t)s->csr16) & 15u) == 0;
}

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
  StepSolveParams P;
  P.store = *solve; P.ids = ids; P.pred = pred; P.B = B; P.mode = CAVE_MODE_INNER_IPM; P.sign = sign; P.inner_ratio = 0.0f;
  P.max_iter = max_iter > 0 ? max_iter : 3;
  P.flags = flags;
  P.o = OutPtrs{proj, rnorm, target, loss, grad, status, iters};
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
