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
#include "../../cave_amd/csrc/cone_step.h"

using namespace cave;

namespace {

using CtxStep = BlockCtx<2, true>;  // pack half of the step kernels (k_step_sparse.hip)

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

// pack half from the sparse wire format: the instances of `cones` (host arrays) into slots [0, B) of `dst`
int32_t cave_simt_step_pack_sparse(const cave_sparse_cones* cones, uint64_t seed, const cave_lite_store* dst, int32_t* status) {
  if (!cones || cones->B < 0 || cones->m_max <= 0 || cones->d <= 0) return CAVE_E_INVALID;
  if (cones->B > 0 && (!cones->ent_off || !cones->key || !cones->val)) return CAVE_E_INVALID;
  int32_t cap = 0, lds = 0;
  if (step_limits(cones->m_max, cones->d, cap, lds) != CAVE_OK || !lite_store_ok(dst, cones->B, cones->d)) return CAVE_E_INVALID;
  StepSparsePackParams Q;
  Q.ent_off = cones->ent_off; Q.key = cones->key; Q.val = cones->val; Q.B = cones->B; Q.m = cones->m_max; Q.d = cones->d;
  Q.nnz_cap = (uint32_t)cap; Q.store = *dst; Q.status = status; Q.lite_pmax = lite_pmax_table((int)cones->d);
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
