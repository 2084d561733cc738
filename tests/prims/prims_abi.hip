// prims_abi.hip — the linear solvers of the Newton loop as kernels of their own (TEST INFRASTRUCTURE ONLY).
//
// tests/prims/prim_entries.h compiled by hipcc for gfx950 with the product's flags: one workgroup per system, the
// product's context types and launch bounds.  Built into tests/prims/_prims.so by tests/prims/prims_lib.py; never loaded
// by cave_amd.  Compiled a second time with -DCAVE_DENSE_NO_MFMA -DCAVE_PRIMS_SUFFIX=_nomfma (dense entries only),
// so that both forms of the trailing update of cone_dense.h run on the same hardware.
#include <hip/hip_runtime.h>

#include "cave_hip.h"
#include "cone_common.h"
#include "cone_core.h"
#include "ctx_wave.h"
#include "ctx_block.h"
#include "prim_entries.h"

using namespace cave_prims;

#ifndef CAVE_PRIMS_SUFFIX
#define CAVE_PRIMS_SUFFIX
#endif
#define CAVE_PRIMS_CAT2(a, b) a##b
#define CAVE_PRIMS_CAT(a, b) CAVE_PRIMS_CAT2(a, b)
#define CAVE_PRIMS_SYM(name) CAVE_PRIMS_CAT(name, CAVE_PRIMS_SUFFIX)

namespace {

template <int KIND>
__global__ __launch_bounds__(kind_threads(KIND), CtxInfo<typename PrimCtx<KIND>::type>::min_waves) void prim_kernel(PrimBatch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  prim_body<KIND>(smem, a, (int64_t)blockIdx.x);
}

template <int KIND>
int32_t prim_launch(const PrimBatch& a, hipStream_t stream) {
  const uint32_t lds = kind_lds_bytes(KIND, a.p, a.nF, a.bw);
  if (lds > 160u * 1024u) return CAVE_E_INVALID;
  if (a.B == 0) return CAVE_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(prim_kernel<KIND>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return CAVE_E_INVALID;
  hipLaunchKernelGGL(prim_kernel<KIND>, dim3((unsigned)a.B), dim3((unsigned)kind_threads(KIND)), lds, stream, a);
  return hipGetLastError() == hipSuccess ? CAVE_OK : CAVE_E_INVALID;
}

}  // namespace

extern "C" {

// every pointer of `a` is device memory; the launch goes to `stream` and is not waited for
int32_t CAVE_PRIMS_SYM(cave_prims_run)(int32_t kind, const PrimBatch* a, void* stream) {
  if (!a || a->B < 0 || a->B > 65535 || !kind_valid(kind, a->p, a->nF, a->bw, a->n_ex)) return CAVE_E_INVALID;
  switch (kind) {
#ifdef CAVE_PRIMS_DENSE_ONLY
    case K_DENSE_W2: return prim_launch<K_DENSE_W2>(*a, (hipStream_t)stream);
    case K_DENSE_W4: return prim_launch<K_DENSE_W4>(*a, (hipStream_t)stream);
    case K_DENSE_MODEL_W1: return prim_launch<K_DENSE_MODEL_W1>(*a, (hipStream_t)stream);
    case K_DENSE_MODEL_W2: return prim_launch<K_DENSE_MODEL_W2>(*a, (hipStream_t)stream);
    case K_DENSE_MODEL_W4: return prim_launch<K_DENSE_MODEL_W4>(*a, (hipStream_t)stream);
#else
#define CAVE_PRIM_CASE(K) case K: return prim_launch<K>(*a, (hipStream_t)stream);
    CAVE_PRIM_KINDS(CAVE_PRIM_CASE)
#undef CAVE_PRIM_CASE
#endif
  }
  return CAVE_E_INVALID;
}

#ifndef CAVE_PRIMS_DENSE_ONLY
int64_t cave_prims_info(int32_t kind, int32_t what, int32_t p, int32_t nF, int32_t bw) {  // sizes the caller allocates by
  if (!kind_valid(kind, p, nF, bw, 0)) return -1;
  switch (what) {
    case 0: return kind_h_entries(kind, p, bw);
    case 1: return kind_ws_entries(kind, p, bw);
    case 2: return kind_lds_bytes(kind, p, nF, bw);
  }
  return -1;
}
#endif

}  // extern "C"
