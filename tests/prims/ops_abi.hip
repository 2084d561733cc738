// ops_abi.hip — the operators of the Newton loop as kernels of their own (TEST INFRASTRUCTURE ONLY).
//
// tests/prims/op_entries.h compiled by hipcc for gfx950 with the product's flags: one workgroup per case, the product's
// context types and launch bounds.  A unit of tests/prims/_prims.so (tests/prims/prims_lib.py); never loaded by cave_amd.
#include <hip/hip_runtime.h>

#include "cave_hip.h"
#include "cone_common.h"
#include "cone_core.h"
#include "ctx_wave.h"
#include "ctx_block.h"
#include "prim_entries.h"
#include "op_entries.h"

using namespace cave_ops;

namespace {

int32_t g_where = 0, g_hip = 0;  // where the last refused call stopped (1 case limits, 2 attribute, 3 launch) and HIP's code

template <int OP, int CX, bool PM1>
__global__ __launch_bounds__(cx_threads(CX), CtxInfo<typename OpCtx<CX>::type>::min_waves) void op_kernel(const OpCase* cases) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const OpCase k = cases[blockIdx.x];
  op_body<OP, CX, PM1>(smem, k);
}

// host: the cases as the device sees them (device pointers inside; only their sizes are read here); dev: the same bytes
// in device memory
template <int OP, int CX, bool PM1>
int32_t op_launch(const OpCase* host, const OpCase* dev, int64_t B, hipStream_t stream) {
  uint32_t lds = 0;
  for (int64_t b = 0; b < B; ++b) {
    if (!op_case_valid(OP, PM1, host[b])) { g_where = 1; g_hip = (int32_t)b; return CAVE_E_INVALID; }
    const uint32_t n = op_lds_bytes(OP, PM1, host[b]);
    lds = n > lds ? n : lds;
  }
  if (B == 0) return CAVE_OK;
  (void)hipGetLastError();  // (the caller's runtime may have left one behind, e.g. an event that was not ready)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(op_kernel<OP, CX, PM1>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { g_where = 2; g_hip = (int32_t)e; return CAVE_E_INVALID; }
  hipLaunchKernelGGL((op_kernel<OP, CX, PM1>), dim3((unsigned)B), dim3((unsigned)cx_threads(CX)), lds, stream, dev);
  e = hipGetLastError();
  if (e != hipSuccess) { g_where = 3; g_hip = (int32_t)e; return CAVE_E_INVALID; }
  return CAVE_OK;
}

}  // namespace

extern "C" {

// the launch goes to `stream` and is not waited for
int32_t cave_ops_run(int32_t kind, const OpCase* host, const OpCase* dev, int64_t B, void* stream) {
  if (!host || !dev || B < 0 || B > 65535) return CAVE_E_INVALID;
  switch (kind) {
#define CAVE_OP_CASE(OP, CX, PM1) case op_kind(OP, CX, PM1): return op_launch<OP, CX, PM1>(host, dev, B, (hipStream_t)stream);
    CAVE_OP_KINDS(CAVE_OP_CASE)
#undef CAVE_OP_CASE
  }
  return CAVE_E_INVALID;
}

int32_t cave_ops_last_refusal(int32_t what) { return what ? g_hip : g_where; }
int32_t cave_ops_case_bytes(void) { return (int32_t)sizeof(OpCase); }

}  // extern "C"
