// k_tsp_hk.hip -- the Held-Karp kernels (tsp_hk.h): one 256-thread workgroup per instance, workgroups striding over the
// batch.  Two kernels, one per tier: the table in LDS (n <= 12; at n = 12 92 KB, one workgroup per compute unit) or in
// the workgroup's slot of the global workspace (n = 13, 14; LDS holds D, the list and the small arrays only).
#include "tsp_hk.h"

namespace cave {

__global__ __launch_bounds__(kTspHkThreads) void tsp_hk_lds_kernel(TspHkParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  tsp_hk_block<false>(P, smem);
}

__global__ __launch_bounds__(kTspHkThreads) void tsp_hk_ws_kernel(TspHkParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  tsp_hk_block<true>(P, smem);
}

hipError_t launch_tsp_hk(unsigned grid, hipStream_t stream, const TspHkParams& P) {
  const uint32_t lds = tsp_hk_lds_bytes(P.n);
  if (P.ws) {
    hipLaunchKernelGGL(tsp_hk_ws_kernel, dim3(grid), dim3((unsigned)kTspHkThreads), (size_t)lds, stream, P);
    return hipGetLastError();
  }
  if (lds > 48u * 1024u) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(tsp_hk_lds_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(tsp_hk_lds_kernel, dim3(grid), dim3((unsigned)kTspHkThreads), (size_t)lds, stream, P);
  return hipGetLastError();
}

}  // namespace cave
