// k_apgd_w4.hip -- the APGD projector (apgd.h) on four waves per instance: the dense and the sparse loader around one core.
#include "apgd.h"

namespace cave {

template <bool SPARSE>
__global__ __launch_bounds__(256) void apgd_w4_kernel(ApgdParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  apgd_block<4, SPARSE>(P, smem);
}

template <bool SPARSE>
static hipError_t launch(unsigned grid, hipStream_t stream, const ApgdParams& P) {
  const int lds = (int)P.L.bytes;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(apgd_w4_kernel<SPARSE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(apgd_w4_kernel<SPARSE>, dim3(grid), dim3(256u), (size_t)lds, stream, P);
  return hipGetLastError();
}

hipError_t launch_apgd_w4(bool sparse, unsigned grid, hipStream_t stream, const ApgdParams& P) {
  return sparse ? launch<true>(grid, stream, P) : launch<false>(grid, stream, P);
}

}  // namespace cave
