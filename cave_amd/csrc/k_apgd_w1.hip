// k_apgd_w1.hip -- the APGD projector (apgd.h) on one wave per instance: the dense and the sparse loader around one core.
#include "apgd.h"

namespace cave {

template <bool SPARSE>
__global__ __launch_bounds__(64) void apgd_w1_kernel(ApgdParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  apgd_block<1, SPARSE>(P, smem);
}

template <bool SPARSE>
static hipError_t launch(unsigned grid, hipStream_t stream, const ApgdParams& P) {
  const int lds = (int)P.L.bytes;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(apgd_w1_kernel<SPARSE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(apgd_w1_kernel<SPARSE>, dim3(grid), dim3(64u), (size_t)lds, stream, P);
  return hipGetLastError();
}

hipError_t launch_apgd_w1(bool sparse, unsigned grid, hipStream_t stream, const ApgdParams& P) {
  return sparse ? launch<true>(grid, stream, P) : launch<false>(grid, stream, P);
}

}  // namespace cave
