// k_sp_grid.hip -- the grid shortest-path kernel (sp_grid.h): one 64-lane wave per instance, up to four instances per
// workgroup, no barrier (the waves of a workgroup share nothing but the LDS allocation).  64 VGPRs: the LDS, not the
// registers, sets the residency (30x30: 7.7 KB per wave, five four-wave workgroups per compute unit).
#include "sp_grid.h"

namespace cave {

__global__ __launch_bounds__(256) void sp_grid_kernel(SpGridParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t wv = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * (int64_t)(blockDim.x >> 6) + (int64_t)wv;
  if (b >= P.N) return;
  sp_grid_instance(P, smem + wv * P.wave_lds, b, (int)(threadIdx.x & 63u));
}

hipError_t launch_sp_grid(unsigned grid, int waves, hipStream_t stream, const SpGridParams& P) {
  const uint32_t lds = (uint32_t)waves * P.wave_lds;
  if (lds > 48u * 1024u) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sp_grid_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(sp_grid_kernel, dim3(grid), dim3(64u * (unsigned)waves), (size_t)lds, stream, P);
  return hipGetLastError();
}

}  // namespace cave
