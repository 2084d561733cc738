// k_tight_cones.hip -- the tight-cone kernels (tight_cones.h): one 64-lane wave per instance, four instances per
// workgroup, no LDS and no barrier (the waves of a workgroup share nothing).  The count pass and the fill pass are two
// kernels around the same per-instance routines.
#include "tight_cones.h"

namespace cave {

template <bool FILL>
__global__ __launch_bounds__(64 * kTightWaves) void tight_cones_kernel(TightConesParams P) {
  const int64_t b = (int64_t)blockIdx.x * (int64_t)kTightWaves + (int64_t)(threadIdx.x >> 6);
  if (b >= P.N) return;
  if (FILL) tight_cones_fill_instance(P, b, (int)(threadIdx.x & 63u));
  else tight_cones_count_instance(P, b, (int)(threadIdx.x & 63u));
}

hipError_t launch_tight_cones(bool fill, unsigned grid, hipStream_t stream, const TightConesParams& P) {
  if (fill) hipLaunchKernelGGL(tight_cones_kernel<true>, dim3(grid), dim3(64u * kTightWaves), 0, stream, P);
  else hipLaunchKernelGGL(tight_cones_kernel<false>, dim3(grid), dim3(64u * kTightWaves), 0, stream, P);
  return hipGetLastError();
}

}  // namespace cave
