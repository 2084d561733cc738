// k_vrp_dp.hip -- the CVRP dynamic program (vrp_dp.h): one 256-thread workgroup per instance, workgroups striding over
// the batch.  Three kernels, one per tier: both tables in LDS; the Held-Karp table in the workgroup's slot of the global
// workspace and the partition tables in LDS; both in the slot.
#include "vrp_dp.h"

namespace cave {

template <int kTier>
__global__ __launch_bounds__(kVrpDpThreads) void vrp_dp_kernel(VrpDpParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  vrp_dp_block<kTier>(P, smem);
}

template <int kTier>
static hipError_t launch_tier(unsigned grid, uint32_t lds, hipStream_t stream, const VrpDpParams& P) {
  if (lds > 48u * 1024u) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(vrp_dp_kernel<kTier>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(vrp_dp_kernel<kTier>, dim3(grid), dim3((unsigned)kVrpDpThreads), (size_t)lds, stream, P);
  return hipGetLastError();
}

hipError_t launch_vrp_dp(unsigned grid, hipStream_t stream, const VrpDpParams& P) {
  const uint32_t lds = vrp_dp_lds_bytes(P.n, P.K);
  switch (vrp_dp_tier(P.n, P.K)) {
    case 0: return launch_tier<0>(grid, lds, stream, P);
    case 1: return launch_tier<1>(grid, lds, stream, P);
    default: return launch_tier<2>(grid, lds, stream, P);
  }
}

}  // namespace cave
