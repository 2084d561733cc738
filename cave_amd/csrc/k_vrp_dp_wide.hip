// k_vrp_dp_wide.hip -- the wide CVRP tier (vrp_dp_wide.h), 13 <= n <= 20: the list kernel of the wide Held-Karp tier (the
// popcount-sorted list of the m-bit numbers into the workspace's header region), then the dynamic program, one
// 512-thread workgroup per slot, workgroups striding over the batch; one instantiation per m = n - 1 (phase 1 is
// tsp_hk_wide_sweep<M>).  Both go into the caller's stream, the list first.
#include "vrp_dp_wide.h"

namespace cave {

__global__ __launch_bounds__(kTspHkWideListThreads) void vrp_dp_wide_list_kernel(uint32_t* list, int m) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kTspHkWideListLds];
  tsp_hk_wide_list_block(list, m, smem);
}

template <int M>
__global__ __launch_bounds__(kVrpDpWideThreads) void vrp_dp_wide_kernel(VrpDpWideParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  vrp_dp_wide_block<M>(P, smem);
}

template <int M>
static void launch_m(unsigned grid, size_t lds, hipStream_t stream, const VrpDpWideParams& P) {
  hipLaunchKernelGGL(vrp_dp_wide_kernel<M>, dim3(grid), dim3((unsigned)kVrpDpWideThreads), lds, stream, P);
}

hipError_t launch_vrp_dp_wide(unsigned grid, hipStream_t stream, const VrpDpWideParams& P) {
  const int m = P.n - 1;
  const unsigned total = 1u << m, per = (unsigned)kTspHkWideListThreads;
  hipLaunchKernelGGL(vrp_dp_wide_list_kernel, dim3((total + per - 1u) / per), dim3(per), 0, stream, P.list, m);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t lds = vrp_dp_wide_lds_bytes(P.n);
  switch (m) {
    case 12: launch_m<12>(grid, lds, stream, P); break;
    case 13: launch_m<13>(grid, lds, stream, P); break;
    case 14: launch_m<14>(grid, lds, stream, P); break;
    case 15: launch_m<15>(grid, lds, stream, P); break;
    case 16: launch_m<16>(grid, lds, stream, P); break;
    case 17: launch_m<17>(grid, lds, stream, P); break;
    case 18: launch_m<18>(grid, lds, stream, P); break;
    case 19: launch_m<19>(grid, lds, stream, P); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace cave
