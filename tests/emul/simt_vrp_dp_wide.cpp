// simt_vrp_dp_wide.cpp — SIMT emulation of the wide CVRP tier (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_vrp_dp.cpp and simt_tsp_hk_wide.cpp (same shim, same conventions: host pointers, a schedule
// seed -- 0 = round robin, else the lanes between two rendezvous run in a seeded random order).  It holds ONE code path:
// the list kernel's tsp_hk_wide_list_block, then vrp_dp_wide_block<M> (vrp_dp_wide.h), 512-thread workgroups striding
// over the instances exactly as k_vrp_dp_wide.hip launches them, behind the argument checks of the C ABI entry point
// (vrp_dp_wide_plan, the function the library calls), on an exact-size LDS block that is poisoned before every workgroup
// and on the caller's workspace (an exact-size heap block of the size the caller states: the header region, then the slots).
//
// Built two ways (tests/emul_vrp_dp_wide_lib.py): a shared library for ctypes, and -- with VRP_DP_WIDE_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input, every output and the workspace in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include "../../cave_amd/csrc/vrp_dp_wide.h"
#include "simt_solver.h"

using namespace cave;

namespace {

void block(const VrpDpWideParams& P, unsigned char* lds) {  // the switch of launch_vrp_dp_wide
  switch (P.n - 1) {
    case 12: vrp_dp_wide_block<12>(P, lds); break;
    case 13: vrp_dp_wide_block<13>(P, lds); break;
    case 14: vrp_dp_wide_block<14>(P, lds); break;
    case 15: vrp_dp_wide_block<15>(P, lds); break;
    case 16: vrp_dp_wide_block<16>(P, lds); break;
    case 17: vrp_dp_wide_block<17>(P, lds); break;
    case 18: vrp_dp_wide_block<18>(P, lds); break;
    case 19: vrp_dp_wide_block<19>(P, lds); break;
    default: abort();
  }
}

}  // namespace

extern "C" {

int64_t cave_simt_vrp_dp_wide_slot_bytes(int64_t n, int64_t K) {
  return vrp_dp_wide_valid(n, K) ? vrp_dp_wide_slot_bytes(n, K) : (int64_t)CAVE_E_INVALID;
}

int64_t cave_simt_vrp_dp_wide_workspace_bytes(int64_t n, int64_t K, int64_t N) {
  if (!vrp_dp_wide_valid(n, K) || N < 0) return CAVE_E_INVALID;
  return solver_workspace_bytes(tsp_hk_wide_header_bytes(n), vrp_dp_wide_slot_bytes(n, K), N, vrp_dp_wide_default_slots(n, K));
}

int64_t cave_simt_vrp_dp_wide_header_bytes(int64_t n, int64_t K) {
  return vrp_dp_wide_valid(n, K) ? tsp_hk_wide_header_bytes(n) : (int64_t)CAVE_E_INVALID;
}

int64_t cave_simt_vrp_dp_wide_lds_bytes(int64_t n, int64_t K) {
  return vrp_dp_wide_valid(n, K) ? (int64_t)vrp_dp_wide_lds_bytes(n) : (int64_t)CAVE_E_INVALID;
}

// cave_hip_vrp_dp_wide_solve (cave_hip.hip), its checks and its launch shape; `grid_out`: workgroups launched
int32_t cave_simt_vrp_dp_wide_solve(const float* costs, const float* eval_costs, const float* demands, double capacity, int64_t K,
                                    int64_t N, int64_t n, float* sol, double* obj, double* eval, int32_t* routes, int32_t* status,
                                    void* workspace, int64_t workspace_bytes, uint64_t seed, int32_t* grid_out) {
  VrpDpWideParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = vrp_dp_wide_plan(costs, eval_costs, demands, capacity, K, N, n, sol, obj, eval, routes, status, workspace,
                                      workspace_bytes, &P, &grid, msg);
  if (rc != CAVE_OK || grid == 0) return rc;
  if (grid_out) *grid_out = (int32_t)grid;
  const int m = (int)n - 1;  // the list kernel
  const unsigned total = 1u << m, per = (unsigned)kTspHkWideListThreads;
  simt_solver::run_grid((int)per, (total + per - 1u) / per, kTspHkWideListLds, seed ? seed + 977u : 0,
                        [&](unsigned char* lds) { tsp_hk_wide_list_block(P.list, m, lds); });
  simt_solver::run_grid(kVrpDpWideThreads, grid, vrp_dp_wide_lds_bytes(n), seed, [&](unsigned char* lds) { block(P, lds); });
  return CAVE_OK;
}

}  // extern "C"

#ifdef VRP_DP_WIDE_MAIN
// prog IN OUT (simt_solver.h): the case file of simt_vrp_dp.cpp.  Per case int64 {N, n, K, flags, seed, workspace_bytes},
// fp64 capacity, demands [n-1] fp32, costs [N d] fp32 (+ eval_costs [N d] when flags & 1).  flags: 1 eval_costs, 2 sol,
// 4 obj, 8 eval, 16 routes, 32 status, 64 hand over a null demands pointer.  workspace_bytes: the heap block handed over
// as the workspace, 0xFF-filled (0: none).
int main(int argc, char** argv) {
  return simt_solver::case_main(argc, argv, "vrp-dp-wide-ok", [](simt_solver::Case& k) {
    int64_t hdr[6];
    if (!k.header(hdr, 6)) return false;
    const int64_t N = hdr[0], n = hdr[1], K = hdr[2], flags = hdr[3], wsb = hdr[5];
    const size_t nd = (size_t)(N * (n * (n - 1) / 2)), nr = (size_t)(N * (n + K));
    double* cap = k.input<double>(1);
    float* dem = k.input<float>((size_t)(n - 1));
    float* costs = k.input<float>(nd);
    float* ev = k.input<float>(nd, flags & 1);
    if (!k.good) return false;
    float* sol = k.output<float>(flags & 2, nd);
    double* obj = k.output<double>(flags & 4, (size_t)N);
    double* evo = k.output<double>(flags & 8, (size_t)N);
    int32_t* routes = k.output<int32_t>(flags & 16, nr);
    int32_t* st = k.output<int32_t>(flags & 32, (size_t)N);
    unsigned char* ws = k.workspace(wsb);
    return k.done(cave_simt_vrp_dp_wide_solve(costs, ev, (flags & 64) ? nullptr : dem, *cap, K, N, n, sol, obj, evo, routes, st, ws, wsb,
                                         (uint64_t)hdr[4], nullptr));
  });
}
#endif
