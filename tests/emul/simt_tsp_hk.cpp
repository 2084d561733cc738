// simt_tsp_hk.cpp — SIMT emulation of the Held-Karp kernels (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_sp_grid.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin,
// else the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: tsp_hk_block (tsp_hk.h),
// 256-thread workgroups striding over the instances exactly as k_tsp_hk.hip launches them, behind the argument checks
// of the C ABI entry point (tsp_hk_plan, the function the library calls), on an exact-size LDS block that is poisoned
// before every workgroup and, in the global tier, on the caller's workspace (an exact-size heap block of the size the
// caller states).
//
// Built two ways (tests/emul_tsp_hk_lib.py): a shared library for ctypes, and -- with TSP_HK_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input, every output and the workspace in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include "../../cave_amd/csrc/tsp_hk.h"
#include "simt_solver.h"

using namespace cave;

extern "C" {

int64_t cave_simt_tsp_hk_slot_bytes(int64_t n) { return tsp_hk_valid_n(n) ? tsp_hk_slot_bytes(n) : (int64_t)CAVE_E_INVALID; }

int64_t cave_simt_tsp_hk_workspace_bytes(int64_t n, int64_t N) {
  if (!tsp_hk_valid_n(n) || N < 0) return CAVE_E_INVALID;
  return solver_workspace_bytes(0, tsp_hk_slot_bytes(n), N, kTspHkDefaultSlots);
}

int64_t cave_simt_tsp_hk_lds_bytes(int64_t n) { return tsp_hk_valid_n(n) ? (int64_t)tsp_hk_lds_bytes(n) : (int64_t)CAVE_E_INVALID; }

// cave_hip_tsp_hk_solve (cave_hip.hip): its checks and its launch shape; `grid_out`: workgroups launched
int32_t cave_simt_tsp_hk_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                               double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                               uint64_t seed, int32_t* grid_out) {
  TspHkParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = tsp_hk_plan(costs, eval_costs, N, n, sol, obj, eval, tour, status, workspace, workspace_bytes, &P, &grid, msg);
  if (rc != CAVE_OK || grid == 0) return rc;
  if (grid_out) *grid_out = (int32_t)grid;
  simt_solver::run_grid(kTspHkThreads, grid, tsp_hk_lds_bytes(n), seed, [&](unsigned char* lds) {  // the bodies of the two kernels
    if (P.ws) tsp_hk_block<true>(P, lds);
    else tsp_hk_block<false>(P, lds);
  });
  return CAVE_OK;
}

}  // extern "C"

#ifdef TSP_HK_MAIN
// prog IN OUT: the Held-Karp case file of simt_solver.h (tsp_case)
int main(int argc, char** argv) {
  return simt_solver::case_main(argc, argv, "tsp-hk-ok", [](simt_solver::Case& k) { return simt_solver::tsp_case(k, cave_simt_tsp_hk_solve); });
}
#endif
