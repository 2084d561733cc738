// simt_tsp_hk_wide.cpp — SIMT emulation of the wide Held-Karp tier (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_tsp_hk.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin,
// else the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: the list kernel's
// tsp_hk_wide_list_block, then tsp_hk_wide_block<M> (tsp_hk_wide.h), 512-thread workgroups striding over the instances
// exactly as k_tsp_hk_wide.hip launches them, behind the argument checks of the C ABI entry point (tsp_hk_wide_plan, the
// function the library calls), on an exact-size LDS block that is poisoned before every workgroup and on the caller's
// workspace (an exact-size heap block of the size the caller states: the header region, then the slots).
//
// Built two ways (tests/emul_tsp_hk_wide_lib.py): a shared library for ctypes, and -- with TSP_HK_WIDE_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input, every output and the workspace in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include "../../cave_amd/csrc/tsp_hk_wide.h"
#include "simt_solver.h"

using namespace cave;

namespace {

template <int M>
void block_m(const TspHkParams& P, unsigned char* lds) { tsp_hk_wide_block<M>(P, lds); }

void block(const TspHkParams& P, unsigned char* lds) {  // the switch of launch_tsp_hk_wide
  switch (P.n - 1) {
    case 12: block_m<12>(P, lds); break;
    case 13: block_m<13>(P, lds); break;
    case 14: block_m<14>(P, lds); break;
    case 15: block_m<15>(P, lds); break;
    case 16: block_m<16>(P, lds); break;
    case 17: block_m<17>(P, lds); break;
    case 18: block_m<18>(P, lds); break;
    case 19: block_m<19>(P, lds); break;
    default: abort();
  }
}

}  // namespace

extern "C" {

int64_t cave_simt_tsp_hk_wide_slot_bytes(int64_t n) {
  return tsp_hk_wide_valid_n(n) ? tsp_hk_wide_slot_bytes(n) : (int64_t)CAVE_E_INVALID;
}

int64_t cave_simt_tsp_hk_wide_workspace_bytes(int64_t n, int64_t N) {
  if (!tsp_hk_wide_valid_n(n) || N < 0) return CAVE_E_INVALID;
  return solver_workspace_bytes(tsp_hk_wide_header_bytes(n), tsp_hk_wide_slot_bytes(n), N, tsp_hk_wide_default_slots(n));
}

int64_t cave_simt_tsp_hk_wide_header_bytes(int64_t n) {
  return tsp_hk_wide_valid_n(n) ? tsp_hk_wide_header_bytes(n) : (int64_t)CAVE_E_INVALID;
}

int64_t cave_simt_tsp_hk_wide_lds_bytes(int64_t n) {
  return tsp_hk_wide_valid_n(n) ? (int64_t)tsp_hk_wide_lds_bytes(n) : (int64_t)CAVE_E_INVALID;
}

// cave_hip_tsp_hk_wide_solve (cave_hip.hip): its checks and its launch shape; `grid_out`: workgroups launched
int32_t cave_simt_tsp_hk_wide_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                                    double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                                    uint64_t seed, int32_t* grid_out) {
  TspHkParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = tsp_hk_wide_plan(costs, eval_costs, N, n, sol, obj, eval, tour, status, workspace, workspace_bytes, &P, &grid, msg);
  if (rc != CAVE_OK || grid == 0) return rc;
  if (grid_out) *grid_out = (int32_t)grid;
  const int m = (int)n - 1;  // the list kernel
  const unsigned total = 1u << m, per = (unsigned)kTspHkWideListThreads;
  simt_solver::run_grid((int)per, (total + per - 1u) / per, kTspHkWideListLds, seed ? seed + 977u : 0,
                        [&](unsigned char* lds) { tsp_hk_wide_list_block(P.list, m, lds); });
  simt_solver::run_grid(kTspHkWideThreads, grid, tsp_hk_wide_lds_bytes(n), seed, [&](unsigned char* lds) { block(P, lds); });
  return CAVE_OK;
}

}  // extern "C"

#ifdef TSP_HK_WIDE_MAIN
// prog IN OUT: the Held-Karp case file of simt_solver.h (tsp_case)
int main(int argc, char** argv) {
  return simt_solver::case_main(argc, argv, "tsp-hk-wide-ok", [](simt_solver::Case& k) { return simt_solver::tsp_case(k, cave_simt_tsp_hk_wide_solve); });
}
#endif
