// simt_sp_grid.cpp — SIMT emulation of the grid shortest-path kernel (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_abi.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin, else
// the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: sp_grid_instance (sp_grid.h),
// one 64-lane wave per instance in workgroups of sp_grid_waves() waves exactly as k_sp_grid.hip launches it, behind the
// argument checks of the C ABI entry point (sp_grid_plan, the function the library calls), on an exact-size LDS block that is poisoned before every workgroup.
//
// Built two ways (tests/emul_sp_grid_lib.py): a shared library for ctypes, and -- with SP_GRID_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input and output in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include "../../cave_amd/csrc/sp_grid.h"
#include "simt_solver.h"

using namespace cave;

extern "C" {

int32_t cave_simt_sp_grid_lds_bytes(int64_t h, int64_t w) {
  const uint32_t lds = sp_grid_wave_lds_bytes(h, w);
  return lds ? (int32_t)lds : CAVE_E_INVALID;
}

// cave_hip_sp_grid_solve (cave_hip.hip), its checks and its launch shape; `waves_out`: waves per workgroup used
int32_t cave_simt_sp_grid_solve(const float* costs, const float* eval_costs, int64_t N, int64_t h, int64_t w, float* sol,
                                double* obj, double* eval, int32_t* status, uint32_t* key, float* val, uint64_t seed,
                                int32_t* waves_out) {
  SpGridParams P;
  int64_t grid;
  int waves;
  char msg[kSolverMsg];
  const int32_t rc = sp_grid_plan(costs, eval_costs, N, h, w, sol, obj, eval, status, key, val, &P, &grid, &waves, msg);
  if (rc != CAVE_OK || grid == 0) return rc;
  if (waves_out) *waves_out = waves;
  simt_solver::run_grid(64 * waves, grid, (size_t)waves * P.wave_lds, seed, [&](unsigned char* lds) {  // the body of sp_grid_kernel
    const uint32_t wv = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * (int64_t)(blockDim.x >> 6) + (int64_t)wv;
    if (b >= P.N) return;
    sp_grid_instance(P, lds + wv * P.wave_lds, b, (int)(threadIdx.x & 63u));
  });
  return CAVE_OK;
}

}  // extern "C"

#ifdef SP_GRID_MAIN
// prog IN OUT (simt_solver.h).  Per case int64 {N, h, w, flags, seed} + costs [N d] fp32 (+ eval_costs [N d] when
// flags & 1).  flags: 1 eval_costs, 2 sol, 4 obj, 8 eval, 16 status, 32 key + val.
int main(int argc, char** argv) {
  return simt_solver::case_main(argc, argv, "sp-grid-ok", [](simt_solver::Case& k) {
    int64_t hdr[5];
    if (!k.header(hdr, 5)) return false;
    const int64_t N = hdr[0], h = hdr[1], w = hdr[2], flags = hdr[3];
    const size_t nd = (size_t)(N * sp_grid_arcs(h, w));
    float* costs = k.input<float>(nd);
    float* ev = k.input<float>(nd, flags & 1);
    if (!k.good) return false;
    float* sol = k.output<float>(flags & 2, nd);
    double* obj = k.output<double>(flags & 4, (size_t)N);
    double* evo = k.output<double>(flags & 8, (size_t)N);
    int32_t* st = k.output<int32_t>(flags & 16, (size_t)N);
    uint32_t* key = k.output<uint32_t>(flags & 32, 5 * nd);
    float* val = k.output<float>(flags & 32, 5 * nd);
    return k.done(cave_simt_sp_grid_solve(costs, ev, N, h, w, sol, obj, evo, st, key, val, (uint64_t)hdr[4], nullptr));
  });
}
#endif
