// simt_vrp_dp.cpp — SIMT emulation of the CVRP dynamic-program kernels (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_tsp_hk.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin,
// else the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: vrp_dp_block (vrp_dp.h),
// 256-thread workgroups striding over the instances exactly as k_vrp_dp.hip launches them, behind the argument checks
// of the C ABI entry point, on an exact-size LDS block that is poisoned before every workgroup and, in the workspace
// tiers, on the caller's workspace (an exact-size heap block of the size the caller states).
//
// Built two ways (tests/emul_vrp_dp_lib.py): a shared library for ctypes, and -- with VRP_DP_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input, every output and the workspace in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/cave_hip.h"
#include "../../cave_amd/csrc/cone_common.h"
#include "../../cave_amd/csrc/vrp_dp.h"

using namespace cave;

namespace {

struct Lds {  // exact-size, 16-byte aligned heap block standing in for the workgroup's LDS (as simt_tsp_hk.cpp)
  std::vector<unsigned char> raw;
  unsigned char* p;
  size_t len;
  explicit Lds(size_t n) : raw(n + 16), len(n) {
    const size_t off = (16 - ((uintptr_t)raw.data() & 15)) & 15;
    raw.resize(off + n);  // no slack behind the arena (shrinking keeps the buffer where it is)
    p = raw.data() + off;
  }
  void poison() { memset(p, 0xFF, len); }  // LDS is not cleared between workgroups
};

}  // namespace

extern "C" {

int64_t cave_simt_vrp_dp_slot_bytes(int64_t n, int64_t K) { return vrp_dp_valid(n, K) ? vrp_dp_slot_bytes(n, K) : (int64_t)CAVE_E_INVALID; }

int64_t cave_simt_vrp_dp_workspace_bytes(int64_t n, int64_t K, int64_t N) {
  if (!vrp_dp_valid(n, K) || N < 0) return CAVE_E_INVALID;
  return vrp_dp_slot_bytes(n, K) * (N < kTspHkDefaultSlots ? N : kTspHkDefaultSlots);
}

int64_t cave_simt_vrp_dp_lds_bytes(int64_t n, int64_t K) { return vrp_dp_valid(n, K) ? (int64_t)vrp_dp_lds_bytes(n, K) : (int64_t)CAVE_E_INVALID; }

int32_t cave_simt_vrp_dp_tier(int64_t n, int64_t K) { return vrp_dp_valid(n, K) ? vrp_dp_tier(n, K) : CAVE_E_INVALID; }

// cave_hip_vrp_dp_solve (cave_hip.hip), its checks and its launch shape; `grid_out`: workgroups launched
int32_t cave_simt_vrp_dp_solve(const float* costs, const float* eval_costs, const float* demands, double capacity, int64_t K,
                               int64_t N, int64_t n, float* sol, double* obj, double* eval, int32_t* routes, int32_t* status,
                               void* workspace, int64_t workspace_bytes, uint64_t seed, int32_t* grid_out) {
  if (!vrp_dp_valid(n, K)) return CAVE_E_INVALID;
  if (eval && !eval_costs) return CAVE_E_INVALID;
  if (N < 0) return CAVE_E_INVALID;
  if (!(capacity > 0.0 && capacity <= 1.7976931348623157e308)) return CAVE_E_INVALID;
  if (N == 0) return CAVE_OK;
  const int64_t slot = vrp_dp_slot_bytes(n, K);
  if (slot > 0 && (!workspace || workspace_bytes < slot || ((uintptr_t)workspace & 7u) != 0u)) return CAVE_E_INVALID;
  if (!costs || !demands) return CAVE_E_INVALID;
  int64_t grid = slot > 0 ? workspace_bytes / slot : kTspHkLdsGrid;
  if (grid > N) grid = N;
  if (grid > ((int64_t)1 << 20)) grid = (int64_t)1 << 20;
  if (grid_out) *grid_out = (int32_t)grid;
  VrpDpParams P;
  P.costs = costs; P.eval_costs = eval_costs; P.demands = demands; P.capacity = capacity; P.N = N;
  P.n = (int32_t)n; P.d = (int32_t)tsp_hk_edges(n); P.K = (int32_t)K;
  P.sol = sol; P.obj = obj; P.eval = eval; P.routes = routes; P.status = status;
  P.ws = slot > 0 ? static_cast<double*>(workspace) : nullptr; P.slot_doubles = slot / 8;
  Lds mem(vrp_dp_lds_bytes(n, K));
  const int tier = vrp_dp_tier(n, K);
  for (int64_t g = 0; g < grid; ++g) {
    mem.poison();
    simt::run_block(kVrpDpThreads, (unsigned)g, (unsigned)grid, [&]() {  // the bodies of the three kernels
      if (tier == 0) vrp_dp_block<0>(P, mem.p);
      else if (tier == 1) vrp_dp_block<1>(P, mem.p);
      else vrp_dp_block<2>(P, mem.p);
    }, seed ? seed + (uint64_t)g : 0);
  }
  return CAVE_OK;
}

}  // extern "C"

#ifdef VRP_DP_MAIN
// prog IN OUT.  IN: int64 ncases, then per case int64 {N, n, K, flags, seed, workspace_bytes}, fp64 capacity, demands [n-1]
// fp32, costs [N d] fp32 (+ eval_costs [N d] when flags & 1).  flags: 1 eval_costs, 2 sol, 4 obj, 8 eval, 16 routes,
// 32 status, 64 hand over a null demands pointer.  workspace_bytes: the heap block handed over as the workspace,
// 0xFF-filled (0: none).  OUT: per case int32 rc, then (rc == 0) the requested outputs in that order.
template <class T>
static T* exact(size_t n) { return n ? (T*)malloc(n * sizeof(T)) : nullptr; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int64_t ncases = 0;
  if (fread(&ncases, 8, 1, in) != 1) return 2;
  for (int64_t c = 0; c < ncases; ++c) {
    int64_t hdr[6];
    double cap = 0.0;
    if (fread(hdr, 8, 6, in) != 6 || fread(&cap, 8, 1, in) != 1) return 2;
    const int64_t N = hdr[0], n = hdr[1], K = hdr[2], flags = hdr[3], wsb = hdr[5];
    const size_t m = (size_t)(n - 1), nd = (size_t)(N * (n * (n - 1) / 2)), nr = (size_t)(N * (n + K));
    float* dem = exact<float>(m);
    float* costs = exact<float>(nd);
    float* ev = (flags & 1) ? exact<float>(nd) : nullptr;
    if (m && fread(dem, 4, m, in) != m) return 2;
    if (nd && fread(costs, 4, nd, in) != nd) return 2;
    if (ev && fread(ev, 4, nd, in) != nd) return 2;
    float* sol = (flags & 2) ? exact<float>(nd) : nullptr;
    double* obj = (flags & 4) ? exact<double>((size_t)N) : nullptr;
    double* evo = (flags & 8) ? exact<double>((size_t)N) : nullptr;
    int32_t* routes = (flags & 16) ? exact<int32_t>(nr) : nullptr;
    int32_t* st = (flags & 32) ? exact<int32_t>((size_t)N) : nullptr;
    unsigned char* ws = exact<unsigned char>((size_t)wsb);
    if (ws) memset(ws, 0xFF, (size_t)wsb);
    const int32_t rc = cave_simt_vrp_dp_solve(costs, ev, (flags & 64) ? nullptr : dem, cap, K, N, n, sol, obj, evo, routes, st, ws,
                                              wsb, (uint64_t)hdr[4], nullptr);
    fwrite(&rc, 4, 1, out);
    if (rc == CAVE_OK) {
      if (sol) fwrite(sol, 4, nd, out);
      if (obj) fwrite(obj, 8, (size_t)N, out);
      if (evo) fwrite(evo, 8, (size_t)N, out);
      if (routes) fwrite(routes, 4, nr, out);
      if (st) fwrite(st, 4, (size_t)N, out);
    }
    free(dem); free(costs); free(ev); free(sol); free(obj); free(evo); free(routes); free(st); free(ws);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  puts("vrp-dp-ok");
  return 0;
}
#endif
