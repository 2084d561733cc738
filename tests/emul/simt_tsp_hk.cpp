// simt_tsp_hk.cpp — SIMT emulation of the Held-Karp kernels (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_sp_grid.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin,
// else the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: tsp_hk_block (tsp_hk.h),
// 256-thread workgroups striding over the instances exactly as k_tsp_hk.hip launches them, behind the argument checks
// of the C ABI entry point, on an exact-size LDS block that is poisoned before every workgroup and, in the global tier,
// on the caller's workspace (an exact-size heap block of the size the caller states).
//
// Built two ways (tests/emul_tsp_hk_lib.py): a shared library for ctypes, and -- with TSP_HK_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input, every output and the workspace in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/cave_hip.h"
#include "../../cave_amd/csrc/cone_common.h"
#include "../../cave_amd/csrc/tsp_hk.h"

using namespace cave;

namespace {

struct Lds {  // exact-size, 16-byte aligned heap block standing in for the workgroup's LDS (as simt_sp_grid.cpp)
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

int64_t cave_simt_tsp_hk_slot_bytes(int64_t n) { return tsp_hk_valid_n(n) ? tsp_hk_slot_bytes(n) : (int64_t)CAVE_E_INVALID; }

int64_t cave_simt_tsp_hk_workspace_bytes(int64_t n, int64_t N) {
  if (!tsp_hk_valid_n(n) || N < 0) return CAVE_E_INVALID;
  return tsp_hk_slot_bytes(n) * (N < kTspHkDefaultSlots ? N : kTspHkDefaultSlots);
}

int64_t cave_simt_tsp_hk_lds_bytes(int64_t n) { return tsp_hk_valid_n(n) ? (int64_t)tsp_hk_lds_bytes(n) : (int64_t)CAVE_E_INVALID; }

// cave_hip_tsp_hk_solve (cave_hip.hip), its checks and its launch shape; `grid_out`: workgroups launched
int32_t cave_simt_tsp_hk_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                               double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                               uint64_t seed, int32_t* grid_out) {
  if (!tsp_hk_valid_n(n)) return CAVE_E_INVALID;
  if (eval && !eval_costs) return CAVE_E_INVALID;
  if (N < 0) return CAVE_E_INVALID;
  if (N == 0) return CAVE_OK;
  const int64_t slot = tsp_hk_slot_bytes(n);
  if (slot > 0 && (!workspace || workspace_bytes < slot || ((uintptr_t)workspace & 7u) != 0u)) return CAVE_E_INVALID;
  if (!costs) return CAVE_E_INVALID;
  int64_t grid = slot > 0 ? workspace_bytes / slot : kTspHkLdsGrid;
  if (grid > N) grid = N;
  if (grid > ((int64_t)1 << 20)) grid = (int64_t)1 << 20;
  if (grid_out) *grid_out = (int32_t)grid;
  TspHkParams P;
  P.costs = costs; P.eval_costs = eval_costs; P.N = N; P.n = (int32_t)n; P.d = (int32_t)tsp_hk_edges(n);
  P.sol = sol; P.obj = obj; P.eval = eval; P.tour = tour; P.status = status;
  P.ws = slot > 0 ? static_cast<double*>(workspace) : nullptr; P.slot_doubles = slot / 8;
  Lds mem(tsp_hk_lds_bytes(n));
  for (int64_t g = 0; g < grid; ++g) {
    mem.poison();
    simt::run_block(kTspHkThreads, (unsigned)g, (unsigned)grid, [&]() {  // the bodies of the two kernels
      if (P.ws) tsp_hk_block<true>(P, mem.p);
      else tsp_hk_block<false>(P, mem.p);
    }, seed ? seed + (uint64_t)g : 0);
  }
  return CAVE_OK;
}

}  // extern "C"

#ifdef TSP_HK_MAIN
// prog IN OUT.  IN: int64 ncases, then per case int64 {N, n, flags, seed, workspace_bytes} + costs [N d] fp32 (+ eval_costs
// [N d] when flags & 1).  flags: 1 eval_costs, 2 sol, 4 obj, 8 eval, 16 tour, 32 status.  workspace_bytes: the heap block
// handed over as the workspace, 0xFF-filled (0: none).  OUT: per case int32 rc, then the requested outputs in that order.
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
    int64_t hdr[5];
    if (fread(hdr, 8, 5, in) != 5) return 2;
    const int64_t N = hdr[0], n = hdr[1], flags = hdr[2], wsb = hdr[4];
    const size_t nd = (size_t)(N * (n * (n - 1) / 2)), nn = (size_t)(N * n);
    float* costs = exact<float>(nd);
    float* ev = (flags & 1) ? exact<float>(nd) : nullptr;
    if (nd && fread(costs, 4, nd, in) != nd) return 2;
    if (ev && fread(ev, 4, nd, in) != nd) return 2;
    float* sol = (flags & 2) ? exact<float>(nd) : nullptr;
    double* obj = (flags & 4) ? exact<double>((size_t)N) : nullptr;
    double* evo = (flags & 8) ? exact<double>((size_t)N) : nullptr;
    int32_t* tour = (flags & 16) ? exact<int32_t>(nn) : nullptr;
    int32_t* st = (flags & 32) ? exact<int32_t>((size_t)N) : nullptr;
    unsigned char* ws = exact<unsigned char>((size_t)wsb);
    if (ws) memset(ws, 0xFF, (size_t)wsb);
    const int32_t rc = cave_simt_tsp_hk_solve(costs, ev, N, n, sol, obj, evo, tour, st, ws, wsb, (uint64_t)hdr[3], nullptr);
    fwrite(&rc, 4, 1, out);
    if (rc == CAVE_OK) {
      if (sol) fwrite(sol, 4, nd, out);
      if (obj) fwrite(obj, 8, (size_t)N, out);
      if (evo) fwrite(evo, 8, (size_t)N, out);
      if (tour) fwrite(tour, 4, nn, out);
      if (st) fwrite(st, 4, (size_t)N, out);
    }
    free(costs); free(ev); free(sol); free(obj); free(evo); free(tour); free(st); free(ws);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  puts("tsp-hk-ok");
  return 0;
}
#endif
