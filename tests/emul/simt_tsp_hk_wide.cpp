// simt_tsp_hk_wide.cpp — SIMT emulation of the wide Held-Karp tier (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_tsp_hk.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin,
// else the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: the list kernel's
// tsp_hk_wide_list_block, then tsp_hk_wide_block<M> (tsp_hk_wide.h), 512-thread workgroups striding over the instances
// exactly as k_tsp_hk_wide.hip launches them, behind the argument checks of the C ABI entry point, on an exact-size LDS
// block that is poisoned before every workgroup and on the caller's workspace (an exact-size heap block of the size the
// caller states: the header region, then the slots).
//
// Built two ways (tests/emul_tsp_hk_wide_lib.py): a shared library for ctypes, and -- with TSP_HK_WIDE_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input, every output and the workspace in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/cave_hip.h"
#include "../../cave_amd/csrc/cone_common.h"
#include "../../cave_amd/csrc/tsp_hk_wide.h"

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

template <int M>
void block_m(const TspHkWideParams& P, unsigned char* lds) { tsp_hk_wide_block<M>(P, lds); }

void block(const TspHkWideParams& P, unsigned char* lds) {  // the switch of launch_tsp_hk_wide
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
  const int64_t slots = tsp_hk_wide_default_slots(n);
  return tsp_hk_wide_header_bytes(n) + tsp_hk_wide_slot_bytes(n) * (N < slots ? N : slots);
}

int64_t cave_simt_tsp_hk_wide_header_bytes(int64_t n) {
  return tsp_hk_wide_valid_n(n) ? tsp_hk_wide_header_bytes(n) : (int64_t)CAVE_E_INVALID;
}

int64_t cave_simt_tsp_hk_wide_lds_bytes(int64_t n) {
  return tsp_hk_wide_valid_n(n) ? (int64_t)tsp_hk_wide_lds_bytes(n) : (int64_t)CAVE_E_INVALID;
}

// cave_hip_tsp_hk_wide_solve (cave_hip.hip), its checks and its launch shape; `grid_out`: workgroups launched
int32_t cave_simt_tsp_hk_wide_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                                    double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                                    uint64_t seed, int32_t* grid_out) {
  if (!tsp_hk_wide_valid_n(n)) return CAVE_E_INVALID;
  if (eval && !eval_costs) return CAVE_E_INVALID;
  if (N < 0) return CAVE_E_INVALID;
  if (N == 0) return CAVE_OK;
  const int64_t slot = tsp_hk_wide_slot_bytes(n), header = tsp_hk_wide_header_bytes(n);
  if (!workspace || workspace_bytes < header + slot || ((uintptr_t)workspace & 7u) != 0u) return CAVE_E_INVALID;
  if (!costs) return CAVE_E_INVALID;
  int64_t grid = (workspace_bytes - header) / slot;
  if (grid > N) grid = N;
  if (grid > ((int64_t)1 << 20)) grid = (int64_t)1 << 20;
  if (grid_out) *grid_out = (int32_t)grid;
  TspHkWideParams P;
  P.costs = costs; P.eval_costs = eval_costs; P.N = N; P.n = (int32_t)n; P.d = (int32_t)tsp_hk_wide_edges(n);
  P.sol = sol; P.obj = obj; P.eval = eval; P.tour = tour; P.status = status;
  P.list = static_cast<uint32_t*>(workspace);
  P.ws = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + header); P.slot_doubles = slot / 8;
  {  // the list kernel
    const int m = (int)n - 1;
    const unsigned total = 1u << m, per = (unsigned)kTspHkWideListThreads, lgrid = (total + per - 1u) / per;
    Lds lmem(kTspHkWideListLds);
    for (unsigned g = 0; g < lgrid; ++g) {
      lmem.poison();
      simt::run_block((int)per, g, lgrid, [&]() { tsp_hk_wide_list_block(P.list, m, lmem.p); }, seed ? seed + 977u + g : 0);
    }
  }
  Lds mem(tsp_hk_wide_lds_bytes(n));
  for (int64_t g = 0; g < grid; ++g) {
    mem.poison();
    simt::run_block(kTspHkWideThreads, (unsigned)g, (unsigned)grid, [&]() { block(P, mem.p); }, seed ? seed + (uint64_t)g : 0);
  }
  return CAVE_OK;
}

}  // extern "C"

#ifdef TSP_HK_WIDE_MAIN
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
    const int32_t rc = cave_simt_tsp_hk_wide_solve(costs, ev, N, n, sol, obj, evo, tour, st, ws, wsb, (uint64_t)hdr[3], nullptr);
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
  puts("tsp-hk-wide-ok");
  return 0;
}
#endif
