// simt_solver.h — what the emulation drivers of the exact solvers share (simt_sp_grid.cpp, simt_tsp_hk.cpp,
// simt_tsp_hk_wide.cpp, simt_vrp_dp.cpp; TEST INFRASTRUCTURE ONLY): the heap block that stands in for a workgroup's LDS,
// the loop over the workgroups of a launch, and the case files of the stand-alone sanitizer programs.  Included after
// the shim <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../include/cave_hip.h"

namespace simt_solver {

struct Lds {  // exact-size, 16-byte aligned heap block standing in for the workgroup's LDS: ASan sees overruns
  std::vector<unsigned char> raw;
  unsigned char* p;
  size_t len;
  explicit Lds(size_t n) : raw(n + 16), len(n) {
    const size_t off = (16 - ((uintptr_t)raw.data() & 15)) & 15;
    raw.resize(off + n);  // no slack behind the arena (shrinking keeps the buffer where it is)
    p = raw.data() + off;
  }
  void poison() { memset(p, 0xFF, len); }  // LDS is not cleared between workgroups: NaN as a float, 255 as a byte
};

// A launch: `grid` workgroups of `threads` threads one after the other, each on a freshly poisoned LDS block of
// lds_bytes; body(lds) is the kernel's body.  seed: 0 = round robin, else workgroup g runs under schedule seed + g.
template <class F>
void run_grid(int threads, int64_t grid, size_t lds_bytes, uint64_t seed, F body) {
  Lds mem(lds_bytes);
  for (int64_t g = 0; g < grid; ++g) {
    mem.poison();
    simt::run_block(threads, (unsigned)g, (unsigned)grid, [&]() { body(mem.p); }, seed ? seed + (uint64_t)g : 0);
  }
}

// One case of a case file (prog IN OUT; IN: int64 ncases, then per case a header of int64s and the input arrays; OUT: per
// case int32 rc, then -- rc == 0 -- the requested outputs in the order they were asked for).  Every array is a heap
// block of its exact size.
struct Case {
  FILE *in, *out;
  std::vector<void*> blocks;
  std::vector<std::pair<void*, size_t>> outs;
  bool good = true;

  template <class T>
  T* block(size_t n) {
    T* p = n ? (T*)malloc(n * sizeof(T)) : nullptr;
    if (p) blocks.push_back(p);
    return p;
  }
  bool header(int64_t* h, size_t n) { return good = good && fread(h, 8, n, in) == n; }
  template <class T>
  T* input(size_t n, bool present = true) {
    T* p = present ? block<T>(n) : nullptr;
    if (p && fread(p, sizeof(T), n, in) != n) good = false;
    return p;
  }
  template <class T>
  T* output(bool wanted, size_t n) {
    T* p = wanted ? block<T>(n) : nullptr;
    if (p) outs.push_back({p, n * sizeof(T)});
    return p;
  }
  unsigned char* workspace(int64_t bytes) {  // 0xFF-filled (0: none)
    unsigned char* p = block<unsigned char>((size_t)bytes);
    if (p) memset(p, 0xFF, (size_t)bytes);
    return p;
  }
  bool done(int32_t rc) {
    fwrite(&rc, 4, 1, out);
    if (rc == CAVE_OK)
      for (auto& o : outs) fwrite(o.first, 1, o.second, out);
    for (void* p : blocks) free(p);
    return good;
  }
};

// main of a stand-alone program: one(Case&) reads, runs and finishes (done) one case; `word` is printed after the last
template <class F>
int case_main(int argc, char** argv, const char* word, F one) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int64_t ncases = 0;
  if (fread(&ncases, 8, 1, in) != 1) return 2;
  for (int64_t c = 0; c < ncases; ++c) {
    Case k{in, out};
    if (!one(k)) return 2;
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  puts(word);
  return 0;
}

// One case of the two Held-Karp programs: int64 {N, n, flags, seed, workspace_bytes} + costs [N d] fp32 (+ eval_costs
// [N d] when flags & 1).  flags: 1 eval_costs, 2 sol, 4 obj, 8 eval, 16 tour, 32 status.  workspace_bytes: the heap block
// handed over as the workspace, 0xFF-filled (0: none).  solve: cave_simt_tsp_hk_solve or cave_simt_tsp_hk_wide_solve.
template <class Solve>
bool tsp_case(Case& k, Solve solve) {
  int64_t hdr[5];
  if (!k.header(hdr, 5)) return false;
  const int64_t N = hdr[0], n = hdr[1], flags = hdr[2], wsb = hdr[4];
  const size_t nd = (size_t)(N * (n * (n - 1) / 2)), nn = (size_t)(N * n);
  float* costs = k.input<float>(nd);
  float* ev = k.input<float>(nd, flags & 1);
  if (!k.good) return false;
  float* sol = k.output<float>(flags & 2, nd);
  double* obj = k.output<double>(flags & 4, (size_t)N);
  double* evo = k.output<double>(flags & 8, (size_t)N);
  int32_t* tour = k.output<int32_t>(flags & 16, nn);
  int32_t* st = k.output<int32_t>(flags & 32, (size_t)N);
  unsigned char* ws = k.workspace(wsb);
  return k.done(solve(costs, ev, N, n, sol, obj, evo, tour, st, ws, wsb, (uint64_t)hdr[3], nullptr));
}

}  // namespace simt_solver
