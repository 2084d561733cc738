// simt_sp_grid.cpp — SIMT emulation of the grid shortest-path kernel (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_abi.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin, else
// the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: sp_grid_instance (sp_grid.h),
// one 64-lane wave per instance in workgroups of sp_grid_waves() waves exactly as k_sp_grid.hip launches it, behind the
// argument checks of the C ABI entry point, on an exact-size LDS block that is poisoned before every workgroup.
//
// Built two ways (tests/emul_sp_grid_lib.py): a shared library for ctypes, and -- with SP_GRID_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input and output in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/cave_hip.h"
#include "../../cave_amd/csrc/cone_common.h"
#include "../../cave_amd/csrc/wave_prims.h"
#include "../../cave_amd/csrc/sp_grid.h"

using namespace cave;

namespace {

struct Lds {  // exact-size, 16-byte aligned heap block standing in for the workgroup's LDS (as simt_abi.cpp): ASan sees overruns
  std::vector<unsigned char> raw;
  unsigned char* p;
  size_t len;
  explicit Lds(size_t n) : raw(n + 16), len(n) {
    const size_t off = (16 - ((uintptr_t)raw.data() & 15)) & 15;
    raw.resize(off + n);  // no slack behind the arena (shrinking keeps the buffer where it is)
    p = raw.data() + off;
  }
  void poison() { memset(p, 0xFF, len); }  // LDS is not cleared between workgroups: NaN as a float, 255 as a predecessor
};

}  // namespace

extern "C" {

int32_t cave_simt_sp_grid_lds_bytes(int64_t h, int64_t w) {
  const uint32_t lds = sp_grid_wave_lds_bytes(h, w);
  return lds ? (int32_t)lds : CAVE_E_INVALID;
}

// cave_hip_sp_grid_solve (cave_hip.hip), its checks and its launch shape; `waves_out`: waves per workgroup used
int32_t cave_simt_sp_grid_solve(const float* costs, const float* eval_costs, int64_t N, int64_t h, int64_t w, float* sol,
                                double* obj, double* eval, int32_t* status, uint32_t* key, float* val, uint64_t seed,
                                int32_t* waves_out) {
  if (h < 1 || w < 1 || h * w < 2) return CAVE_E_INVALID;
  const uint32_t wave_lds = sp_grid_wave_lds_bytes(h, w);
  if (wave_lds == 0u) return CAVE_E_INVALID;
  const int64_t d = sp_grid_arcs(h, w);
  if ((key == nullptr) != (val == nullptr)) return CAVE_E_INVALID;
  if (key && (d > 65535 || 2 * h * w + d > 65535)) return CAVE_E_INVALID;
  if (eval && !eval_costs) return CAVE_E_INVALID;
  if (N < 0) return CAVE_E_INVALID;
  if (N == 0) return CAVE_OK;
  if (!costs) return CAVE_E_INVALID;
  const int waves = sp_grid_waves(wave_lds);
  if (waves_out) *waves_out = waves;
  const int64_t grid = (N + waves - 1) / waves;
  SpGridParams P;
  P.costs = costs; P.eval_costs = eval_costs; P.N = N; P.h = (int32_t)h; P.w = (int32_t)w; P.d = (int32_t)d;
  P.wave_lds = wave_lds; P.sol = sol; P.obj = obj; P.eval = eval; P.status = status; P.key = key; P.val = val;
  Lds mem((size_t)waves * wave_lds);
  for (int64_t g = 0; g < grid; ++g) {
    mem.poison();
    simt::run_block(64 * waves, (unsigned)g, (unsigned)grid, [&]() {  // the body of sp_grid_kernel
      const uint32_t wv = threadIdx.x >> 6;
      const int64_t b = (int64_t)blockIdx.x * (int64_t)(blockDim.x >> 6) + (int64_t)wv;
      if (b >= P.N) return;
      sp_grid_instance(P, mem.p + wv * P.wave_lds, b, (int)(threadIdx.x & 63u));
    }, seed ? seed + (uint64_t)g : 0);
  }
  return CAVE_OK;
}

}  // extern "C"

#ifdef SP_GRID_MAIN
// prog IN OUT.  IN: int64 ncases, then per case int64 {N, h, w, flags, seed} + costs [N d] fp32 (+ eval_costs [N d] when
// flags & 1).  flags: 1 eval_costs, 2 sol, 4 obj, 8 eval, 16 status, 32 key + val.  OUT: per case int32 rc, then the
// requested outputs in that order.
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
    const int64_t N = hdr[0], h = hdr[1], w = hdr[2], flags = hdr[3];
    const size_t nd = (size_t)(N * sp_grid_arcs(h, w));
    float* costs = exact<float>(nd);
    float* ev = (flags & 1) ? exact<float>(nd) : nullptr;
    if (nd && fread(costs, 4, nd, in) != nd) return 2;
    if (ev && fread(ev, 4, nd, in) != nd) return 2;
    float* sol = (flags & 2) ? exact<float>(nd) : nullptr;
    double* obj = (flags & 4) ? exact<double>((size_t)N) : nullptr;
    double* evo = (flags & 8) ? exact<double>((size_t)N) : nullptr;
    int32_t* st = (flags & 16) ? exact<int32_t>((size_t)N) : nullptr;
    uint32_t* key = (flags & 32) ? exact<uint32_t>(5 * nd) : nullptr;
    float* val = (flags & 32) ? exact<float>(5 * nd) : nullptr;
    const int32_t rc = cave_simt_sp_grid_solve(costs, ev, N, h, w, sol, obj, evo, st, key, val, (uint64_t)hdr[4], nullptr);
    fwrite(&rc, 4, 1, out);
    if (rc == CAVE_OK) {
      if (sol) fwrite(sol, 4, nd, out);
      if (obj) fwrite(obj, 8, (size_t)N, out);
      if (evo) fwrite(evo, 8, (size_t)N, out);
      if (st) fwrite(st, 4, (size_t)N, out);
      if (key) { fwrite(key, 4, 5 * nd, out); fwrite(val, 4, 5 * nd, out); }
    }
    free(costs); free(ev); free(sol); free(obj); free(evo); free(st); free(key); free(val);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  puts("sp-grid-ok");
  return 0;
}
#endif
