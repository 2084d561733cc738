// simt_tight_cones.cpp — SIMT emulation of the tight-cone kernels (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_sp_grid.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin,
// else the lanes between two rendezvous run in a seeded random order).  It holds the two kernel bodies of
// k_tight_cones.hip (tight_cones_count_instance, tight_cones_fill_instance: tight_cones.h), one 64-lane wave per instance
// in workgroups of kTightWaves waves exactly as the library launches them, behind the argument checks of the C ABI entry
// points (tight_cones_plan, the function the library calls).  The kernels use no LDS.
//
// Built two ways (tests/emul_tight_cones_lib.py): a shared library for ctypes, and -- with TIGHT_CONES_MAIN, under
// AddressSanitizer + UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every
// input and output in a heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include "../../cave_amd/csrc/tight_cones.h"
#include "simt_solver.h"

using namespace cave;

static int32_t simt_tight_cones(bool fill, const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off,
                                const float* sol, int64_t N, double tol, int32_t* n_rows, int64_t* n_ent, const int64_t* ent_off,
                                int64_t ent_cap, uint32_t* key, float* val, int32_t* status, uint64_t seed) {
  TightConesParams P;
  int64_t grid;
  char msg[kSolverMsg];
  const int32_t rc = tight_cones_plan(fill, sys, lazy, lazy_off, sol, N, tol, n_rows, n_ent, ent_off, ent_cap, key, val, status, &P,
                                      &grid, msg);
  if (rc != CAVE_OK || grid == 0) return rc;
  simt_solver::run_grid(64 * kTightWaves, grid, 0, seed, [&](unsigned char*) {  // the body of tight_cones_kernel<FILL>
    const int64_t b = (int64_t)blockIdx.x * (int64_t)kTightWaves + (int64_t)(threadIdx.x >> 6);
    if (b >= P.N) return;
    if (fill) tight_cones_fill_instance(P, b, (int)(threadIdx.x & 63u));
    else tight_cones_count_instance(P, b, (int)(threadIdx.x & 63u));
  });
  return CAVE_OK;
}

extern "C" {

// cave_hip_tight_cones_count / cave_hip_tight_cones_fill (cave_hip.hip), their checks and their launch shape
int32_t cave_simt_tight_cones_count(const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off, const float* sol,
                                    int64_t N, double tol, int32_t* n_rows, int64_t* n_ent, int32_t* status, uint64_t seed) {
  return simt_tight_cones(false, sys, lazy, lazy_off, sol, N, tol, n_rows, n_ent, nullptr, 0, nullptr, nullptr, status, seed);
}
int32_t cave_simt_tight_cones_fill(const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off, const float* sol,
                                   int64_t N, double tol, const int64_t* ent_off, int64_t ent_cap, uint32_t* key, float* val,
                                   int32_t* status, uint64_t seed) {
  return simt_tight_cones(true, sys, lazy, lazy_off, sol, N, tol, nullptr, nullptr, ent_off, ent_cap, key, val, status, seed);
}

}  // extern "C"

#ifdef TIGHT_CONES_MAIN
// prog IN OUT (simt_solver.h).  Per case int64 {N, d, R, Z, L, LZ, flags, seed, cap, the bits of the fp64 tol}, then
// row_off [R+1], col [Z], coef [Z], sense [R], rhs [R] of the shared system, the same five of the lazy system (flags & 1),
// lazy_off [N+1] (flags & 2) and sol [N d].  The program runs the count pass, forms the exclusive scan and runs the fill
// pass on key / val blocks of exactly `cap` entries (filled with 0xFF before).  Outputs: n_rows, n_ent, status of the
// count pass, status of the fill pass, key, val.
static cave_lin_system read_system(simt_solver::Case& k, int64_t R, int64_t Z, int64_t d) {
  cave_lin_system s;
  s.R = R; s.Z = Z; s.d = (int32_t)d; s.reserved = 0;
  s.row_off = k.input<int64_t>((size_t)R + 1);
  s.col = k.input<int32_t>((size_t)Z);
  s.coef = k.input<float>((size_t)Z);
  s.sense = k.input<int8_t>((size_t)R);
  s.rhs = k.input<double>((size_t)R);
  return s;
}

int main(int argc, char** argv) {
  return simt_solver::case_main(argc, argv, "tight-cones-ok", [](simt_solver::Case& k) {
    int64_t hdr[10];
    if (!k.header(hdr, 10)) return false;
    const int64_t N = hdr[0], d = hdr[1], flags = hdr[6], cap = hdr[8];
    double tol;
    memcpy(&tol, &hdr[9], 8);
    cave_lin_system sys = read_system(k, hdr[2], hdr[3], d), lazy;
    if (flags & 1) lazy = read_system(k, hdr[4], hdr[5], d);
    int64_t* lazy_off = k.input<int64_t>((size_t)N + 1, flags & 2);
    float* sol = k.input<float>((size_t)(N * d));
    if (!k.good) return false;
    int32_t* n_rows = k.output<int32_t>(true, (size_t)N);
    int64_t* n_ent = k.output<int64_t>(true, (size_t)N);
    int32_t* st = k.output<int32_t>(true, (size_t)N);
    int32_t* fst = k.output<int32_t>(true, (size_t)N);
    uint32_t* key = k.output<uint32_t>(true, (size_t)cap);
    float* val = k.output<float>(true, (size_t)cap);
    if (key) memset(key, 0xFF, (size_t)cap * 4);
    if (val) memset(val, 0xFF, (size_t)cap * 4);
    int32_t rc = cave_simt_tight_cones_count(&sys, (flags & 1) ? &lazy : nullptr, lazy_off, sol, N, tol, n_rows, n_ent, st, (uint64_t)hdr[7]);
    if (rc == CAVE_OK) {
      int64_t* ent_off = k.block<int64_t>((size_t)N + 1);
      ent_off[0] = 0;
      for (int64_t b = 0; b < N; ++b) ent_off[b + 1] = ent_off[b] + n_ent[b];
      rc = cave_simt_tight_cones_fill(&sys, (flags & 1) ? &lazy : nullptr, lazy_off, sol, N, tol, ent_off, cap, key, val, fst,
                                      (uint64_t)hdr[7]);
    }
    return k.done(rc);
  });
}
#endif
