// simt_apgd.cpp — SIMT emulation of the APGD projector (TEST INFRASTRUCTURE ONLY).
//
// A small unit beside simt_tsp_hk.cpp (same shim, same conventions: host pointers, a schedule seed -- 0 = round robin,
// else the lanes between two rendezvous run in a seeded random order).  It holds ONE code path: apgd_block (apgd.h), one
// workgroup of one or four waves per instance exactly as k_apgd_w1.hip / k_apgd_w4.hip launch it, behind the argument
// checks of the C ABI entry points (apgd_plan, the function the library calls), on an exact-size LDS block that is
// poisoned before every workgroup.  `waves`: 0 = the plan's choice, 1 or 4 = that workgroup size whatever the plan says
// (the results do not depend on it: tests/test_apgd_emul.py).
//
// Built two ways (tests/emul_apgd_lib.py): a shared library for ctypes, and -- with APGD_MAIN, under AddressSanitizer +
// UBSan -- a stand-alone program that reads a file of cases and writes a file of results, every input and output in a
// heap block of its exact size.  Never loaded by cave_amd.
#define CAVE_SIMT_EMUL 1
#include <hip/hip_runtime.h>

#include "../../cave_amd/csrc/apgd.h"
#include "simt_solver.h"

using namespace cave;

static char g_msg[kSolverMsg] = "";

static int32_t simt_apgd(bool sparse, const float* ctrs, const cave_sparse_cones* cones, const float* pred, int64_t B, int64_t m_max,
                         int64_t d, int32_t mode, float sign, int32_t k_start, int32_t n_iter, int32_t power_iter, int32_t nnz_cap,
                         double* x_curr, double* x_prev, double* step, float* proj, float* rnorm, float* target, float* loss,
                         float* grad, int32_t* status, int32_t* iters, double* pgrad, uint64_t seed, int32_t waves_forced) {
  ApgdParams P;
  int64_t grid;
  int waves;
  g_msg[0] = 0;
  const int32_t rc = apgd_plan(sparse, ctrs, cones, pred, B, m_max, d, mode, sign, k_start, n_iter, power_iter, nnz_cap, x_curr, x_prev,
                               step, proj, rnorm, target, loss, grad, status, iters, pgrad, &P, &grid, &waves, g_msg);
  if (rc != CAVE_OK || grid == 0) return rc;
  if (waves_forced == 1 || waves_forced == 4) waves = waves_forced;
  simt_solver::run_grid(64 * waves, grid, (size_t)P.L.bytes, seed, [&](unsigned char* lds) {  // the bodies of the four kernels
    if (waves == 1) { if (sparse) apgd_block<1, true>(P, lds); else apgd_block<1, false>(P, lds); }
    else { if (sparse) apgd_block<4, true>(P, lds); else apgd_block<4, false>(P, lds); }
  });
  return CAVE_OK;
}

extern "C" {

const char* cave_simt_apgd_last_error(void) { return g_msg; }
int32_t cave_simt_apgd_lds_bytes(int64_t m_max, int64_t d, int64_t nnz_cap) { return (int32_t)apgd_lds_bytes(m_max, d, nnz_cap); }
int32_t cave_simt_apgd_waves(int64_t m_max, int64_t d, int64_t nnz_cap) { return apgd_waves(m_max, d, nnz_cap); }

// cave_hip_cone_apgd / cave_hip_cone_apgd_sparse (cave_hip.hip), their checks and their launch shape
int32_t cave_simt_cone_apgd(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d, int32_t mode, float sign,
                            int32_t k_start, int32_t n_iter, int32_t power_iter, int32_t nnz_cap, double* x_curr, double* x_prev,
                            double* step, float* proj, float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                            int32_t* iters, double* pgrad, uint64_t seed, int32_t waves) {
  return simt_apgd(false, ctrs, nullptr, pred, B, m_max, d, mode, sign, k_start, n_iter, power_iter, nnz_cap, x_curr, x_prev, step, proj,
                   rnorm, target, loss, grad, status, iters, pgrad, seed, waves);
}
int32_t cave_simt_cone_apgd_sparse(const cave_sparse_cones* cones, const float* pred, int32_t mode, float sign, int32_t k_start,
                                   int32_t n_iter, int32_t power_iter, int32_t nnz_cap, double* x_curr, double* x_prev, double* step,
                                   float* proj, float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                                   int32_t* iters, double* pgrad, uint64_t seed, int32_t waves) {
  return simt_apgd(true, nullptr, cones, pred, 0, 0, 0, mode, sign, k_start, n_iter, power_iter, nnz_cap, x_curr, x_prev, step, proj,
                   rnorm, target, loss, grad, status, iters, pgrad, seed, waves);
}

}  // extern "C"

#ifdef APGD_MAIN
// prog IN OUT (simt_solver.h).  Per case int64 {sparse, B, m_max, d, Z, mode, sign, n_iter, power_iter, nnz_cap, seed,
// waves}, then ctrs [B m_max d] fp32 (dense) or ent_off [B+1] int64, key [Z] uint32, val [Z] fp32 (sparse), then pred
// [B d] fp32.  A cold launch (k_start = 0) with every output given.  Outputs: proj, rnorm, target, loss, grad, status,
// iters, x_curr, x_prev, step, pgrad.
int main(int argc, char** argv) {
  return simt_solver::case_main(argc, argv, "apgd-ok", [](simt_solver::Case& k) {
    int64_t h[12];
    if (!k.header(h, 12)) return false;
    const int64_t B = h[1], m = h[2], d = h[3], Z = h[4];
    const bool sparse = h[0] != 0;
    float* ctrs = k.input<float>((size_t)(B * m * d), !sparse);
    cave_sparse_cones S;
    S.B = B; S.m_max = (int32_t)m; S.d = (int32_t)d;
    S.ent_off = k.input<int64_t>((size_t)B + 1, sparse);
    S.key = k.input<uint32_t>((size_t)Z, sparse);
    S.val = k.input<float>((size_t)Z, sparse);
    float* pred = k.input<float>((size_t)(B * d));
    if (!k.good) return false;
    float* proj = k.output<float>(true, (size_t)(B * d));
    float* rnorm = k.output<float>(true, (size_t)B);
    float* target = k.output<float>(true, (size_t)(B * d));
    float* loss = k.output<float>(true, (size_t)B);
    float* grad = k.output<float>(true, (size_t)(B * d));
    int32_t* st = k.output<int32_t>(true, (size_t)B);
    int32_t* it = k.output<int32_t>(true, (size_t)B);
    double* xc = k.output<double>(true, (size_t)(B * m));
    double* xp = k.output<double>(true, (size_t)(B * m));
    double* step = k.output<double>(true, (size_t)B);
    double* pg = k.output<double>(true, (size_t)B);
    if (xc) memset(xc, 0xFF, (size_t)(B * m) * 8);  // (a failed instance leaves its state alone)
    if (xp) memset(xp, 0xFF, (size_t)(B * m) * 8);
    if (step) memset(step, 0xFF, (size_t)B * 8);
    const int32_t rc = simt_apgd(sparse, ctrs, sparse ? &S : nullptr, pred, B, m, d, (int32_t)h[5], (float)h[6], 0, (int32_t)h[7],
                                 (int32_t)h[8], (int32_t)h[9], xc, xp, step, proj, rnorm, target, loss, grad, st, it, pg,
                                 (uint64_t)h[10], (int32_t)h[11]);
    return k.done(rc);
  });
}
#endif
