// ipm_entries.h — the interior-point iterate of CAVE_MODE_INNER_IPM, callable ALONE (TEST INFRASTRUCTURE ONLY).
//
// solve_cone_ipm_impl<C, PM1, false> (cone_core.h) on WaveCtx and on BlockCtx<4> (fixed-point Hessian), and
// lite_solve_ipm on SoloCtx<32, 4> behind the product's own lite_build: the test supplies the reduced cone as the arrays
// of a SolveView and the prediction, and reads back what the float outputs of the kernels hide: rho (w.res), theta and
// z (w.ttry) in DOUBLE after n_seq steps, f, iters and status.  Included by op_entries.h behind its helpers (OpCase,
// Carve, poison_f64); compiled, like the other entries, by g++ into the SIMT emulation and by hipcc into
// tests/prims/_prims.so.  Nothing here is algorithm code.
//
// Every array of the SolveWork is carved at the size cone_instance.h (solve_and_finish) / cone_step.h
// (run_lite_instance) give it and poisoned; the last one ends where the workgroup's LDS block ends (under emulation an
// exact-size heap block: an overrun is a finding of the sanitizer build).
//
//   OP_IPM_ITER / OP_IPM_LITE:  fin = y [d] | unused [d], n_seq = steps, ldh = p | 1
//        -> out = rho [d] | theta [p] | z [p] | f | iters | status
#pragma once

namespace cave_ops {

// bytes of the work arrays below; own_h: H [p ldh] and wold [d] too (the lite entry gets them from op_body)
CAVE_HOSTDEV uint64_t ipm_work_bytes(int d_, int p_, bool own_h) {
  const uint64_t d = (uint64_t)d_, pp = (uint64_t)(p_ > 0 ? p_ : 1), pg = pp < 33u ? 33u : pp, ldh = (uint64_t)(p_ | 1);
  uint64_t n = up16(8 * (d + 1)) + 2 * up16(8 * pg) + 5 * up16(8 * pp) + up16(pp) + 2 * up16(8 * d);
  if (own_h) n += up16(4 * d) + up16(8 * (p_ > 0 ? (uint64_t)p_ * ldh : 1u));
  return n;
}

template <int NT>
__device__ __forceinline__ void ipm_carve(Carve& lds, SolveWork& w, int d, int p, bool own_h, const float* y, int tid) {
  const uint64_t pp = (uint64_t)(p > 0 ? p : 1), pg = pp < 33u ? 33u : pp;
  w.y = const_cast<float*>(y);
  w.rc = lds.get<double>((uint64_t)d + 1);
  if (own_h) w.wold = lds.get<float>((uint64_t)d);
  w.theta = lds.get<double>(pg);
  w.ttry = lds.get<double>(pp);
  w.told = lds.get<double>(pp);
  w.g = lds.get<double>(pp);
  w.dv = lds.get<double>(pg);
  w.g2 = lds.get<double>(pp);
  w.step = lds.get<double>(pp);
  if (own_h) {
    w.ldh = p | 1;
    w.H = lds.get<double>(p > 0 ? (uint64_t)p * (uint64_t)w.ldh : 1u);
    for (int i = tid; i < p * w.ldh; i += NT) w.H[i] = poison_f64();
    for (int i = tid; i < d; i += NT) w.wold[i] = 1e30f;
  }
  w.act = lds.get<uint8_t>(pp);
  w.res = lds.get<double>((uint64_t)d);
  w.q = lds.get<double>((uint64_t)d);
  for (int i = tid; i < d; i += NT) { w.rc[i] = poison_f64(); w.res[i] = poison_f64(); w.q[i] = poison_f64(); }
  // (slot 32 of theta and dv and rc[d]: the always-zero dummies of the lite index structures, cone_instance.h / cone_step.h)
  for (int i = tid; i < (int)pg; i += NT) { w.theta[i] = (i == 32 && p <= 32) ? 0.0 : poison_f64(); w.dv[i] = w.theta[i]; }
  for (int i = tid; i < (int)pp; i += NT) {
    w.ttry[i] = poison_f64(); w.told[i] = poison_f64(); w.g[i] = poison_f64(); w.g2[i] = poison_f64(); w.step[i] = poison_f64();
    w.act[i] = 0xff;
  }
  if (tid == 0) w.rc[d] = 0.0;
  w.ls_on = false;
  w.bw = 0; w.band_wave = false; w.band_hot = false; w.bwin = nullptr; w.bfac = nullptr; w.bz = nullptr; w.bstg = nullptr; w.bch = 0;
  w.dn.on = false;
  w.gen.on = false;
  w.warm = nullptr;
}

template <int NT>
__device__ __forceinline__ void ipm_copy_out(const OpCase& k, const SolveWork& w, const SolveResult& r, int tid) {
  const int d = k.d, p = k.p;
  for (int i = tid; i < d; i += NT) k.out[i] = w.res[i];
  for (int i = tid; i < p; i += NT) { k.out[d + i] = w.theta[i]; k.out[d + p + i] = w.ttry[i]; }
  if (tid == 0) { k.out[d + 2 * p] = r.f; k.out[d + 2 * p + 1] = (double)r.iters; k.out[d + 2 * p + 2] = (double)r.status; }
}

// general form: the one-wave context sums in floating point, BlockCtx in 64-bit fixed point at the scale run_solve gives it
template <class C, bool PM1>
__device__ __forceinline__ void ipm_iter_run(C& c, Carve& lds, const SolveView& v, const OpCase& k, const float* fin) {
  constexpr int NT = C::NT;
  const int tid = (int)threadIdx.x;
  SolveWork w{};
  ipm_carve<NT>(lds, w, k.d, k.p, true, fin, tid);
  w.hscale = 1.0;
  w.hinv = 1.0;
  if constexpr (C::NWAVES > 1) {
    double vm, ml;
    cone_scales(c, v, vm, ml);
    w.hscale = fixed_scale(vm, vm * ml);
    w.hinv = 1.0 / w.hscale;
  }
  __syncthreads();
  const SolveResult r = solve_cone_ipm_impl<C, PM1, false>(c, v, w, k.n_seq);
  __syncthreads();
  ipm_copy_out<NT>(k, w, r, tid);
}

#if defined(CAVE_GPU_CODE)
// lite form: c.lite is what lite_build made of the view; H and wold are op_body's
template <class C>
__device__ __forceinline__ void ipm_lite_run(C& c, Carve& lds, const SolveView& v, const OpCase& k, const float* fin, double* H,
                                             float* wold) {
  constexpr int NT = C::NT;
  const int tid = (int)threadIdx.x;
  SolveWork w{};
  ipm_carve<NT>(lds, w, k.d, k.p, false, fin, tid);
  w.ldh = k.ldh;
  w.H = H;
  w.wold = wold;
  for (int i = tid; i < k.p * k.ldh; i += NT) H[i] = poison_f64();
  for (int i = tid; i < k.d; i += NT) wold[i] = 1e30f;
  c.sync();
  const SolveResult r = lite_solve_ipm(c, v, w, k.n_seq);
  c.sync();
  ipm_copy_out<NT>(k, w, r, tid);
}
#endif

}  // namespace cave_ops
