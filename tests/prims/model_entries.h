// model_entries.h — the model minimisation of one Newton iteration, callable ALONE (TEST INFRASTRUCTURE ONLY).
//
// lite_model_step (cone_core.h) on the one-wave context of the fused step kernel and dense_model_step (cone_dense.h) on
// the three contexts the large-cone kernels instantiate it on (WaveCtx, BlockCtx<2, true>, BlockCtx<4, true>).  Included
// by prim_entries.h behind its helpers (PrimBatch, Carve, poison_f64); compiled, like the other entries, by g++ into the
// SIMT emulation builds and by hipcc into tests/prims/_prims.so.  Nothing here is algorithm code.
//
// Every array the functions touch is carved at the size the product documents for it and poisoned; the arrays are
// ordered so that the last one ends where the workgroup's LDS block ends (the emulation's block is an exact-size heap
// block: an overrun is a finding of the sanitizer build).
#pragma once

namespace cave_prims {

// lite form: H is copied as the LOWER triangle of rows of ldh = p | 1 doubles (cone_step.h run_lite_instance); the
// strict upper triangle and the padding column are poisoned and come back in M, so a write there shows
template <class C>
__device__ __forceinline__ void model_lite_body(unsigned char* smem, const PrimBatch& a, int64_t b) {
  constexpr int NT = C::NT;
  C c = make_ctx<C>(smem);
  const int tid = (int)threadIdx.x;
  const int p = a.p, nF = a.nF, nI = p - nF, ldh = p | 1;
  const double* Hg = a.H + b * a.h_stride;
  Carve lds(smem);
  double* H = lds.get<double>((uint64_t)p * ldh);
  double* g = lds.get<double>(p);
  double* theta = lds.get<double>(p);
  double* tc = lds.get<double>(p);
  double* step = lds.get<double>(p);
  double* g2 = lds.get<double>(p);
  double* scr = lds.get<double>(lite_model_scratch(p, nI));  // XS [p * nI] | st [nI]: what the function indexes
  for (int idx = tid; idx < p * ldh; idx += NT) {
    const int i = idx / ldh, j = idx - i * ldh;
    H[idx] = (j <= i) ? Hg[i * p + j] : poison_f64();
  }
  for (int i = tid; i < p; i += NT) {
    g[i] = a.g[b * p + i];
    theta[i] = a.theta[b * p + i];
    tc[i] = poison_f64(); step[i] = poison_f64(); g2[i] = poison_f64();
  }
  for (int i = tid; i < (int)lite_model_scratch(p, nI); i += NT) scr[i] = poison_f64();
  __syncthreads();
  SolveView v{};
  v.p = p;
  SolveWork w{};
  w.H = H; w.ldh = ldh; w.g = g; w.g2 = g2; w.step = step;
  w.ls_on = true; w.ls_nF = nF; w.ls_nI = nI; w.ls_scr = scr;
  const bool moved = lite_model_step(c, v, w, theta, tc, a.reg_rel);
  __syncthreads();
  for (int i = tid; i < p; i += NT) a.tc[b * p + i] = tc[i];
  for (int idx = tid; idx < p * ldh; idx += NT) a.M[b * a.m_stride + idx] = H[idx];
  if (tid == 0) a.moved[b] = moved ? 1 : 0;
}

// dense form: A arrives folded, in elimination order; theta, g and tc are in reduced-row order; ord is the test's
// permutation (free rows at positions < nF).  The DenseWork arrays sit in one block of dense_lds_bytes(p, nI) at most,
// in the order cone_instance.h carves them, the last one ending at the end of the workgroup's LDS.
template <class C>
__device__ __forceinline__ void model_dense_body(unsigned char* smem, const PrimBatch& a, int64_t b) {
  constexpr int NT = C::NT;
  C c = make_ctx<C>(smem);
  const int tid = (int)threadIdx.x;
  const int p = a.p, nF = a.nF, nI = p - nF, ldS = nI | 1;
  const int64_t hs = (int64_t)fold_entries(p);
  const double* Hg = a.H + b * a.h_stride;
  Carve lds(smem);
  double* theta = lds.get<double>(p);
  double* g = lds.get<double>(p);
  double* tc = lds.get<double>(p);
  unsigned char* q = lds.q + model_dense_lead(p, nI);
  auto take = [&](uint64_t bytes) { unsigned char* r = q; q += bytes; return r; };
  DenseWork dw{};
  dw.on = true;
  dw.nF = nF; dw.nI = nI; dw.ldS = ldS;
  dw.A = reinterpret_cast<double*>(take(8ull * (uint64_t)hs));
  dw.dinv = reinterpret_cast<double*>(take(8ull * p));
  dw.z = reinterpret_cast<double*>(take(8ull * p));
  dw.x = reinterpret_cast<double*>(take(8ull * p));
  take((8ull * (uint64_t)hs + 24ull * p) & 8u);  // scr on a 16-byte boundary
  dw.scr = reinterpret_cast<double*>(take(8ull * dense_scratch_entries(p)));
  dw.S = reinterpret_cast<double*>(take(8ull * nI * ldS));
  dw.sg = reinterpret_cast<double*>(take(8ull * nI));
  dw.st = reinterpret_cast<double*>(take(8ull * nI));
  dw.ss = reinterpret_cast<double*>(take(8ull * nI));
  dw.sr = reinterpret_cast<double*>(take(8ull * nI));
  dw.pos = reinterpret_cast<uint16_t*>(take(2ull * p));
  dw.ord = reinterpret_cast<uint16_t*>(take(2ull * p));
  dw.sact = reinterpret_cast<uint8_t*>(take((uint64_t)nI));
  for (int64_t i = tid; i < hs; i += NT) dw.A[i] = Hg[i];
  for (int i = tid; i < p; i += NT) {
    theta[i] = a.theta[b * p + i];
    g[i] = a.g[b * p + i];
    tc[i] = poison_f64();
    dw.dinv[i] = poison_f64(); dw.z[i] = poison_f64(); dw.x[i] = poison_f64();
    const uint16_t row = a.ord[b * p + i];
    dw.ord[i] = row;
    dw.pos[row] = (uint16_t)i;
  }
  for (int i = tid; i < (int)dense_scratch_entries(p); i += NT) dw.scr[i] = poison_f64();
  for (int i = tid; i < nI * ldS; i += NT) dw.S[i] = poison_f64();
  for (int i = tid; i < nI; i += NT) {
    dw.sg[i] = poison_f64(); dw.st[i] = poison_f64(); dw.ss[i] = poison_f64(); dw.sr[i] = poison_f64();
    dw.sact[i] = 0xff;
  }
  __syncthreads();
  SolveView v{};
  v.p = p;
  const bool moved = dense_model_step(c, v, dw, theta, g, tc, a.reg_rel);
  __syncthreads();
  for (int i = tid; i < p; i += NT) a.tc[b * p + i] = tc[i];
  for (int i = tid; i < nI; i += NT) {
    a.sact_out[b * nI + i] = dw.sact[i];
    a.ss_out[b * nI + i] = dw.ss[i];
  }
  if (tid == 0) a.moved[b] = moved ? 1 : 0;
}

}  // namespace cave_prims
