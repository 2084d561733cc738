// op_entries.h — the operators of the Newton loop, each callable ALONE (TEST INFRASTRUCTURE ONLY).
//
// The other half of prim_entries.h: the code that builds what the linear solvers are given and consumes what they
// return -- the gathers y - M^T theta, the gradient g = -M Pi(r) in its six forms, the Hessian M W M^T in its five, the
// weight functions, the line search and the epilogue.  One per-workgroup body per operator, written once and compiled
// twice: by g++ into the plain SIMT emulation build (tests/emul/simt_abi.cpp with CAVE_SIMT_OPS, CPU tier; the sanitizer
// and variant builds of that unit leave it out) and by hipcc into tests/prims/_prims.so (tests/prims/ops_abi.hip, GPU
// tier).  A body copies one case of the batch into LDS in the layout the
// product uses, runs the product's function on the product's context type and wave count and copies out what the
// function wrote.  The test supplies the reduced cone directly, as the arrays of a SolveView.  Nothing here is
// algorithm code: the operators are the ones of cave_amd/csrc, untouched.  Never loaded by cave_amd.
//
// Include after prim_entries.h (make_ctx, Carve, poison_f64, CtxInfo come from there).
#pragma once
#include <stdint.h>

namespace cave_ops {
using namespace cave;
using cave_prims::Carve;
using cave_prims::CtxInfo;
using cave_prims::make_ctx;
using cave_prims::poison_f64;
using cave_prims::SoloT;
using cave_prims::up16;

// One case = one workgroup.  Every pointer is memory of the tier (host under emulation, device on the GPU); every
// array is padded by one element (the product's loads of entry `min(e, last)` are unconditional).
struct OpCase {
  int32_t d, p, nnz, nlong, nteam, mode, flags, n_seq;
  int32_t ldh, empty, n_outf, n_out;
  int32_t n_in[4];
  double s[4];              // scalars of the operator (see the kinds)
  const uint32_t* mptr;     // the arrays of the SolveView
  const uint16_t* mcol;
  const float* mval;
  const uint32_t* cptr;
  const uint16_t* cvar;
  const float* cvalc;
  const uint8_t* usign;
  const uint8_t* vkind;
  const uint32_t* longrow;
  const uint32_t* teamrow;
  const float* fin;         // [n_fin = 2 d]  y | avg   (epilogue, gathers: base = y;  lite_hessian_ipm: the weights)
  const double* in[4];      // [n_in[i]]
  double* out;              // [n_out]   NaN-poisoned by the caller
  float* outf;              // [n_outf]  NaN-poisoned by the caller
  int32_t* outi;            // [4]
};

enum : int32_t {
  OP_GATHER = 0,       // gather_mt                       in0 = th [p], s0 = sgn, flags bit 0: base = null   -> out [d]
  OP_GATHER_ST = 1,    // gather_mt_streamed<.., 1>       (view in global memory)
  OP_GATHER_DIET = 2,  // gather_mt_streamed<.., 0>       (cptr in LDS, cvar in global memory)
  OP_REFRESH = 3,      // refresh_clipped<C, 1>           in0 = r [d]                     -> out [d] = rc, out[d] = f
  OP_REFRESH_RB = 4,   // refresh_clipped<C, 8>
  OP_DPHI = 5,         // dphi<C, 1>                      in0 = r, in1 = q, s0 = alpha    -> out[0] = phi', out[1] = phi''
  OP_DPHI_RB = 6,      // dphi<C, 8>
  OP_UPDATE = 7,       // update_theta<C, 1>              in0 = theta, in1 = tc, in2 = dv, s0 = alpha, s1 = amax -> out [p]
  OP_UPDATE_RB = 8,    // update_theta<C, 8>
  OP_GRAD = 9,         // gradient<C, PM1, false>         in0 = rc [d]                    -> out [p]
  OP_GRAD_ST = 10,     // gradient<C, PM1, true>, gcol_bound = 0: short rows, long rows, team rows, all streamed
  OP_GRAD_DENSE = 11,  // gradient<C, PM1, true>, gcol_bound = s0 > 0: dense_gradient
  OP_WEIGHT = 12,      // band_weight(usign[k], in0[k], s0 = 1 / mu)                      -> out [d]
  OP_BAND_H = 13,      // band_hessian    flags bit 0: in_lds, bit 1: weights = in0 (else band_weight(usign, in0 = r, s0))
                       //                 -> out [p ldh] = H, out[p ldh] = hscale, out[p ldh + 1] = vm * ml
  OP_DENSE_H = 14,     // dense_order + dense_hessian   (flags bit 1 as above)
                       //                 -> out = A [fold_entries(p)] | pos [p] | ord [p] | nF | hscale | vm * ml
  OP_EPILOGUE = 15,    // epilogue   fin = y | avg, in0 = res [d], s0 = f, s1 = sign, s2 = inner_ratio,
                       //            flags bits 0..4: proj / rnorm / target / loss / grad are null
                       //                 -> outf = proj [d] | target [d] | grad [d] | rnorm | loss
  OP_LITE_GATHER = 16, // lite_build + lite_gather        in0 = x [33] (x[32] = 0), s0 = sgn -> out [d], outi[0] = accepted
  OP_LITE_GRAD = 17,   // lite_build + lite_gradient      in0 = rc [d + 1] (rc[d] = 0)    -> out [p]
  OP_LITE_HESS = 18,   // lite_build + n_seq calls of lite_hessian on the same H / wold:  in0 = r [n_seq, d],
                       //   in1 = mu [n_seq]  -> out [n_seq, p ldh + d]: H | wold after every call (upper triangle of H
                       //   starts as NaN poison: it must come back untouched)
  OP_LITE_HESS_IPM = 19,  // lite_build + lite_hessian_ipm   fin = weights [d]             -> out [p ldh]
  OP_IPM_ITER = 20,    // n_seq steps of solve_cone_ipm_impl<C, PM1, false>   (ipm_entries.h)   fin = y
                       //                 -> out = rho [d] | theta [p] | z [p] | f | iters | status
  OP_IPM_LITE = 21,    // lite_build + n_seq steps of lite_solve_ipm          (ipm_entries.h)   same outputs
  OP_COUNT = 22,
};
enum : int32_t { CX_W1 = 0, CX_B2 = 1, CX_B4 = 2, CX_L2 = 3, CX_L4 = 4, CX_SOLO = 5, CX_COUNT = 6 };

template <int CX> struct OpCtx { using type = WaveCtx; };
template <> struct OpCtx<CX_B2> { using type = BlockCtx<2>; };
template <> struct OpCtx<CX_B4> { using type = BlockCtx<4>; };
template <> struct OpCtx<CX_L2> { using type = BlockCtx<2, true>; };
template <> struct OpCtx<CX_L4> { using type = BlockCtx<4, true>; };
template <> struct OpCtx<CX_SOLO> { using type = SoloT; };

constexpr int cx_threads(int cx) { return (cx == CX_B4 || cx == CX_L4) ? 256 : (cx == CX_B2 || cx == CX_L2) ? 128 : 64; }
constexpr int32_t op_kind(int op, int cx, bool pm1) { return (op * CX_COUNT + cx) * 2 + (pm1 ? 1 : 0); }

constexpr bool op_is_lite(int op) { return (op >= OP_LITE_GATHER && op <= OP_LITE_HESS_IPM) || op == OP_IPM_LITE; }
// where the cone's index arrays live while the operator runs: LDS (the small-cone kernels) or global memory (the
// large-cone path reads them with global_* loads: space_cast<1>)
constexpr bool op_view_in_lds(int op) {
  return !(op == OP_GATHER_ST || op == OP_GATHER_DIET || op == OP_GRAD_ST || op == OP_GRAD_DENSE || op == OP_BAND_H || op == OP_DENSE_H);
}
// does the operator leave its result in an LDS vector the body copies out (else it writes global memory itself)
constexpr bool op_out_in_lds(int op) {
  return op != OP_BAND_H && op != OP_EPILOGUE && op != OP_LITE_HESS && op != OP_LITE_HESS_IPM && op != OP_IPM_ITER && op != OP_IPM_LITE;
}

// does the operator read y / avg / the float weights
constexpr bool op_uses_fin(int op) { return op <= OP_GATHER_DIET || op == OP_EPILOGUE || op_is_lite(op) || op == OP_IPM_ITER; }

CAVE_HOSTDEV uint32_t lite_arena_bytes(int d, uint32_t nnz) { return lite_lds_bytes(d, nnz) + 64u; }
CAVE_HOSTDEV uint64_t ipm_work_bytes(int d, int p, bool own_h);  // ipm_entries.h

// LDS of one workgroup: [context scratch 256 | view arrays | usign | vkind | fin | in0..3 | out | work arrays of the op]
CAVE_HOSTDEV uint32_t op_lds_bytes(int op, bool pm1, const OpCase& k) {
  const uint64_t d = (uint64_t)k.d, p = (uint64_t)k.p, nz = (uint64_t)k.nnz + 1u;
  uint64_t n = 256;
  if (op_view_in_lds(op)) {
    n += up16(4 * (p + 1)) + up16(2 * nz) + up16(4 * (d + 1)) + up16(2 * nz) + up16(4 * ((uint64_t)k.nlong + 1)) + up16(4 * ((uint64_t)k.nteam + 1));
    if (!pm1) n += 2 * up16(4 * nz);
  } else if (op == OP_GATHER_DIET) n += up16(4 * (d + 1));
  n += up16(d + 1) + up16(p + 1) + (op_uses_fin(op) ? up16(4 * (2 * d + 1)) : 0u);
  for (int i = 0; i < 4; ++i) n += up16(8 * ((uint64_t)k.n_in[i] + 1));
  if (op_out_in_lds(op)) n += up16(8 * ((uint64_t)k.n_out + 1));
  if (op == OP_BAND_H && (k.flags & 1)) n += up16(8 * p * (uint64_t)k.ldh);
  if (op == OP_DENSE_H) n += up16(8ull * fold_entries(k.p)) + 2 * up16(2 * p) + up16(4 * p);
  if (op == OP_EPILOGUE) n += up16(8 * (d + 1));
  if (op_is_lite(op)) n += up16(lite_arena_bytes(k.d, (uint32_t)k.nnz)) + up16(8 * (p * (uint64_t)k.ldh + 1)) + up16(4 * (d + 1));
  if (op == OP_IPM_ITER || op == OP_IPM_LITE) n += ipm_work_bytes(k.d, k.p, op == OP_IPM_ITER);
  return (uint32_t)(n > 0xffffffffull ? 0xffffffffull : n);
}

template <class T, int NT>
__device__ __forceinline__ T* stage(Carve& lds, const T* src, uint64_t n, int tid) {  // n elements + one of padding
  T* q = lds.get<T>(n + 1);
  for (uint64_t i = (uint64_t)tid; i < n + 1; i += NT) q[i] = src[i];
  return q;
}

// largest |entry| and longest row of the reduced cone -> the fixed-point scale, as cone_instance.h run_solve does
template <class C>
__device__ __forceinline__ void cone_scales(C& c, const SolveView& v, double& vm, double& ml) {
  const int p = v.p;
  vm = v.pm1 ? 1.0 : 0.0;
  ml = 1.0;
  if (!v.pm1) {
    const uint32_t nz = v.mptr[p];
    for (uint32_t e = c.tid(); e < nz; e += (uint32_t)C::NT) vm = fmax(vm, fabs((double)v.mval[e]));
  }
  for (int i = c.tid(); i < p; i += C::NT) ml = fmax(ml, (double)(v.mptr[i + 1] - v.mptr[i]));
  vm = c.reduce_max(vm);
  ml = c.reduce_max(ml);
}

}  // namespace cave_ops
#include "ipm_entries.h"
namespace cave_ops {

template <int OP, int CX, bool PM1>
__device__ __forceinline__ void op_body(unsigned char* smem, const OpCase& k) {
  using C = typename OpCtx<CX>::type;
  constexpr int NT = cx_threads(CX);
  static_assert(NT == C::NT, "workgroup shape");
  C c = make_ctx<C>(smem);
  const int tid = (int)threadIdx.x;
  const int d = k.d, p = k.p;
  const uint64_t nz = (uint64_t)k.nnz;
  Carve lds(smem);
  SolveView v{};
  v.d = d; v.p = p; v.n_valid = k.empty ? 0 : 1; v.pm1 = PM1;
  v.nlong = k.nlong; v.nteam = k.nteam; v.gcol_bound = 0.0; v.csc_far = false;
  if constexpr (op_view_in_lds(OP)) {
    v.mptr = stage<uint32_t, NT>(lds, k.mptr, (uint64_t)p + 1 - 1, tid);
    v.mcol = stage<uint16_t, NT>(lds, k.mcol, nz, tid);
    v.cptr = stage<uint32_t, NT>(lds, k.cptr, (uint64_t)d + 1 - 1, tid);
    v.cvar = stage<uint16_t, NT>(lds, k.cvar, nz, tid);
    v.longrow = stage<uint32_t, NT>(lds, k.longrow, (uint64_t)k.nlong, tid);
    v.teamrow = stage<uint32_t, NT>(lds, k.teamrow, (uint64_t)k.nteam, tid);
    if constexpr (!PM1) {
      v.mval = stage<float, NT>(lds, k.mval, nz, tid);
      v.cvalc = stage<float, NT>(lds, k.cvalc, nz, tid);
    }
  } else {
    v.mptr = k.mptr; v.mcol = k.mcol; v.cptr = k.cptr; v.cvar = k.cvar; v.longrow = k.longrow; v.teamrow = k.teamrow;
    if constexpr (!PM1) { v.mval = k.mval; v.cvalc = k.cvalc; }
    if constexpr (OP == OP_GATHER_DIET) { v.cptr = stage<uint32_t, NT>(lds, k.cptr, (uint64_t)d, tid); v.csc_far = true; }
  }
  v.usign = stage<uint8_t, NT>(lds, k.usign, (uint64_t)d, tid);
  v.vkind = stage<uint8_t, NT>(lds, k.vkind, (uint64_t)p, tid);
  const float* fin = nullptr;
  if constexpr (op_uses_fin(OP)) fin = stage<float, NT>(lds, k.fin, 2 * (uint64_t)d, tid);
  double* a[4];
  for (int i = 0; i < 4; ++i) a[i] = stage<double, NT>(lds, const_cast<const double*>(k.in[i]), (uint64_t)k.n_in[i], tid);
  double* o = nullptr;
  if constexpr (op_out_in_lds(OP)) {
    o = lds.get<double>((uint64_t)k.n_out + 1);
    for (int i = tid; i < k.n_out; i += NT) o[i] = poison_f64();
  }
  __syncthreads();
  const float* base = (k.flags & 1) ? nullptr : fin;

  if constexpr (OP == OP_GATHER) gather_mt<C, PM1>(c, v, base, a[0], k.s[0], o);
  else if constexpr (OP == OP_GATHER_ST) gather_mt_streamed<C, PM1, 1>(c, v, base, a[0], k.s[0], o);
  else if constexpr (OP == OP_GATHER_DIET) gather_mt_streamed<C, PM1, 0>(c, v, base, a[0], k.s[0], o);
  else if constexpr (OP == OP_REFRESH || OP == OP_REFRESH_RB) {
    const double f = refresh_clipped<C, OP == OP_REFRESH ? 1 : 8>(c, v, a[0], o);
    if (tid == 0) o[d] = f;
  } else if constexpr (OP == OP_DPHI || OP == OP_DPHI_RB) {
    double d1, d2;
    dphi<C, OP == OP_DPHI ? 1 : 8>(c, v, a[0], a[1], k.s[0], &d1, &d2);
    if (tid == 0) { o[0] = d1; o[1] = d2; }
  } else if constexpr (OP == OP_UPDATE || OP == OP_UPDATE_RB) {
    for (int i = tid; i < p; i += NT) o[i] = a[0][i];
    __syncthreads();
    update_theta<C, OP == OP_UPDATE ? 1 : 8>(c, v, o, a[1], a[2], k.s[0], k.s[1]);
  } else if constexpr (OP == OP_GRAD) gradient<C, PM1, false>(c, v, a[0], o);
  else if constexpr (OP == OP_GRAD_ST) gradient<C, PM1, true>(c, v, a[0], o);
  else if constexpr (OP == OP_GRAD_DENSE) {
    v.gcol_bound = k.s[0];
    gradient<C, PM1, true>(c, v, a[0], o);
  } else if constexpr (OP == OP_WEIGHT) {
    for (int i = tid; i < d; i += NT) o[i] = band_weight(v.usign[i], a[0][i], k.s[0]);
  } else if constexpr (OP == OP_BAND_H) {
    SolveWork w{};
    w.ldh = k.ldh; w.bw = k.ldh - 1;
    w.H = k.out;
    const bool in_lds = (k.flags & 1) != 0;
    w.bwin = in_lds ? lds.get<double>((uint64_t)p * k.ldh) : nullptr;
    double vm, ml;
    cone_scales(c, v, vm, ml);
    w.hscale = fixed_scale(vm, vm * ml);
    w.hinv = 1.0 / w.hscale;
    const double* x = a[0];
    const double inv_mu = k.s[0];
    if (k.flags & 2) band_hessian<C, PM1>(c, v, w, in_lds, [&](int kk) -> double { return x[kk]; });
    else band_hessian<C, PM1>(c, v, w, in_lds, [&](int kk) -> double { return band_weight(v.usign[kk], x[kk], inv_mu); });
    if (tid == 0) { k.out[(int64_t)p * k.ldh] = w.hscale; k.out[(int64_t)p * k.ldh + 1] = vm * ml; }
  } else if constexpr (OP == OP_DENSE_H) {
    DenseWork dw{};
    const int ne = (int)fold_entries(p);
    dw.A = lds.get<double>((uint64_t)ne);
    dw.pos = lds.get<uint16_t>((uint64_t)p);
    dw.ord = lds.get<uint16_t>((uint64_t)p);
    uint32_t* tmp = lds.get<uint32_t>((uint64_t)p);
    for (int i = tid; i < ne; i += NT) dw.A[i] = poison_f64();
    for (int i = tid; i < p; i += NT) { dw.pos[i] = 0xffffu; dw.ord[i] = 0xffffu; }
    __syncthreads();
    dw.on = true;
    dense_order(c, v, dw, tmp);
    double vm, ml;
    cone_scales(c, v, vm, ml);
    dw.hscale = fixed_scale(vm, vm * ml);
    dw.hinv = 1.0 / dw.hscale;
    const double* x = a[0];
    const double inv_mu = k.s[0];
    if (k.flags & 2) dense_hessian<C, PM1>(c, v, [=](int kk) -> double { return x[kk]; }, dw);
    else {
      const uint8_t* us = v.usign;
      dense_hessian<C, PM1>(c, v, [=](int kk) -> double { return band_weight(us[kk], x[kk], inv_mu); }, dw);
    }
    __syncthreads();
    for (int i = tid; i < ne; i += NT) o[i] = dw.A[i];
    for (int i = tid; i < p; i += NT) { o[ne + i] = (double)dw.pos[i]; o[ne + p + i] = (double)dw.ord[i]; }
    if (tid == 0) { o[ne + 2 * p] = (double)dw.nF; o[ne + 2 * p + 1] = dw.hscale; o[ne + 2 * p + 2] = vm * ml; }
  } else if constexpr (OP == OP_EPILOGUE) {
    double* tvec = lds.get<double>((uint64_t)d + 1);
    for (int i = tid; i < d; i += NT) tvec[i] = poison_f64();
    __syncthreads();
    EpilogueOut eo;
    eo.proj = (k.flags & 1) ? nullptr : k.outf;
    eo.rnorm = (k.flags & 2) ? nullptr : k.outf + 3 * d;
    eo.target = (k.flags & 4) ? nullptr : k.outf + d;
    eo.loss = (k.flags & 8) ? nullptr : k.outf + 3 * d + 1;
    eo.grad = (k.flags & 16) ? nullptr : k.outf + 2 * d;
    epilogue(c, k.mode, d, (float)k.s[1], (float)k.s[2], k.empty != 0, fin, a[0], k.s[0], fin + d, tvec, eo);
  } else if constexpr (OP == OP_IPM_ITER) ipm_iter_run<C, PM1>(c, lds, v, k, fin);
#if defined(CAVE_GPU_CODE)
  else if constexpr (op_is_lite(OP)) {
    // the structures come from the product's own lite_build, on the one-wave context of the one-wave kernels; the solver
    // then runs on SoloCtx<32, 4> with sc.lite = L (cone_instance.h run_solve)
    static_assert(CX == CX_SOLO && PM1, "the lite form: one wave, +-1 cones");
    Arena ar;
    const uint32_t ab = lite_arena_bytes(d, (uint32_t)k.nnz);
    ar.init(lds.get<unsigned char>(ab), ab);
    double* H = lds.get<double>((uint64_t)p * k.ldh + 1);
    float* wold = lds.get<float>((uint64_t)d + 1);
    WaveCtx wc;
    wc.init(smem);
    LiteCone L{};
    const bool ok = lite_build(wc, ar, v, L);
    if (tid == 0) k.outi[0] = ok ? 1 : 0;
    if (ok) {
      c.lite = L;
      SolveWork w{};
      w.ldh = k.ldh; w.H = H; w.wold = wold;
      const int hs = p * k.ldh;
      if constexpr (OP == OP_LITE_GATHER) lite_gather(c, L, d, base, a[0], k.s[0], o);
      else if constexpr (OP == OP_LITE_GRAD) lite_gradient(c, L, p, a[0], o);
      else if constexpr (OP == OP_IPM_LITE) ipm_lite_run(c, lds, v, k, fin, H, wold);
      else if constexpr (OP == OP_LITE_HESS) {
        for (int i = tid; i < hs; i += NT) H[i] = (i % k.ldh) > (i / k.ldh) ? poison_f64() : 0.0;
        for (int i = tid; i < d; i += NT) wold[i] = 0.0f;
        c.sync();
        for (int s = 0; s < k.n_seq; ++s) {
          const double mu = a[1][s];
          lite_hessian(c, L, v, w, a[0] + (int64_t)s * d, mu, mu > 0.0 ? 1.0 / mu : 0.0);
          c.sync();
          double* dst = k.out + (int64_t)s * (hs + d);
          for (int i = tid; i < hs; i += NT) dst[i] = H[i];
          for (int i = tid; i < d; i += NT) dst[hs + i] = (double)wold[i];
          c.sync();
        }
      } else {
        for (int i = tid; i < hs; i += NT) H[i] = poison_f64();
        for (int i = tid; i < d; i += NT) wold[i] = fin[i];
        c.sync();
        lite_hessian_ipm(c, L, v, w);
        for (int i = tid; i < hs; i += NT) k.out[i] = H[i];
      }
    }
  }
#endif
  __syncthreads();
  if constexpr (op_out_in_lds(OP))
    for (int i = tid; i < k.n_out; i += NT) k.out[i] = o[i];
}

// X(op, ctx, pm1) for every entry: each function on the contexts the product instantiates it on
#define CAVE_OP_SMALL3(X, OP) X(OP, CX_W1, false) X(OP, CX_W1, true) X(OP, CX_B2, false) X(OP, CX_B2, true) X(OP, CX_B4, false) X(OP, CX_B4, true)
#define CAVE_OP_LARGE3(X, OP) X(OP, CX_W1, false) X(OP, CX_W1, true) X(OP, CX_L2, false) X(OP, CX_L2, true) X(OP, CX_L4, false) X(OP, CX_L4, true)
#define CAVE_OP_R1(X, OP) X(OP, CX_W1, true) X(OP, CX_B2, true) X(OP, CX_B4, true) X(OP, CX_SOLO, true)
#define CAVE_OP_RB(X, OP) X(OP, CX_W1, true) X(OP, CX_L2, true) X(OP, CX_L4, true)
#if defined(CAVE_GPU_CODE)
#define CAVE_OP_LITE_KINDS(X) \
  X(OP_LITE_GATHER, CX_SOLO, true) X(OP_LITE_GRAD, CX_SOLO, true) X(OP_LITE_HESS, CX_SOLO, true) X(OP_LITE_HESS_IPM, CX_SOLO, true) \
  X(OP_IPM_LITE, CX_SOLO, true)
#else
#define CAVE_OP_LITE_KINDS(X)
#endif
#define CAVE_OP_KINDS(X)                                                                                   \
  CAVE_OP_SMALL3(X, OP_GATHER) CAVE_OP_LARGE3(X, OP_GATHER_ST) X(OP_GATHER_DIET, CX_L4, true)             \
  CAVE_OP_R1(X, OP_REFRESH) CAVE_OP_RB(X, OP_REFRESH_RB) CAVE_OP_R1(X, OP_DPHI) CAVE_OP_RB(X, OP_DPHI_RB)  \
  CAVE_OP_R1(X, OP_UPDATE) CAVE_OP_RB(X, OP_UPDATE_RB)                                                    \
  CAVE_OP_SMALL3(X, OP_GRAD) CAVE_OP_LARGE3(X, OP_GRAD_ST)                                                \
  X(OP_GRAD_DENSE, CX_L2, false) X(OP_GRAD_DENSE, CX_L2, true) X(OP_GRAD_DENSE, CX_L4, false) X(OP_GRAD_DENSE, CX_L4, true) \
  X(OP_WEIGHT, CX_W1, true)                                                                               \
  CAVE_OP_LARGE3(X, OP_BAND_H)                                                                            \
  X(OP_DENSE_H, CX_L2, false) X(OP_DENSE_H, CX_L2, true) X(OP_DENSE_H, CX_L4, false) X(OP_DENSE_H, CX_L4, true) \
  X(OP_EPILOGUE, CX_W1, true) X(OP_EPILOGUE, CX_B4, true) X(OP_EPILOGUE, CX_SOLO, true)                   \
  X(OP_IPM_ITER, CX_W1, false) X(OP_IPM_ITER, CX_W1, true) X(OP_IPM_ITER, CX_B4, false) X(OP_IPM_ITER, CX_B4, true) \
  CAVE_OP_LITE_KINDS(X)

// the limits the product's dispatch guarantees, and the ones of this harness
CAVE_HOSTDEV bool op_case_valid(int op, bool pm1, const OpCase& k) {
  if (k.d < 1 || k.d > 32767 || k.p < 0 || k.p > 32767 || k.nnz < 0 || k.nlong < 0 || k.nteam < 0 || k.n_out < 0 || k.n_outf < 0) return false;
  for (int i = 0; i < 4; ++i)
    if (k.n_in[i] < 0) return false;
  if (op == OP_BAND_H && (k.ldh < 1 || k.p < 1)) return false;
  if (op == OP_DENSE_H && (k.p < 1 || k.p > kDenseMaxP)) return false;
  if (op == OP_GRAD_DENSE && !(k.s[0] > 0.0)) return false;
  if ((op == OP_IPM_ITER || op == OP_IPM_LITE) && (k.n_seq < 0 || k.n_seq > 64 || k.ldh != (k.p | 1) || k.n_out < k.d + 2 * k.p + 3)) return false;
  if (op == OP_IPM_ITER && k.p > 32) return false;  // PMAX of BlockCtx<4>: the smallest of the contexts
  if (op_is_lite(op) && (k.p < 1 || k.p > kLiteMaxRows || k.d > kLiteMaxD || k.ldh < k.p)) return false;
  return op_lds_bytes(op, pm1, k) <= 160u * 1024u;
}

#if defined(CAVE_SIMT_EMUL)
// exact_step is CAVE_HD and takes a callable: driven on the host by a piecewise-linear phi' given as breakpoints
// (x ascending, phi'(x_j) = y_j, linear in between and extended by the end segments; phi'' = the segment's slope).
// trace[2 i] / trace[2 i + 1]: the i-th evaluation point and its phi' (n_trace slots), returns alpha
inline double exact_step_driver(const double* x, const double* y, int n, double psi0, double amax, int* n_eval) {
  int evals = 0;
  const double alpha = exact_step([&](double a, double& d1, double& d2) {
    int j = 0;
    while (j + 2 < n && a >= x[j + 1]) ++j;
    const double sl = (y[j + 1] - y[j]) / (x[j + 1] - x[j]);
    d1 = y[j] + sl * (a - x[j]);
    d2 = sl;
    ++evals;
  }, psi0, amax);
  if (n_eval) *n_eval = evals;
  return alpha;
}
#endif

}  // namespace cave_ops
