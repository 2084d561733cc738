// prim_entries.h — the linear solvers of the Newton loop, each callable ALONE (TEST INFRASTRUCTURE ONLY).
//
// One per-workgroup body per solver, written once and compiled twice: by g++ into the SIMT emulation build
// (tests/emul/simt_abi.cpp, CPU tier) and by hipcc into tests/prims/_prims.so (tests/prims/prims_abi.hip, GPU tier).
// A body copies one system of the batch into LDS in the layout the product uses, runs the product's solver on the
// product's workgroup shape (context type, wave count) and copies out what the solver wrote.  Nothing here is
// algorithm code: the solvers are the ones of cave_amd/csrc, untouched.  Never loaded by cave_amd.
//
// Include after cone_core.h / ctx_wave.h / ctx_block.h (cone_band.h and cone_dense.h come with cone_core.h).
// The model minimisation alone (lite_model_step / dense_model_step) is in model_entries.h, included below.
#pragma once
#include <stdint.h>

#include "../../cave_amd/csrc/cone_step.h"  // lite_scratch_doubles: what the product reserves for lite_model_step

namespace cave_prims {
using namespace cave;

struct PrimBatch {
  int64_t B;             // systems; one workgroup each
  int32_t p, nF, bw, n_ex;
  double reg_rel;
  const double* H;       // [B, h_stride]  full rows (ld = p) / packed triangle / folded triangle / band / tableau
  int64_t h_stride;
  const double* rhs;     // [B, p]
  const uint8_t* act;    // [B, p]  (entries that take it)
  const int32_t* ex;     // [n_ex]  pivots to exchange, in order (tableau)
  double* x;             // [B, p]  solution; dense: entries nF .. p-1 are INPUT (the bound rows' part)
  double* M;             // [B, m_stride]  matrix output: XS / factor / tableau
  int64_t m_stride;
  double* aux;           // [B, 2 p]  dense: dinv | z
  double* ws;            // [B, ws_stride]  global workspace (band: factor rows; cold band form: every work array)
  int64_t ws_stride;
  int32_t* fail;         // [B]  band wave form: the hand-over failure word; tableau: mask of refused exchanges
  // the model minimisation alone (model_entries.h); H: full rows (lite) / folded triangle in elimination order (dense)
  const double* theta;   // [B, p]  multipliers, reduced-row order
  const double* g;       // [B, p]  gradient, reduced-row order
  const uint16_t* ord;   // [B, p]  dense: reduced row at elimination position q (free rows at q < nF)
  double* tc;            // [B, p]  the trial point (poisoned by the caller)
  int32_t* moved;        // [B]     what the function returned (preset to -7)
  uint8_t* sact_out;     // [B, nI] dense: the held-at-zero flags the loop ended with
  double* ss_out;        // [B, nI] dense: the step of the last inner round (tc - ss: the working point it started from)
};

enum : int32_t {
  K_GJ = 0,         // gj_solve<64, false>            one wave
  K_GJ_LOWER = 1,   // gj_solve<64, true>             one wave, upper triangle never read
  K_GJS = 2,        // gj_solve_small<64, false>      = WaveCtx::solve_spd
  K_GJS_TRI = 3,    // gj_solve_small<64, true>       packed triangle
  K_SPD_B2 = 4,     // BlockCtx<2>::solve_spd
  K_SPD_B4 = 5,     // BlockCtx<4>::solve_spd         (p <= 32)
  K_SPD_L2 = 6,     // BlockCtx<2, true>::solve_spd
  K_SPD_L4 = 7,     // BlockCtx<4, true>::solve_spd   = gj_solve_wide_call<false>
  K_SPD_SOLO = 8,   // SoloCtx<32, 4>::solve_spd      = gj_solve_regs<8, true> (p <= 8)
  K_TRI_L4 = 9,     // BlockCtx<4, true>::solve_spd_tri = gj_solve_wide_call<true>
  K_TRI_B4 = 10,    // BlockCtx<4>::solve_spd_tri     (p <= 32)
  K_TRI_B2 = 11,    // BlockCtx<2>::solve_spd_tri
  K_PARTIAL = 12,   // gj_partial<32, true>           -> M = XS [p, nI], x = xg
  K_TABLEAU = 13,   // tableau_exchange<8, J>         H = T [8, 9] -> M
  K_DENSE_W2 = 14,  // dense_factor + dense_backsub on BlockCtx<2, true>
  K_DENSE_W4 = 15,  //                               on BlockCtx<4, true>
  K_BANDW1 = 16,    // solve_spd_band_wave<1>, materialised band
  K_BANDW2 = 17,    // solve_spd_band_wave<2>
  K_BAND_HOT_W1 = 18,   // solve_spd_band<WaveCtx, true>
  K_BAND_HOT_L2 = 19,   // solve_spd_band<BlockCtx<2, true>, true>
  K_BAND_HOT_L4 = 20,   // solve_spd_band<BlockCtx<4, true>, true>
  K_BAND_COLD_L4 = 21,  // solve_spd_band<BlockCtx<4, true>, false>: every work array in the global workspace
  K_LITE_MODEL = 22,      // lite_model_step on SoloCtx<32, 4>             H = full rows [p, p] -> M = H as left in LDS [p, p | 1]
  K_DENSE_MODEL_W1 = 23,  // dense_model_step on WaveCtx (cone_packed_large_kernel<Ctx1, 2>)
  K_DENSE_MODEL_W2 = 24,  //                  on BlockCtx<2, true>
  K_DENSE_MODEL_W4 = 25,  //                  on BlockCtx<4, true>
  K_COUNT = 26,
};

using SoloT = SoloCtx<32, 4>;
template <int KIND> struct PrimCtx { using type = WaveCtx; };
template <> struct PrimCtx<K_SPD_B2> { using type = BlockCtx<2>; };
template <> struct PrimCtx<K_SPD_B4> { using type = BlockCtx<4>; };
template <> struct PrimCtx<K_SPD_L2> { using type = BlockCtx<2, true>; };
template <> struct PrimCtx<K_SPD_L4> { using type = BlockCtx<4, true>; };
template <> struct PrimCtx<K_SPD_SOLO> { using type = SoloT; };
template <> struct PrimCtx<K_TRI_L4> { using type = BlockCtx<4, true>; };
template <> struct PrimCtx<K_TRI_B4> { using type = BlockCtx<4>; };
template <> struct PrimCtx<K_TRI_B2> { using type = BlockCtx<2>; };
template <> struct PrimCtx<K_DENSE_W2> { using type = BlockCtx<2, true>; };
template <> struct PrimCtx<K_DENSE_W4> { using type = BlockCtx<4, true>; };
template <> struct PrimCtx<K_BANDW2> { using type = BlockCtx<2, true>; };
template <> struct PrimCtx<K_BAND_HOT_L2> { using type = BlockCtx<2, true>; };
template <> struct PrimCtx<K_BAND_HOT_L4> { using type = BlockCtx<4, true>; };
template <> struct PrimCtx<K_BAND_COLD_L4> { using type = BlockCtx<4, true>; };
template <> struct PrimCtx<K_LITE_MODEL> { using type = SoloT; };
template <> struct PrimCtx<K_DENSE_MODEL_W2> { using type = BlockCtx<2, true>; };
template <> struct PrimCtx<K_DENSE_MODEL_W4> { using type = BlockCtx<4, true>; };

template <class C> struct CtxInfo { static constexpr uint32_t scratch = C::SCRATCH_BYTES; static constexpr int min_waves = C::MIN_WAVES_PER_EU; };
template <> struct CtxInfo<SoloT> { static constexpr uint32_t scratch = 0; static constexpr int min_waves = 2; };

constexpr bool kind_is_tri(int k) { return k == K_GJS_TRI || k == K_TRI_L4 || k == K_TRI_B4 || k == K_TRI_B2; }
constexpr bool kind_is_reg(int k) { return k <= K_TRI_B2; }
constexpr bool kind_is_band_team(int k) { return k >= K_BAND_HOT_W1 && k <= K_BAND_COLD_L4; }
constexpr bool kind_is_dense_model(int k) { return k >= K_DENSE_MODEL_W1 && k <= K_DENSE_MODEL_W4; }
constexpr int kind_threads(int k) {
  return (k == K_SPD_B4 || k == K_SPD_L4 || k == K_TRI_L4 || k == K_TRI_B4 || k == K_DENSE_W4 || k == K_BAND_HOT_L4 || k == K_BAND_COLD_L4 || k == K_DENSE_MODEL_W4) ? 256
       : (k == K_SPD_B2 || k == K_SPD_L2 || k == K_TRI_B2 || k == K_DENSE_W2 || k == K_BANDW2 || k == K_BAND_HOT_L2 || k == K_DENSE_MODEL_W2) ? 128 : 64;
}
// doubles lite_model_step indexes in w.ls_scr: XS [p * nI] and the nI multipliers behind it (lite_scratch_doubles of
// cone_step.h, what the product reserves, is never smaller)
CAVE_HOSTDEV uint32_t lite_model_scratch(int p, int nI) { return (uint32_t)(p * nI + nI); }
// bytes of the DenseWork arrays as model_entries.h lays them out (the order of cone_instance.h; A and scr on 16-byte
// boundaries), and the gap in front of them that makes the block end where dense_lds_bytes(p, nI) ends
CAVE_HOSTDEV uint64_t model_dense_used(int p, int nI) {
  const uint64_t P = (uint64_t)p, I = (uint64_t)nI, head = 8ull * fold_entries(p) + 24ull * P;
  return head + (head & 8u) + 8ull * dense_scratch_entries(p) + 8ull * I * (I | 1u) + 32ull * I + 4ull * P + I;
}
CAVE_HOSTDEV uint32_t model_dense_lead(int p, int nI) { return (uint32_t)((dense_lds_bytes(p, nI) - model_dense_used(p, nI)) & ~15ull); }
CAVE_HOSTDEV int kind_pmax(int k) {
  if (k == K_LITE_MODEL) return kLiteMaxRows;
  if (kind_is_dense_model(k)) return kDenseMaxP;
  if (k == K_SPD_SOLO) return 8;
  if (k == K_SPD_B4 || k == K_TRI_B4 || k == K_PARTIAL) return 32;
  if (k == K_TABLEAU) return 8;
  if (k == K_DENSE_W2 || k == K_DENSE_W4) return kDenseMaxP;
  if (k >= K_BANDW1) return 4096;
  return 64;
}
CAVE_HOSTDEV uint32_t up16(uint64_t n) { return (uint32_t)((n + 15u) & ~15ull); }
CAVE_HOSTDEV int64_t kind_h_entries(int k, int p, int bw) {
  if (k == K_LITE_MODEL) return (int64_t)p * p;
  if (kind_is_dense_model(k)) return fold_entries(p);
  if (k == K_TABLEAU) return 72;
  if (kind_is_tri(k)) return (int64_t)p * (p + 1) / 2;
  if (k == K_DENSE_W2 || k == K_DENSE_W4) return fold_entries(p);
  if (k >= K_BANDW1) return (int64_t)p * (bw + 1);
  return (int64_t)p * p;
}
// rows per staged chunk of the team form: band_chunk_rows<C> of cone_band.h (device code there), restated for the host
CAVE_HOSTDEV int band_team_ch(int k, int ld) {
  const int byregs = (16 * kind_threads(k)) / ld;
  return byregs < 32 ? byregs : 32;
}
// global workspace doubles per system
CAVE_HOSTDEV int64_t kind_ws_entries(int k, int p, int bw) {
  if (k < K_BANDW1 || k > K_BAND_COLD_L4) return 0;
  const int64_t ld = bw + 1;
  int64_t n = (int64_t)p * ld;  // factor rows
  if (k == K_BAND_COLD_L4) n += ld * ld + p + 2 * (int64_t)band_team_ch(k, (int)ld) * ld;
  return n;
}
// does the entry take this shape at all (the limits the product's dispatch guarantees)
CAVE_HOSTDEV bool kind_valid(int k, int p, int nF, int bw, int n_ex) {
  if (k < 0 || k >= K_COUNT || p < 1 || p > kind_pmax(k)) return false;
  if (k == K_PARTIAL) return nF >= 0 && nF <= p;
  if (k == K_LITE_MODEL) return nF >= 0 && nF <= p && p - nF <= 8 && lite_model_scratch(p, p - nF) <= lite_scratch_doubles(p, p - nF);
  if (kind_is_dense_model(k))
    return nF >= 0 && nF <= p && p - nF <= kDenseMaxBound && model_dense_used(p, p - nF) <= dense_lds_bytes(p, p - nF);
  if (k == K_TABLEAU) return p == 8 && n_ex >= 0;
  if (k == K_DENSE_W2 || k == K_DENSE_W4) return nF >= 0 && nF <= p && p - nF <= kDenseMaxBound;
  if (k == K_BANDW1 || k == K_BANDW2) return band_wave_fits(bw, p);
  if (kind_is_band_team(k)) return bw >= 1 && bw <= 64 && p >= bw + 1;
  return true;
}
// LDS of one workgroup: [context scratch | the arrays of the kind, 16-byte aligned each]
CAVE_HOSTDEV uint32_t kind_lds_bytes(int k, int p, int nF, int bw) {
  const uint64_t P = (uint64_t)p, h = (uint64_t)kind_h_entries(k, p, bw);
  uint64_t n = 256;
  if (kind_is_reg(k)) n += up16(8 * h) + 2 * up16(8 * P) + up16(P);
  else if (k == K_LITE_MODEL) n += up16(8 * P * (P | 1u)) + 5 * up16(8 * P) + up16(8ull * lite_model_scratch(p, p - nF));
  else if (kind_is_dense_model(k)) n += 3 * up16(8 * P) + model_dense_lead(p, p - nF) + model_dense_used(p, p - nF);
  else if (k == K_PARTIAL) n += up16(8 * h) + 2 * up16(8 * P) + up16(8 * P * (uint64_t)(p - nF) + 8);
  else if (k == K_TABLEAU) n += 0;
  else if (k == K_DENSE_W2 || k == K_DENSE_W4) n += up16(8 * h) + 3 * up16(8 * P) + up16(8ull * dense_scratch_entries(p));
  else if (k == K_BANDW1 || k == K_BANDW2) n += up16(8ull * band_wave_region(bw, p)) + 2 * up16(8 * P) + up16(P);
  else if (k == K_BAND_COLD_L4) n += 0;
  else if (kind_is_band_team(k)) {
    const uint64_t ld = (uint64_t)bw + 1;
    n += up16(8 * ld * ld) + 2 * up16(8 * P) + up16(8 * 2 * (uint64_t)band_team_ch(k, (int)ld) * ld) + up16(P);
  }
  return (uint32_t)n;
}

template <class C>
__device__ __forceinline__ C make_ctx(unsigned char* smem) {
  C c;
  if constexpr (std::is_same<C, SoloT>::value) c.lane = (int)threadIdx.x;
  else c.init(smem);
  return c;
}

struct Carve {  // hands out 16-byte aligned pieces of the workgroup's LDS behind the context scratch
  unsigned char* q;
  __device__ __forceinline__ explicit Carve(unsigned char* smem) : q(smem + 256) {}
  template <class T> __device__ __forceinline__ T* get(uint64_t n) {
    T* r = reinterpret_cast<T*>(q);
    q += up16(n * sizeof(T));
    return r;
  }
};

__device__ __forceinline__ double poison_f64() { return __hiloint2double(0x7ff80000, 0x00abcdef); }

}  // namespace cave_prims
#include "model_entries.h"
namespace cave_prims {

template <int KIND>
__device__ __forceinline__ void prim_body(unsigned char* smem, const PrimBatch& a, int64_t b) {
  using C = typename PrimCtx<KIND>::type;
  constexpr int NT = kind_threads(KIND);
  static_assert(NT == C::NT, "workgroup shape");
  C c = make_ctx<C>(smem);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = a.p, nF = a.nF, bw = a.bw;
  const int64_t hs = kind_h_entries(KIND, p, bw);
  const double* Hg = a.H + b * a.h_stride;
  const double* rg = a.rhs + b * p;
  Carve lds(smem);
  if constexpr (kind_is_reg(KIND)) {
    double* H = lds.get<double>((uint64_t)hs);
    double* rhs = lds.get<double>(p);
    double* dv = lds.get<double>(p);
    uint8_t* act = lds.get<uint8_t>(p);
    for (int64_t i = tid; i < hs; i += NT) H[i] = Hg[i];
    for (int i = tid; i < p; i += NT) { rhs[i] = rg[i]; dv[i] = poison_f64(); act[i] = a.act[b * p + i]; }
    __syncthreads();
    if constexpr (KIND == K_GJ) gj_solve<64, false>(lane, H, p, rhs, act, p, a.reg_rel, dv);
    else if constexpr (KIND == K_GJ_LOWER) gj_solve<64, true>(lane, H, p, rhs, act, p, a.reg_rel, dv);
    else if constexpr (KIND == K_GJS_TRI) gj_solve_small<64, true>(lane, H, 0, rhs, act, p, a.reg_rel, dv);
    else if constexpr (kind_is_tri(KIND)) c.solve_spd_tri(H, rhs, act, p, a.reg_rel, dv);
    else c.solve_spd(H, p, rhs, act, p, a.reg_rel, dv);
    __syncthreads();
    for (int i = tid; i < p; i += NT) a.x[b * p + i] = dv[i];
  } else if constexpr (KIND == K_PARTIAL) {
    const int nI = p - nF;
    double* H = lds.get<double>((uint64_t)hs);
    double* rhs = lds.get<double>(p);
    double* xg = lds.get<double>(p);
    double* XS = lds.get<double>((uint64_t)p * nI + 1);
    for (int64_t i = tid; i < hs; i += NT) H[i] = Hg[i];
    for (int i = tid; i < p; i += NT) { rhs[i] = rg[i]; xg[i] = poison_f64(); }
    for (int i = tid; i < p * nI; i += NT) XS[i] = poison_f64();
    __syncthreads();
    gj_partial<32, true>(lane, H, p, rhs, p, nF, a.reg_rel, XS, xg);
    __syncthreads();
    for (int i = tid; i < p; i += NT) a.x[b * p + i] = xg[i];
    for (int i = tid; i < p * nI; i += NT) a.M[b * a.m_stride + i] = XS[i];
  } else if constexpr (KIND == K_TABLEAU) {
    constexpr int NM = 8;
    double T[NM + 1];
#pragma unroll
    for (int j = 0; j <= NM; ++j) T[j] = lane < NM ? Hg[lane * (NM + 1) + j] : 0.0;
    int refused = 0;
    for (int e = 0; e < a.n_ex; ++e) {
      const int J = a.ex[e];  // (wave-uniform)
      static_for<0, NM>([&](auto jc) {
        constexpr int JJ = decltype(jc)::value;
        if (J == JJ)
          if (!tableau_exchange<NM, JJ>(T, lane)) refused |= 1 << JJ;
      });
    }
#pragma unroll
    for (int j = 0; j <= NM; ++j)
      if (lane < NM) a.M[b * a.m_stride + lane * (NM + 1) + j] = T[j];
    if (tid == 0) a.fail[b] = refused;
  } else if constexpr (KIND == K_DENSE_W2 || KIND == K_DENSE_W4) {
    DenseWork dw{};
    dw.on = true;
    dw.nF = nF; dw.nI = p - nF; dw.ldS = (p - nF) | 1;
    dw.A = lds.get<double>((uint64_t)hs);
    dw.dinv = lds.get<double>(p);
    dw.z = lds.get<double>(p);
    dw.x = lds.get<double>(p);
    dw.scr = lds.get<double>(dense_scratch_entries(p));
    for (int64_t i = tid; i < hs; i += NT) dw.A[i] = Hg[i];
    for (int i = tid; i < p; i += NT) {
      dw.z[i] = rg[i];
      dw.dinv[i] = poison_f64();
      dw.x[i] = i >= nF ? a.x[b * p + i] : poison_f64();
    }
    __syncthreads();
    dense_factor(c, dw, p, a.reg_rel, nF);
    __syncthreads();
    for (int64_t i = tid; i < hs; i += NT) a.M[b * a.m_stride + i] = dw.A[i];
    for (int i = tid; i < p; i += NT) { a.aux[b * 2 * p + i] = dw.dinv[i]; a.aux[b * 2 * p + p + i] = dw.z[i]; }
    __syncthreads();
    dense_backsub(c, dw, p, nF);
    __syncthreads();
    for (int i = tid; i < p; i += NT) a.x[b * p + i] = dw.x[i];
  } else if constexpr (KIND == K_LITE_MODEL) {
    model_lite_body<C>(smem, a, b);
  } else if constexpr (kind_is_dense_model(KIND)) {
    model_dense_body<C>(smem, a, b);
  } else if constexpr (KIND == K_BANDW1 || KIND == K_BANDW2) {
    constexpr int NW = KIND == K_BANDW1 ? 1 : 2;
    double* win = lds.get<double>(band_wave_region(bw, p));
    double* z = lds.get<double>(p);
    double* x = lds.get<double>(p);
    uint8_t* act = lds.get<uint8_t>(p);
    for (int i = tid; i < p; i += NT) { act[i] = a.act[b * p + i]; x[i] = poison_f64(); }
    int* words = reinterpret_cast<int*>(win + band_wave_flags_at(bw));
    if (tid == 0) words[4] = 0;  // the failure word (cone_instance.h clears it where it carves the region)
    __syncthreads();
    solve_spd_band_wave<NW>(lane, wave, Hg, bw, rg, act, p, a.reg_rel, win, a.ws + b * a.ws_stride, z, x, nullptr);
    __syncthreads();
    for (int i = tid; i < p; i += NT) a.x[b * p + i] = x[i];
    if (tid == 0) a.fail[b] = words[4];
  } else if constexpr (KIND == K_BAND_COLD_L4) {
    const int ld = bw + 1, CH = band_chunk_rows<C>(ld);
    double* w = a.ws + b * a.ws_stride;
    double* fac = w; w += (int64_t)p * ld;
    double* win = w; w += ld * ld;
    double* z = w; w += p;
    double* stg = w;
    solve_spd_band<C, false>(c, Hg, bw, rg, a.act + b * p, p, a.reg_rel, win, fac, z, a.x + b * p, stg, CH);
    __syncthreads();
  } else {
    const int ld = bw + 1, CH = band_chunk_rows<C>(ld);
    double* win = lds.get<double>((uint64_t)ld * ld);
    double* z = lds.get<double>(p);
    double* x = lds.get<double>(p);
    double* stg = lds.get<double>(2ull * CH * ld);
    uint8_t* act = lds.get<uint8_t>(p);
    for (int i = tid; i < p; i += NT) { act[i] = a.act[b * p + i]; x[i] = poison_f64(); }
    __syncthreads();
    solve_spd_band<C, true>(c, Hg, bw, rg, act, p, a.reg_rel, win, a.ws + b * a.ws_stride, z, x, stg, CH);
    __syncthreads();
    for (int i = tid; i < p; i += NT) a.x[b * p + i] = x[i];
  }
}

// X(kind) for every entry
#define CAVE_PRIM_KINDS(X) \
  X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) \
  X(22) X(23) X(24) X(25)

}  // namespace cave_prims
