// cone_step.h — the two halves of the fused "step" kernel (kernels.h cone_step_kernel) for small +-1 cones on the
// dense wire format (TSP-20, small grids: what the one-wave lite solver of cone_core.h takes).
//
// A training step on the reference's dense format is  scan + cone build (depends on the cones only)  ->  Newton solve
// + loss / gradient (needs the prediction).  The reference hands the cones of batch i+1 to the loop before the
// predictor has produced the prediction of batch i+1 (the DataLoader collates ahead, src/dataset.py:133-144), so the
// first half of batch i+1 can run beside the second half of batch i.  Here both halves sit in ONE grid:
//   blocks [0, B)            solve instance b of the CURRENT batch from a transient "lite store" (one wave each)
//   blocks [B, B + B_next)   pack instance b - B of the NEXT dense batch into the other lite store (four waves each)
// Blocks are dispatched in index order, so the solve waves take their SIMDs first and the pack workgroups fill what is
// left of each compute unit: no second stream, no event, no dependence on how the runtime maps streams to hardware
// queues (the side-stream form of rounds 2-3 needed a spacer kernel to win a dispatch race).
//
// The lite store holds, per instance, exactly what the one-wave solver reads, in the layout it reads it (the `ell` and
// `csr16` index structures of cone_core.h are built ONCE, by the pack half, instead of by every solve).
#pragma once
#include "../../include/cave_hip.h"
#include "cone_common.h"
#include "cone_core.h"
#include "cone_instance.h"

namespace cave {

static constexpr int kLiteHdr = 8;           // int32 words per slot: see cave_lite_store::hdr
static constexpr int kLiteCsrWords = 32 * kLiteMaxChunk;  // csr16 stride (uint32 words) per slot
static constexpr uint32_t kStepElectBytes = 64;           // head of the LDS block: words of the wave election

struct StepSolveParams {
  cave_lite_store store;
  const int64_t* ids;   // store slot of batch entry b (null: slot b -- the transient per-batch stores)
  const float* pred;
  int64_t B;
  int32_t mode;
  float sign, inner_ratio;
  int32_t max_iter;
  int32_t flags;        // CAVE_STEP_ZERO_FAILED: a failed instance gets loss 0 and a zero gradient instead of NaN / its last iterate
  OutPtrs o;
};

struct StepPackParams {
  const float* ctrs;
  int64_t B;
  int32_t m, d;
  uint32_t nnz_cap;
  cave_lite_store store;
  int32_t* status;
  uint64_t lite_pmax;   // lite_pmax_table(d): most reduced rows a cone with nI = 1 .. 8 bound rows may have (byte nI - 1)
};

// the pack half from the sparse wire format (cave_sparse_cones): a kernel argument of its own (cone_step_sparse_kernel)
struct StepSparsePackParams {
  const int64_t* ent_off;
  const uint32_t* key;
  const float* val;
  int64_t B;
  int32_t m, d;
  uint32_t nnz_cap;
  cave_lite_store store;
  int32_t* status;
  uint64_t lite_pmax;
};

// Multiplier cache of the warm solve half (cave_warm_cache, include/cave_hip.h): n entries of one 64-bit key and 32
// float multipliers each, grouped in sets of min(4, n) ways.  A key hashes to one set; lanes 0..ways-1 load the set's
// keys (ONE load) and lanes 0..31 the multipliers of all its ways beside them, so a hit costs no second round trip.
// Keys: caller keys (the store slot of a device-resident store) carry kWarmTagId, content keys (lite_content_key: the
// fingerprint of the cone + p, nF, non-zeros) kWarmTagContent; 0 = empty.  Plain loads and stores,
// no atomics: a torn or stale entry is a worse starting point, never a wrong result (solve_cone_impl sanitises it and
// the projection is unique).
struct StepWarm {
  uint64_t* key;         // [n]
  float* theta;          // [n * 32]
  int64_t n;             // entries (a power of two); the cold kernel never reads this block
  const int64_t* keys;   // [B] caller keys, or null: the key comes from the slot's content
  uint8_t* hit;          // [B] 1 where the instance started from cached multipliers, or null
  uint32_t lds_extra;    // LDS bytes at the end of the launch's block kept out of both arenas (the arenas stay those of
                         // the cold launch): the LDS copy of a hit's multipliers.  0: taken from the solve arena if room
};
static constexpr uint64_t kWarmTagContent = 1ull << 63, kWarmTagId = 1ull << 62;

struct StepParams {
  StepSolveParams S;
  StepPackParams Q;
  uint32_t lds_bytes;   // dynamic LDS of the launch (both halves size their arenas from it)
  uint32_t* tickets;    // [4096] per-compute-unit SIMD claim masks of the wave election (caller-owned, zeroed once)
};
// the warm variant's kernel argument (cone_step_kernel<CP, true>): the cold one keeps its own as it was
struct StepParamsWarm : StepParams {
  StepWarm W;
};
// the same pair for a NEXT batch on the sparse wire format (cone_step_sparse_kernel): the solve half is the dense
// kernels' (it reads only the lite store), the pack half copies the coordinate list instead of scanning a dense block
struct StepSparseParams {
  StepSolveParams S;
  StepSparsePackParams Q;
  uint32_t lds_bytes;
  uint32_t* tickets;
};
struct StepSparseParamsWarm : StepSparseParams {
  StepWarm W;
};

// ---- fingerprint of the cone in a lite slot: a sum (mod 2^32) of one mixed term per (position, word) of the row
// pointers and the csr16 words (what defines the reduced rows), the sign bytes of the unit rows and the count of rows
// the projection keeps, so the per-lane partial sums may be combined in any order.  Neither the batch position nor the zero padding of the dense block (m_max) enters.  The warm solve half forms
// it from the words its prologue loads anyway; the pack half (shared with the cold kernel) does not pay for it.
CAVE_HOSTDEV uint32_t lite_fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
CAVE_HOSTDEV uint32_t lite_fp_term(uint32_t pos, uint32_t word) { return lite_fmix32(word ^ lite_fmix32(pos * 0x9e3779b1u + 0x7f4a7c15u)); }
// positions of the hashed words: csr16 words 0 .. 767, row pointers, sign bytes, rows kept by the projection
static constexpr uint32_t kLiteFpRowPos = 1u << 20, kLiteFpSignPos = 2u << 20, kLiteFpValidPos = 3u << 20;
// the cache key of a slot: fingerprint, p, nF, non-zeros (p, nF <= 32; non-zeros <= 1536)
CAVE_HOSTDEV uint64_t lite_content_key(uint32_t fp, int p, int nF, uint32_t nnz) {
  return kWarmTagContent | ((uint64_t)fp << 26) | ((uint64_t)(p & 63) << 20) | ((uint64_t)(nF & 63) << 14) | (uint64_t)(nnz & 0x3fffu);
}
CAVE_HOSTDEV uint64_t warm_mix64(uint64_t x) {  // (splitmix64 finaliser: set index of a key)
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
  return x;
}

// LDS one solve block needs for cost dimension d (reduced systems of up to 32 rows, up to 1536 non-zeros)
static inline uint32_t step_solve_lds_bytes(int64_t d) {
  const uint64_t p = kLiteMaxRows;
  uint64_t s = kStepElectBytes;
  s += 2 * align8u(4 * d) + align8u(d) + align8u(4 * (p + 1)) + align8u(p);   // y, avg, usign, mptr, vkind
  s += 16 + 16 * (uint64_t)d + 16 + 4 * (uint64_t)kLiteCsrWords + 8 * (33 + 64 + 65) + 40;  // ell, csr16, rs, rl
  s += 2 * align8u(8 * d) + align8u(8 * (d + 1)) + align8u(4 * d);             // res, tvec, rc, wold
  s += 2 * 8 * 33 + 5 * align8u(8 * p) + align8u(8 * p * (p | 1)) + align8u(p) + 64;  // theta, dv, 5 vectors, H, act
  return (uint32_t)((s + 255u) & ~255ull);
}

// Scratch of lite_model_step (cone_core.h) for p reduced rows of which nI have bounds, in doubles: XS [p * nI],
// S [nI * (nI | 1)], four vectors of nI, flags
CAVE_HOSTDEV uint32_t lite_scratch_doubles(int p, int nI) { return (uint32_t)(p * nI + nI * (nI | 1) + 4 * nI + (nI + 7) / 8); }

// Does the solve half find that scratch for a cone of p reduced rows, nI of them with bounds?  It takes the epilogue's
// target vector (d doubles, idle while the solver runs) when that is big enough, else a block of its own behind its
// other arrays -- and step_solve_lds_bytes has no term for such a block: what is there is what the arrays sized by p
// leave of their p = 32 figures.  The smallest arena a solve can meet is that of a launch without a pack half
// (step_solve_lds_bytes(d): a fused launch has max(pack, solve)), so the allocations of run_lite_instance are replayed
// against it here, for the mode that allocates most (INNER: the average normal too) and 24 csr16 entries per lane.
// write_lite_slot refuses a cone that fails this (its slot says -1 and the host takes the general operator), so a slot
// that says 1 is solved by every launch form.  At d = 256: p = 32 with up to 5 bound rows, p <= 31 with 6, p <= 28
// with 7, p <= 27 with 8.  Host code: the kernels get the rule as a table (lite_pmax_table), one compare per cone.
static inline bool lite_scratch_fits(int d, int p, int nI) {
  const uint32_t need = lite_scratch_doubles(p, nI);
  if (need <= (uint32_t)d) return true;
  const uint32_t pp = (uint32_t)(p > 0 ? p : 1), ud = (uint32_t)d;
  uint32_t off = 0;
  auto take = [&off](uint32_t bytes, uint32_t align) { off = ((off + align - 1u) & ~(align - 1u)) + bytes; };
  take(4u * ud, 8u); take(4u * ud, 8u); take(ud, 8u); take(4u * (pp + 1u), 8u); take(pp, 8u);   // y, avg, usign, mptr, vkind
  take(16u * ud, 16u); take(4u * (uint32_t)kLiteCsrWords, 16u); take(8u * (33u + 64u + 65u), 8u); take(40u, 8u);  // ell, csr16, rs, rl
  take(8u * ud, 8u); take(8u * ud, 8u); take(8u * (ud + 1u), 8u); take(4u * ud, 8u);            // res, tvec, rc, wold
  take(8u * 33u, 8u); take(8u * 33u, 8u);                                                        // theta, dv
  for (int i = 0; i < 5; ++i) take(8u * pp, 8u);                                                 // ttry, told, g, g2, step
  take(8u * (uint32_t)(p > 0 ? p * (p | 1) : 1), 8u); take(pp, 8u);                              // H, act
  take(8u * need, 8u);
  return off <= ((step_solve_lds_bytes(d) - kStepElectBytes) & ~7u);
}

// The rule as the kernels read it (StepPackParams / LiteFromPackedParams::lite_pmax): byte nI - 1 holds the most reduced
// rows a cone with nI bound rows may have at dimension d (the need grows with p, so the accepted p are an interval from
// nI up; 0 = none).  A cone without bound rows needs no scratch.
// (Evaluated once per process for every d: a launch costs a table look-up on the host.)
struct LitePmaxTables {
  uint64_t t[kLiteMaxD + 1];
  LitePmaxTables() {
    t[0] = 0;
    for (int d = 1; d <= kLiteMaxD; ++d) {
      uint64_t x = 0;
      for (int nI = 1; nI <= 8; ++nI) {
        int pmax = 0;
        for (int p = nI; p <= kLiteMaxRows && lite_scratch_fits(d, p, nI); ++p) pmax = p;
        x |= (uint64_t)pmax << (8 * (nI - 1));
      }
      t[d] = x;
    }
  }
};
static inline uint64_t lite_pmax_table(int d) {
  static const LitePmaxTables tabs;
  return d >= 1 && d <= kLiteMaxD ? tabs.t[d] : 0;
}
CAVE_HOSTDEV bool lite_pmax_allows(uint64_t table, int p, int nI) {
  return nI == 0 || p <= (int)((table >> (8 * (nI - 1))) & 0xffu);
}

// Launch limits of the fused step for dense batches of shape (m_max, d) (m_max = 0: a launch without a pack half -- the
// lite slots of a device-resident store): non-zeros kept per instance by the pack half and the dynamic LDS per
// workgroup; CAVE_E_INVALID when the shape does not qualify.  Host code (cave_hip.hip and the emulation build of
// tests/emul size their launches from this one function).
static inline int32_t step_limits(int64_t m_max, int64_t d, int32_t& cap, int32_t& lds) {
  if (m_max < 0 || d <= 0 || d > kLiteMaxD || m_max > 32767) return CAVE_E_INVALID;
  cap = 0;
  uint64_t pack_lds = 0;
  if (m_max > 0) {
    // non-zeros kept per instance: structured cones carry <= d unit entries + a few sparse rows (cone_instance.h
    // default_limits); the arena of the two-wave pack half: no dump slots behind the scan output, no prediction
    int64_t c = 4 * (m_max + d) + 128;
    if (c > m_max * d) c = m_max * d;
    if (c < 64) c = 64;
    cap = (int32_t)c;
    pack_lds = arena_bytes_dense(m_max, d, c, 64, 32, c * 6 / 10, 0, true, false) - align8u(4 * d);
  }
  const uint32_t solve_lds = step_solve_lds_bytes(d);
  uint32_t need = pack_lds > solve_lds ? (uint32_t)pack_lds : solve_lds;
  need = (need + 255u) & ~255u;
  // four solve blocks + two pack blocks per compute unit: the fused form only pays when six workgroups fit
  // (a launch without a pack half -- m_max = 0: the lite slots of a device-resident store -- needs four)
  if ((uint64_t)need * (m_max > 0 ? 6u : 4u) > kMaxLds) return CAVE_E_INVALID;
  lds = (int32_t)need;
  return CAVE_OK;
}

// LDS bytes the warm variant adds behind both arenas of a launch of `lds` bytes per workgroup (the LDS copy of a hit's
// multipliers, StepWarm::lds_extra): 256 when the launch keeps its residency with them -- six workgroups per compute
// unit with a pack half, four without --, else 0 (the copy is then taken from the solve arena if there is room)
static inline uint32_t step_warm_lds_extra(uint32_t lds, bool has_pack) {
  const uint32_t extra = 256u;
  return (uint64_t)(lds + extra) * (has_pack ? 6u : 4u) <= kMaxLds ? extra : 0u;
}

// dynamic LDS of one workgroup of lite_from_packed_kernel (cost dimension d; any cone the lite solver takes)
static inline uint32_t lite_from_packed_lds_bytes(int64_t d) {
  const uint64_t lds = 256 + 64 + align8u(4 * d) + align8u(d) + align8u(4 * (d + 1)) + align8u(4 * (kLiteMaxRows + 1)) + 64 +
                       2 * align8u(2 * 64 * kLiteMaxChunk) + lite_lds_bytes((int)d, 64u * kLiteMaxChunk) + 64;
  return (uint32_t)lds;
}

// -------------------------------------------------------------------------------------------------- pack half
// Eligibility + lite index structures of one cone (SolveView in LDS, `avg` its average normal) -> slot `slot` of the
// lite store.  hdr[0] = 1: the slot holds a cone the one-wave solver takes;  -1: it does not (not +-1, more than 32
// reduced rows / 8 entries per column / 8 bound rows, rows not ordered [free | bound], no room in the arena, or no room
// for the active-set scratch in the solve half's arena: lite_scratch_fits): the
// solve half reports CAVE_ST_TOO_LARGE for it and the host falls back to the general operator.  Returns the state.
template <class C>
CAVE_HD int32_t write_lite_slot(C& c, Arena& ar, const SolveView& v, const float* avg, uint32_t nnzM, const cave_lite_store& S,
                                int64_t slot, uint64_t lite_pmax) {
  const int NT = C::NT;
  const int d = v.d, p = v.p;
  int nF = 0;
  bool ok = v.pm1 && p <= kLiteMaxRows && d <= kLiteMaxD;
  LiteCone L;
  L.ell = nullptr; L.csr16 = nullptr; L.rs = nullptr; L.rl = nullptr; L.chn8 = 0; L.cmax = 0;
  if (ok && p > 0) {
    uint32_t nfree = 0, bad = 0;
    for (int i = c.tid(); i < p; i += NT) nfree += v.vkind[i] ? 1u : 0u;
    nfree = c.reduce_add_u32(nfree);
    for (int i = c.tid(); i < p; i += NT) bad += ((v.vkind[i] != 0) != (i < (int)nfree)) ? 1u : 0u;
    bad = c.reduce_add_u32(bad);
    const int nI = p - (int)nfree;
    ok = bad == 0u && nI <= 8 && lite_pmax_allows(lite_pmax, p, nI);  // (a slot that says 1 is one every launch form solves)
    nF = (int)nfree;
    if (ok) ok = lite_build(c, ar, v, L);
  }
  if (ok) {
    for (int k = c.tid(); k < d; k += NT) {
      S.usign[slot * d + k] = v.usign[k];
      S.avg[slot * d + k] = avg[k];
    }
    for (int i = c.tid(); i <= p; i += NT) S.rowptr[slot * (kLiteMaxRows + 1) + i] = v.mptr[i];
    if (p > 0) {
      // 16-byte copies: both structures are 16-byte aligned in LDS and in the store
      const uint4* e4 = reinterpret_cast<const uint4*>(L.ell);
      uint4* eo = reinterpret_cast<uint4*>(S.ell + slot * 4 * (int64_t)d);
      for (int k = c.tid(); k < d; k += NT) eo[k] = e4[k];
      const uint4* c4 = reinterpret_cast<const uint4*>(L.csr16);
      uint4* co = reinterpret_cast<uint4*>(S.csr16 + slot * (int64_t)kLiteCsrWords);
      for (int k = c.tid(); k < 8 * L.chn8; k += NT) co[k] = c4[k];
      for (int i = c.tid(); i < p; i += NT) S.rl[slot * kLiteMaxRows + i] = L.rl[i];
    }
  }
  if (c.tid() == 0) {
    int32_t* h = S.hdr + slot * kLiteHdr;
    h[0] = ok ? 1 : -1;
    h[1] = ok ? p : 0;
    h[2] = ok ? (int32_t)nnzM : 0;
    h[3] = nF;
    h[4] = ok ? v.n_valid : 0;
    h[5] = L.cmax;
    h[6] = L.chn8;
    h[7] = 0;
  }
  return ok ? 1 : -1;
}

// scan + cone build (as run_pack_instance), then the lite slot
template <class C>
CAVE_HD void run_pack_lite_instance(C& c, unsigned char* smem, uint32_t lds_bytes, const StepPackParams& P, int64_t b) {
  const int d = P.d, m = P.m;
  Arena ar;
  ar.init(smem + C::SCRATCH_BYTES, lds_bytes - C::SCRATCH_BYTES);
  ConeBuild cb;
  CAVE_T0();
  int32_t st = scan_and_build<C, false, true>(c, ar, cb, P.ctrs + b * (int64_t)m * d, m, d, P.nnz_cap);
  CAVE_ACC(0);
  const cave_lite_store& S = P.store;
  float* avg = (st == ST_OK) ? ar.get<float>(d) : nullptr;
  if (st == ST_OK && ar.ovf) st = ST_TOO_LARGE;
  if (st == ST_OK) {
    compute_avg(c, cb, avg);
    ar.release_top();  // build-phase temporaries are dead now
    const SolveView v = view_of(cb);
    if (write_lite_slot(c, ar, v, avg, cb.nnzM, S, b, P.lite_pmax) != 1) st = ST_TOO_LARGE;
  } else if (c.tid() == 0) {
    int32_t* h = S.hdr + b * kLiteHdr;
    h[0] = -1;
    for (int i = 1; i < kLiteHdr; ++i) h[i] = 0;
  }
  CAVE_ACC(1);
  if (c.tid() == 0 && P.status) P.status[b] = st;
}

// Twin of run_pack_lite_instance for one instance of the sparse wire format: load_sparse_and_build in its DEEP form
// (the reservations of scan_and_build<C, false, true>: the same arena from the same step_limits LDS and nnz_cap) is
// the producer, everything after it is the same text.  From the same non-zeros build_cone therefore sees the same
// input in the same arena, and the slot holds the same bits and the same TOO_LARGE verdicts as on the dense route.
// A twin and not a shared tail: the code objects of the dense step kernels stay as they are.  A
// contract-breaking entry: ST_BAD_INPUT in `status`, slot state -1.
template <class C>
CAVE_HD void run_pack_sparse_lite_instance(C& c, unsigned char* smem, uint32_t lds_bytes, const StepSparsePackParams& P, int64_t b) {
  const int d = P.d, m = P.m;
  Arena ar;
  ar.init(smem + C::SCRATCH_BYTES, lds_bytes - C::SCRATCH_BYTES);
  ConeBuild cb;
  CAVE_T0();
  const int64_t e0 = P.ent_off[b];
  int32_t st = load_sparse_and_build<C, false, true>(c, ar, cb, P.key + e0, P.val + e0, P.ent_off[b + 1] - e0, m, d, P.nnz_cap);
  CAVE_ACC(0);
  const cave_lite_store& S = P.store;
  float* avg = (st == ST_OK) ? ar.get<float>(d) : nullptr;
  if (st == ST_OK && ar.ovf) st = ST_TOO_LARGE;
  if (st == ST_OK) {
    compute_avg(c, cb, avg);
    ar.release_top();  // build-phase temporaries are dead now
    const SolveView v = view_of(cb);
    if (write_lite_slot(c, ar, v, avg, cb.nnzM, S, b, P.lite_pmax) != 1) st = ST_TOO_LARGE;
  } else if (c.tid() == 0) {
    int32_t* h = S.hdr + b * kLiteHdr;
    h[0] = -1;
    for (int i = 1; i < kLiteHdr; ++i) h[i] = 0;
  }
  CAVE_ACC(1);
  if (c.tid() == 0 && P.status) P.status[b] = st;
}

// One instance of a packed cone store (cave_cone_store) -> its lite slot: cones are static per instance
// (src/dataset.py:72), so a device-resident store builds the solver's index structures ONCE, when it is created.
struct LiteFromPackedParams {
  cave_cone_store src;
  cave_lite_store dst;
  int64_t n;
  uint32_t lds_bytes;
  int32_t* status;
  uint64_t lite_pmax;   // lite_pmax_table(src.d)
};
template <class C>
CAVE_HD void run_lite_from_packed(C& c, unsigned char* smem, const LiteFromPackedParams& P, int64_t slot) {
  const cave_cone_store& S = P.src;
  const int d = S.d, NT = C::NT;
  Arena ar;
  ar.init(smem + C::SCRATCH_BYTES, P.lds_bytes - C::SCRATCH_BYTES);
  const int64_t r0 = S.row_off[slot], z0 = S.nnz_off[slot];
  const int p = S.n_rows ? (int)S.n_rows[slot] : (int)(S.row_off[slot + 1] - r0);
  const uint32_t nz = S.n_nnz ? (uint32_t)S.n_nnz[slot] : (uint32_t)(S.nnz_off[slot + 1] - z0);
  const bool pm1 = (S.flags[slot] & 1) != 0;
  int32_t state = -1;
  if (p >= 0 && p <= kLiteMaxRows && pm1 && d <= kLiteMaxD && nz <= 64u * (uint32_t)kLiteMaxChunk) {
    float* avg = ar.get<float>(d);
    uint8_t* usign = ar.get<uint8_t>(d);
    uint32_t* cptr = ar.get<uint32_t>(d + 1);
    uint32_t* mptr = ar.get<uint32_t>((uint32_t)p + 1u);
    uint8_t* vkind = ar.get<uint8_t>(p > 0 ? p : 1);
    uint16_t* mcol = ar.get<uint16_t>(nz > 0 ? nz : 1);
    uint16_t* cvar = ar.get<uint16_t>(nz > 0 ? nz : 1);
    if (!ar.ovf) {
      for (int k = c.tid(); k < d; k += NT) { avg[k] = S.avg[slot * d + k]; usign[k] = S.usign[slot * d + k]; }
      for (int k = c.tid(); k <= d; k += NT) cptr[k] = S.cptr[slot * (d + 1) + k];
      for (int i = c.tid(); i < p; i += NT) { mptr[i] = S.rlo[r0 + i]; vkind[i] = S.vkind[r0 + i]; }
      if (c.tid() == 0) mptr[p] = nz;
      for (uint32_t e = c.tid(); e < nz; e += NT) {  // sign into bit 15, as the LDS-resident solvers keep +-1 cones
        mcol[e] = (uint16_t)((S.ccol[z0 + e] & 0x7fffu) | (S.cval[z0 + e] < 0.f ? 0x8000u : 0u));
        cvar[e] = (uint16_t)((S.cvar[z0 + e] & 0x7fffu) | (S.cvalc[z0 + e] < 0.f ? 0x8000u : 0u));
      }
      c.sync();
      SolveView v;
      v.d = d; v.p = p; v.n_valid = S.n_valid[slot]; v.pm1 = true;
      v.mptr = mptr; v.mcol = mcol; v.mval = nullptr; v.vkind = vkind;
      v.cptr = cptr; v.cvar = cvar; v.cvalc = nullptr; v.usign = usign;
      v.nlong = 0; v.longrow = nullptr;
      state = write_lite_slot(c, ar, v, avg, nz, P.dst, slot, P.lite_pmax);
    }
  }
  if (state != 1 && c.tid() == 0) {
    int32_t* h = P.dst.hdr + slot * kLiteHdr;
    h[0] = -1;
    for (int i = 1; i < kLiteHdr; ++i) h[i] = 0;
  }
  if (c.tid() == 0 && P.status) P.status[slot] = state == 1 ? ST_OK : ST_TOO_LARGE;
}

// ------------------------------------------------------------------------------------------------- solve half
#if defined(CAVE_GPU_CODE)
// One wave: load slot b of the lite store into LDS (every load of the prologue is issued before the first store:
// one memory round trip), run the one-wave Newton solver, fused epilogue.  `lane`: 0..63.
// WARM: the multiplier cache W (StepWarm) is probed before the solve and written back after it; an instance that does not
// hit runs exactly the cold instructions from the same state (w.warm = null).
// IPM: the interior-point variant (k_step_ipm.hip, k_step_sparse_ipm.hip): the instance runs P.max_iter steps of
// lite_solve_ipm (cone_core.h) instead of the Newton solver, for MODE_IPM only -- no cache, no average normal, none of
// lite_model_step's scratch.  The cold and warm instantiations refuse that mode (CAVE_ST_TOO_LARGE) as before.
template <class SC, bool WARM = false, bool IPM = false>
CAVE_HD void run_lite_instance(SC& sc, unsigned char* smem, uint32_t lds_bytes, const StepSolveParams& P, int64_t b,
                               const StepWarm& W) {
  const cave_lite_store& S = P.store;
  const int d = S.d;
  const int lane = sc.lane;
  Arena ar;
  ar.init(smem, lds_bytes);
  int32_t st = ST_OK;
  int iters = 0;
  bool whit = false;  // (warm variant: the solve started from cached multipliers)
  const int64_t slot_raw = P.ids ? P.ids[b] : b;
  const bool in_range = slot_raw >= 0 && slot_raw < S.n;
  const int64_t slot = in_range ? slot_raw : 0;
  static_assert(!(WARM && IPM), "the interior iterate is not a starting point: the IPM variant has no cache");
  const int mode = P.mode;
  const bool need_avg = !IPM && (mode == MODE_INNER || mode == MODE_HEURISTIC || mode == MODE_AVG);
  const bool need_proj = IPM || (mode == MODE_PROJECT || mode == MODE_EXACT || mode == MODE_INNER);
  // ---- prologue: EVERY global load of the instance in one memory round trip -- the header words beside the arrays
  // (nothing below depends on them: a slot's arrays have fixed extents, what a cone does not use is loaded and dropped);
  // until round 4 the header came first and the arrays a latency later (~2 us of a 70 us instance)
  constexpr int KC = (kLiteMaxD + 63) / 64;  // coordinates per lane
  float yv[KC], av[KC];
  uint4 ev[KC];
  uint8_t uv[KC];
#pragma unroll
  for (int s = 0; s < KC; ++s) {
    const int k = lane + 64 * s, kc = k < d ? k : d - 1;
    yv[s] = P.pred ? P.pred[b * d + kc] : 0.f;
    uv[s] = S.usign[slot * d + kc];
    av[s] = need_avg ? S.avg[slot * d + kc] : 0.f;
    ev[s] = need_proj ? reinterpret_cast<const uint4*>(S.ell + slot * 4 * (int64_t)d)[kc] : make_uint4(0, 0, 0, 0);
  }
  uint4 cv[kLiteMaxChunk / 8];
#pragma unroll
  for (int g8 = 0; g8 < kLiteMaxChunk / 8; ++g8)
    cv[g8] = need_proj ? reinterpret_cast<const uint4*>(S.csr16 + slot * (int64_t)kLiteCsrWords)[g8 * 64 + lane] : make_uint4(0, 0, 0, 0);
  const uint32_t mp_raw = (need_proj && lane <= kLiteMaxRows) ? S.rowptr[slot * (kLiteMaxRows + 1) + lane] : 0u;
  const uint8_t rl_raw = (need_proj && lane < kLiteMaxRows) ? S.rl[slot * kLiteMaxRows + lane] : (uint8_t)0;
  const int32_t* hdr = S.hdr + slot * kLiteHdr;
  const int32_t hv = lane < kLiteHdr ? hdr[lane] : 0;  // (one load; the words are handed out below)
  const int32_t state = in_range ? __builtin_amdgcn_readlane(hv, 0) : 0;
  const int p = __builtin_amdgcn_readlane(hv, 1), nF = __builtin_amdgcn_readlane(hv, 3), n_valid = __builtin_amdgcn_readlane(hv, 4);
  const int cmax = __builtin_amdgcn_readlane(hv, 5), chn8 = __builtin_amdgcn_readlane(hv, 6);
  if (!in_range) st = ST_BAD_INPUT;
  // (the mode test is a ternary on the template constant: the front end folds it, and the cold and warm kernels keep the
  //  instructions they had when the test read `mode == MODE_IPM`)
  else if (state != 1 || p < 0 || p > kLiteMaxRows || chn8 > kLiteMaxChunk || (IPM ? mode != MODE_IPM : mode == MODE_IPM)) st = ST_TOO_LARGE;
  else {
    const uint32_t pp = (uint32_t)(p > 0 ? p : 1);
    float* y = ar.get<float>(d);
    float* avg = need_avg ? ar.get<float>(d) : nullptr;
    uint8_t* usign = ar.get<uint8_t>(d);
    uint32_t* mptr = ar.get<uint32_t>(pp + 1u);
    uint8_t* vkind = ar.get<uint8_t>(pp);
    uint32_t* ell = ar.try_get<uint32_t, 16u>(4u * (uint32_t)d);
    uint32_t* csr16 = ar.try_get<uint32_t, 16u>(32u * (uint32_t)(chn8 > 0 ? chn8 : 8));
    double* rs = ar.get<double>(33u + 64u + 65u);
    uint8_t* rl = ar.get<uint8_t>(40u);
    double* res = ar.get<double>(d);
    double* tvec = ar.get<double>(d);
    SolveWork w;
    w.y = y;
    w.res = res;
    w.q = tvec;
    w.rc = ar.get<double>((uint32_t)d + 1u);
    w.wold = ar.get<float>(d);
    w.theta = ar.get<double>(33u);
    w.dv = ar.get<double>(33u);
    w.ttry = ar.get<double>(pp);
    w.told = ar.get<double>(pp);
    w.g = ar.get<double>(pp);
    w.g2 = ar.get<double>(pp);
    w.step = ar.get<double>(pp);
    w.ldh = p | 1;
    w.H = ar.get<double>((uint32_t)(p > 0 ? p * w.ldh : 1));
    w.act = ar.get<uint8_t>(pp);
    // ---- warm variant: probe the cache (the set's keys and the multipliers of all its ways in one round trip)
    bool wact = false, wmatch = false;
    int64_t went = 0;
    uint64_t wkey = 0;
    float wsel = 0.f;
    if constexpr (WARM) {
      const int64_t kraw = W.keys ? W.keys[b] : 0;
      if (W.keys) wkey = kraw >= 0 ? ((uint64_t)kraw | kWarmTagId) : 0ull;
      else {
        // content key: the fingerprint of the slot's row pointers and csr16 words, from the registers the prologue
        // loaded them into (what lies beyond the cone's own extents is not hashed: a slot is reused across batches)
        uint32_t fpl = lane <= p ? lite_fp_term(kLiteFpRowPos + (uint32_t)lane, mp_raw) : 0u;
        // ... and the sign bytes of the unit rows and the rows the projection keeps: cones of one problem often share
        // their reduced rows (the TSP degree rows) and differ only in which coordinates are at a bound
#pragma unroll
        for (int s = 0; s < KC; ++s)
          if (lane + 64 * s < d) fpl += lite_fp_term(kLiteFpSignPos + (uint32_t)(lane + 64 * s), uv[s]);
        if (lane == 0) fpl += lite_fp_term(kLiteFpValidPos, (uint32_t)n_valid);
#pragma unroll
        for (int g8 = 0; g8 < kLiteMaxChunk / 8; ++g8)
          if (g8 * 8 < chn8) {
            const uint32_t q = 4u * (uint32_t)(g8 * 64 + lane);
            fpl += lite_fp_term(q, cv[g8].x) + lite_fp_term(q + 1u, cv[g8].y) + lite_fp_term(q + 2u, cv[g8].z) +
                   lite_fp_term(q + 3u, cv[g8].w);
          }
        wkey = lite_content_key(sc.reduce_add_u32(fpl), p, nF, (uint32_t)__builtin_amdgcn_readlane(hv, 2));
      }
      wact = need_proj && p > 0 && n_valid > 0 && wkey != 0ull;
      if (wact) {
        const int ways = W.n < 4 ? (int)W.n : 4;
        // set and home way: caller keys (store slots: dense from 0) map directly -- slot k to way k % ways of set k / ways,
        // so n slots never collide in a cache of n entries or more; content keys are hashed
        const uint64_t mix = W.keys ? (((uint64_t)kraw / (uint64_t)ways) | ((uint64_t)kraw % (uint64_t)ways) << 32) : warm_mix64(wkey);
        const int64_t base = (int64_t)(mix & (uint64_t)(W.n / ways - 1)) * ways;
        const uint64_t kl = lane < ways ? W.key[base + lane] : 0ull;
        float wt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wt[j] = (lane < 32 && j < ways) ? W.theta[(base + j) * 32 + lane] : 0.f;
        const uint64_t hitm = __ballot(lane < ways && kl == wkey), freem = __ballot(lane < ways && kl == 0ull);
        // a miss takes the first free way from the key's own "home" way on (keys of one set that miss in the same launch
        // see the same free ways: starting from way 0 they would all take the same one, and all but one be lost), a full
        // set loses its home way
        const uint32_t home = (uint32_t)(mix >> 32) & (uint32_t)(ways - 1), wmask = (1u << ways) - 1u;
        int way;
        if (hitm) { wmatch = true; way = __ffsll((unsigned long long)hitm) - 1; }
        else if (freem) {
          const uint32_t f = (uint32_t)freem & wmask, rot = ((f >> home) | (f << (ways - home))) & wmask;
          way = (int)((home + (uint32_t)(__ffs(rot) - 1)) & (uint32_t)(ways - 1));
        } else way = (int)home;
        went = base + way;
#pragma unroll
        for (int j = 0; j < 4; ++j) wsel = j == way ? wt[j] : wsel;
      }
    }
    if (ar.ovf || !ell || !csr16) st = ST_TOO_LARGE;
    else {
      // ---- the LDS stores of what the prologue loaded
      const uint32_t mp = lane <= p ? mp_raw : 0u;
      const uint8_t rlv = lane < p ? rl_raw : (uint8_t)0;
#pragma unroll
      for (int s = 0; s < KC; ++s) {
        const int k = lane + 64 * s;
        if (k < d) {
          y[k] = P.sign * yv[s];
          usign[k] = uv[s];
          if (need_avg) avg[k] = av[s];
          if (need_proj && p > 0) reinterpret_cast<uint4*>(ell)[k] = ev[s];
        }
      }
#pragma unroll
      for (int g8 = 0; g8 < kLiteMaxChunk / 8; ++g8)
        if (need_proj && g8 * 8 < chn8) reinterpret_cast<uint4*>(csr16)[g8 * 64 + lane] = cv[g8];
      if (lane <= p) mptr[lane] = mp;
      if (lane < p) { rl[lane] = rlv; vkind[lane] = (uint8_t)(lane < nF ? 1 : 0); }
      if (lane == 0) {
        rs[33 + 64 + 64] = 0.0;
        w.rc[d] = 0.0;
        w.theta[32] = 0.0;
        w.dv[32] = 0.0;
      }
      sc.sync();
      SolveView v;
      v.d = d; v.p = p; v.n_valid = n_valid; v.pm1 = true;
      v.mptr = mptr; v.mcol = nullptr; v.mval = nullptr; v.vkind = vkind;
      v.cptr = nullptr; v.cvar = nullptr; v.cvalc = nullptr; v.usign = usign;
      v.nlong = 0; v.longrow = nullptr;
      const bool empty = (n_valid == 0);
      double f = 0.0;
      // scratch of lite_model_step: the epilogue's target vector (idle while the solver runs) when it is big enough,
      // else a block of its own (small cost dimensions: the arena is sized for d = 256)
      const int nI = p - nF;
      const uint32_t need = IPM ? 0u : lite_scratch_doubles(p, nI);
      double* scr = need <= (uint32_t)d ? w.q : ar.try_get<double>(need);
      // (warm: the hit's multipliers in LDS -- lane i < 32 stores theta_i and the solver's lane i reads it back: no sync --
      //  beyond the arena, or after every cold allocation: a miss sees the arena of the cold kernel; no room = a miss)
      float* wbuf = nullptr;
      if constexpr (WARM) {
        if (wmatch && scr)
          wbuf = W.lds_extra >= 128u ? reinterpret_cast<float*>(smem + lds_bytes) : ar.try_get<float, 16u>(32u);
        if (wbuf && lane < 32) wbuf[lane] = wsel;
      }
      bool solved = false;
      if (need_proj && !empty && !scr) st = ST_TOO_LARGE;
      else if (need_proj && !empty) {
        // (IPM: the interior-point steps need none of the active-set fields; they are set all the same, unread)
        w.ls_on = !IPM;
        w.ls_nF = nF;
        w.ls_nI = nI;
        w.ls_scr = scr;
        w.warm = wbuf;
        w.bw = 0; w.band_wave = false; w.band_hot = false; w.bwin = nullptr; w.bfac = nullptr; w.bz = nullptr; w.bstg = nullptr; w.bch = 0;
        w.dn.on = false;
        w.gen.on = false;
        sc.lite.ell = ell; sc.lite.csr16 = csr16; sc.lite.rs = rs; sc.lite.rl = rl; sc.lite.chn8 = chn8; sc.lite.cmax = cmax;
#ifdef CAVE_EMUL_COUNTERS
        if (lane == 0) ++emul_counters()[6];  // test builds: instances the solve half ran the lite solver for
#endif
        SolveResult r;
        if constexpr (IPM) r = lite_solve_ipm(sc, v, w, P.max_iter);
        else r = solve_cone_impl<SC, true, false>(sc, v, w, P.max_iter, 1e-11);
        st = r.status;
        f = r.f;
        iters = r.iters;
        solved = true;
      }
      if constexpr (WARM) {
        // write-back: the final multipliers after a converged solve; a failed instance clears the entry it matched
        if (wact && solved && st == ST_OK) {
          if (lane < 32) W.theta[went * 32 + lane] = lane < p ? (float)w.theta[lane] : 0.f;
          if (lane == 0) W.key[went] = wkey;
        } else if (wact && wmatch && st != ST_OK && lane == 0) {
          W.key[went] = 0ull;
        }
        whit = wbuf != nullptr;
      }
      if (st != ST_BAD_INPUT && st != ST_TOO_LARGE) {
        EpilogueOut eo;
        eo.proj = P.o.proj ? P.o.proj + b * d : nullptr;
        eo.rnorm = P.o.rnorm ? P.o.rnorm + b : nullptr;
        eo.target = P.o.target ? P.o.target + b * d : nullptr;
        eo.loss = P.o.loss ? P.o.loss + b : nullptr;
        eo.grad = P.o.grad ? P.o.grad + b * d : nullptr;
        epilogue(sc, mode, d, P.sign, P.inner_ratio, empty, y, res, f, avg, tvec, eo);
      }
    }
  }
  if (st == ST_TOO_LARGE || st == ST_BAD_INPUT) fill_failure(sc, d, b, P.o);
  if (st != ST_OK && (P.flags & CAVE_STEP_ZERO_FAILED)) {
    // training with the status examined later (check='lazy'): the failed instance must not reach the optimizer
    if (P.o.grad) for (int k = lane; k < d; k += 64) P.o.grad[b * d + k] = 0.f;
    if (P.o.loss && lane == 0) P.o.loss[b] = 0.f;
  }
  if (lane == 0) {
    if (P.o.status) P.o.status[b] = st;
    if (P.o.iters) P.o.iters[b] = iters;
    if constexpr (WARM) {
      if (W.hit) W.hit[b] = whit ? 1 : 0;
    }
  }
}
#endif  // CAVE_GPU_CODE

}  // namespace cave
