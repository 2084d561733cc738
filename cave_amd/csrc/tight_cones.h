// tight_cones.h — the tight cone of a batch of vertices of ANY binary linear program, on the device, written directly in
// the sparse wire format (cave_hip_tight_cones_count / cave_hip_tight_cones_fill; cave_amd/tight.py tight_cones_hip).
//
// The general form of what sp_grid.h does for one constraint matrix: the reference's extraction rule
// (`_extract_tight_normals`, src/dataset.py:147-215) applied to N vertices sol [N, d] of one shared system of R rows in
// CSR form (struct cave_lin_system) plus, per instance, its own window of a second system of "lazy" rows.  Per instance
// the rows come out in the reference's order and orientation, entries in strictly increasing key = (row << 16) | col:
//     1 tight <= rows as they are   2 tight >= rows negated   3 tight == rows   4 the same == rows negated
//     5 the instance's tight lazy rows in list order, each oriented (>= negated; == the row, then its negation)
//     6 -e_k for (double)sol_k <= tol, ascending k   7 +e_k for (double)sol_k >= 1 - tol and not in 6
// A row is tight when |rhs - sum_j (double)coef_j (double)sol_j| < tol, products and sum in fp64.  A tight row without
// entries takes a row number and writes nothing.
//
// One 64-lane wave per instance, four instances per workgroup, no LDS and no barrier: `sol` is gathered from global
// memory (it is reused by every row and stays in cache), so no shape limit comes from the LDS.  Rows are taken 64 at a
// time, one per lane: a lane sums its own row when the row is short (<= kTightShort entries), the rows beyond that are
// summed four at a time, sixteen lanes each, lanes striding over the entries (coalesced) and a DPP reduction inside the
// sixteen.  The classes and the bound rows are numbered with ballots and wave scans.  One wave per instance means that the
// time of a launch is the latency of a wave's dependent loads (entry -> column -> sol), not the HBM rate: every loop
// issues the loads of several entries (kTightUnroll per lane of a long row, four of a short row, four chunks of sol)
// before it uses the first.
//
// Two passes, because the entry count differs per instance.  Both call ONE routine per 64 rows (tight_eval_chunk) and
// ONE routine for the bounds (tight_bound); the count pass tallies what they report (tight_tally), the fill pass runs
// the same tally first, compares it with the window the caller's ent_off gives the instance, and only then numbers and
// writes (tight_emit) -- so a failed instance, or a window that is not the counted size, writes nothing.
// Every index read from the inputs is checked before it is used: nothing is read or written out of range.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cave_hip.h"
#include "cone_common.h"
#include "solver_entry.h"
#include "wave_prims.h"

namespace cave {

struct TightSys {          // a cave_lin_system by value (device pointers)
  int64_t R, Z;
  const int64_t* row_off;  // [R+1]
  const int32_t* col;      // [Z]
  const float* coef;       // [Z]
  const int8_t* sense;     // [R]
  const double* rhs;       // [R]
};

struct TightConesParams {
  TightSys sys, lazy;       // lazy.R == 0: no lazy rows
  const int64_t* lazy_off;  // [N+1] or null
  const float* sol;         // [N, d]
  int64_t N;
  int32_t d;
  double tol;
  int32_t* n_rows;          // count pass: [N]
  int64_t* n_ent;           // count pass: [N]
  int32_t* status;          // [N] or null
  const int64_t* ent_off;   // fill pass: [N+1]
  int64_t ent_cap;          // fill pass: entries key / val hold
  uint32_t* key;            // fill pass
  float* val;
};

static constexpr int kTightShort = 32;      // a row of up to this many entries is summed by its own lane
static constexpr int kTightWaves = 4;       // instances per workgroup
static constexpr int64_t kTightMaxRows = 65535;

// cave_hip_tight_cones_count (fill == false) and cave_hip_tight_cones_fill: the checks, the grid and the parameter
// block.  -> CAVE_OK and *grid (0: N == 0), or CAVE_E_INVALID and the message.
inline int32_t tight_cones_plan(bool fill, const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off,
                                const float* sol, int64_t N, double tol, int32_t* n_rows, int64_t* n_ent, const int64_t* ent_off,
                                int64_t ent_cap, uint32_t* key, float* val, int32_t* status, TightConesParams* P, int64_t* grid,
                                char* msg) {
  const char* name = fill ? "tight_cones_fill" : "tight_cones_count";
  const char* what = nullptr;
  auto mis = [](const void* p, uintptr_t a) { return p == nullptr || ((uintptr_t)p & (a - 1u)) != 0u; };
  auto sys_bad = [&](const cave_lin_system* s) -> const char* {
    if (s->R < 0 || s->Z < 0) return "negative size in a system";
    if (N > 0 && s->R > 0 && (mis(s->row_off, 8) || mis(s->sense, 1) || mis(s->rhs, 8))) return "null or misaligned row_off / sense / rhs";
    if (N > 0 && s->R > 0 && s->Z > 0 && (mis(s->col, 4) || mis(s->coef, 4))) return "null or misaligned col / coef";
    return nullptr;
  };
  *grid = 0;
  const bool has_lazy = lazy != nullptr && lazy->R > 0;
  if (!sys) what = "sys is null";
  else if (sys->d < 1 || sys->d > 65535) what = "need 1 <= d <= 65535 (16-bit columns)";
  else if (N < 0) what = "bad N";
  else if (!(tol >= 0.0 && tol <= 1.7976931348623157e308)) what = "tol must be finite and >= 0";
  else if (lazy && lazy->d != sys->d) what = "the lazy rows have another d";
  else if (has_lazy && !lazy_off) what = "lazy rows need lazy_off";
  else if ((what = sys_bad(sys)) != nullptr) {}
  else if (lazy && (what = sys_bad(lazy)) != nullptr) {}
  else if (fill && ent_cap < 0) what = "negative ent_cap";
  else if (N == 0) return CAVE_OK;
  else if (mis(sol, 4)) what = "null or misaligned sol";
  else if (lazy_off && mis(lazy_off, 8)) what = "misaligned lazy_off";
  else if (status && mis(status, 4)) what = "misaligned status";
  else if (!fill && (mis(n_rows, 4) || mis(n_ent, 8))) what = "null or misaligned n_rows / n_ent";
  else if (fill && mis(ent_off, 8)) what = "null or misaligned ent_off";
  else if (fill && ent_cap > 0 && (mis(key, 4) || mis(val, 4))) what = "null or misaligned key / val";
  else if ((N + kTightWaves - 1) / kTightWaves >= (int64_t)1 << 31) what = "batch too large";
  if (what) {
    snprintf(msg, kSolverMsg, "%s: %s", name, what);
    return CAVE_E_INVALID;
  }
  auto by_value = [](const cave_lin_system* s) {
    TightSys t;
    t.R = s ? s->R : 0; t.Z = s ? s->Z : 0;
    t.row_off = s ? s->row_off : nullptr; t.col = s ? s->col : nullptr; t.coef = s ? s->coef : nullptr;
    t.sense = s ? s->sense : nullptr; t.rhs = s ? s->rhs : nullptr;
    return t;
  };
  P->sys = by_value(sys); P->lazy = by_value(lazy); P->lazy_off = lazy_off; P->sol = sol; P->N = N; P->d = sys->d; P->tol = tol;
  P->n_rows = fill ? nullptr : n_rows; P->n_ent = fill ? nullptr : n_ent; P->status = status;
  P->ent_off = fill ? ent_off : nullptr; P->ent_cap = fill ? ent_cap : 0; P->key = fill ? key : nullptr; P->val = fill ? val : nullptr;
  *grid = (N + kTightWaves - 1) / kTightWaves;
  return CAVE_OK;
}

#if defined(CAVE_GPU_CODE)
__device__ __forceinline__ bool tight_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ uint32_t tight_bcast_u32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ int64_t tight_bcast_i64(int64_t v, int l) {
  const uint32_t lo = tight_bcast_u32((uint32_t)(uint64_t)v, l), hi = tight_bcast_u32((uint32_t)((uint64_t)v >> 32), l);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// THE bound rule (rows 6 and 7): x a finite solution value
__device__ __forceinline__ void tight_bound(double x, double tol, bool& low, bool& high) {
  low = x <= tol;
  high = !low && x >= 1.0 - tol;
}

static constexpr int kTightUnroll = 8;  // entries of a long row a lane has in flight (16 lanes: 128 entries per step)

// sums over each sixteen lanes (a DPP row): lanes 12..15 of the sixteen hold theirs
__device__ __forceinline__ double tight_row16_sum(double v) {
  v += dpp_f64<0xb1, 0xf>(0.0, v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4e, 0xf>(0.0, v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x114, 0xf>(0.0, v);  // row_shr:4
  v += dpp_f64<0x118, 0xf>(0.0, v);  // row_shr:8
  return v;
}

// The next (up to) four rows of a chunk's mask, one per sixteen lanes: row[g] the lane that owns the row of group g (-1:
// none), mine = row[lane / 16].  The mask loses them.  Uniform.
struct TightFour {
  int row[4];
  int mine;
};
__device__ __forceinline__ TightFour tight_next_four(uint64_t& mask, int lane) {
  TightFour F;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    F.row[g] = mask ? __ffsll((unsigned long long)mask) - 1 : -1;
    mask &= mask - 1;  // (0 stays 0)
  }
  const int g = lane >> 4;
  F.mine = g == 0 ? F.row[0] : g == 1 ? F.row[1] : g == 2 ? F.row[2] : F.row[3];
  return F;
}

struct TightRow {  // what a lane knows about its row of the chunk
  int64_t lo;      // first entry
  int32_t len;     // entries (<= d)
  int32_t sense;
  bool tight;
  bool bad;        // the row breaks the contract of cave_lin_system
};

// THE classification routine, called by the count pass and the fill pass: 64 rows of `S`, lane l takes row `r` (its
// chunk's first row + l; `live`: the row exists), against the vertex `sol` [d].  Uniform control flow around it.
__device__ inline TightRow tight_eval_chunk(const TightSys& S, const float* sol, int32_t d, double tol, int64_t r, bool live, int lane) {
  TightRow w;
  w.lo = 0; w.len = 0; w.sense = 0; w.tight = false; w.bad = false;
  double rhs = 0.0, dot = 0.0;
  if (live) {
    const int64_t lo = S.row_off[r], hi = S.row_off[r + 1];
    const int s = (int)S.sense[r];
    rhs = S.rhs[r];
    w.bad = lo < 0 || hi < lo || hi > S.Z || hi - lo > (int64_t)d || s < 0 || s > 2 || !tight_finite(rhs);
    if (!w.bad) {
      w.lo = lo; w.len = (int32_t)(hi - lo); w.sense = s;
    }
  }
  const bool ok = live && !w.bad;
  if (ok && w.len <= kTightShort) {  // a short row: its own lane, entries in order, four in flight
    int32_t prev = -1;
    for (int32_t j0 = 0; j0 < w.len; j0 += 4) {
      int32_t c[4];
      float v[4];
      bool good[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = j0 + u < w.len;
        c[u] = in ? S.col[w.lo + j0 + u] : 0;
        v[u] = in ? S.coef[w.lo + j0 + u] : 1.0f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = j0 + u < w.len;
        good[u] = in && c[u] > prev && c[u] < d && v[u] != 0.0f && tight_finite((double)v[u]);  // (prev >= -1: c >= 0)
        if (in && !good[u]) w.bad = true;
        if (good[u]) prev = c[u];
      }
      float x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = sol[good[u] ? c[u] : 0];  // (column 0 exists: d >= 1)
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (good[u]) dot += (double)v[u] * (double)x[u];
    }
  }
  uint64_t longm = __ballot(ok && w.len > kTightShort);
  while (longm) {  // long rows: four at a time, sixteen lanes each, striding over the entries
    const TightFour F = tight_next_four(longm, lane);
    int64_t lo = 0, hi = 0;
    if (F.mine >= 0) {  // (the row's own lane found its window in range)
      lo = S.row_off[r - lane + F.mine];
      hi = S.row_off[r - lane + F.mine + 1];
    }
    double acc = 0.0;
    bool badl = false;
    for (int64_t e0 = lo + (lane & 15); e0 < hi; e0 += 16 * kTightUnroll) {
      int32_t c[kTightUnroll], pv[kTightUnroll];
      float v[kTightUnroll], x[kTightUnroll];
#pragma unroll
      for (int u = 0; u < kTightUnroll; ++u) {
        const int64_t e = e0 + 16 * u;
        const bool in = e < hi;
        c[u] = in ? S.col[e] : 0;
        v[u] = in ? S.coef[e] : 1.0f;
        pv[u] = in && e > lo ? S.col[e - 1] : -1;
      }
#pragma unroll
      for (int u = 0; u < kTightUnroll; ++u) {
        const bool in = e0 + 16 * u < hi;
        const bool good = in && c[u] > pv[u] && c[u] >= 0 && c[u] < d && v[u] != 0.0f && tight_finite((double)v[u]);
        badl = badl || (in && !good);
        x[u] = sol[good ? c[u] : 0];  // (column 0 exists: d >= 1)
        if (!good) c[u] = -1;
      }
#pragma unroll
      for (int u = 0; u < kTightUnroll; ++u)
        if (c[u] >= 0) acc += (double)v[u] * (double)x[u];
    }
    const double tot = tight_row16_sum(acc);  // lane 15 of every sixteen holds its row's sum
    const uint64_t bm = __ballot(badl);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (F.row[g] >= 0) {
        const double t = readlane_f64(tot, 16 * g + 15);
        if (lane == F.row[g]) {
          dot = t;
          w.bad = ((bm >> (16 * g)) & 0xffffull) != 0ull;
        }
      }
  }
  w.tight = live && !w.bad && fabs(rhs - dot) < tol;
  return w;
}

struct TightTally {
  int64_t cnt[3], ent[3];  // tight rows of the shared system by sense, and their entries
  int64_t lz_lo, lz_hi;    // the instance's window of lazy rows
  int64_t lz_rows, lz_ent; // oriented tight lazy rows (an == row counts twice) and their entries
  int64_t n_low, n_high;
  int32_t status;
  __device__ int64_t rows() const { return cnt[0] + cnt[1] + 2 * cnt[2] + lz_rows + n_low + n_high; }
  __device__ int64_t entries() const { return ent[0] + ent[1] + 2 * ent[2] + lz_ent + n_low + n_high; }
};

// what the count pass reports for instance b, and what the fill pass checks its window against; uniform over the wave
__device__ inline TightTally tight_tally(const TightConesParams& P, int64_t b, int lane) {
  TightTally T;
  for (int c = 0; c < 3; ++c) T.cnt[c] = T.ent[c] = 0;
  T.lz_lo = T.lz_hi = T.lz_rows = T.lz_ent = T.n_low = T.n_high = 0;
  T.status = CAVE_ST_OK;
  const int32_t d = P.d;
  const float* sol = P.sol + (size_t)b * (size_t)d;
  bool badl = false;
  for (int32_t k0 = 0; k0 < d; k0 += 64 * 4) {  // four chunks of sol in flight
    double x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = k0 + 64 * u + lane < d ? (double)sol[k0 + 64 * u + lane] : 0.5;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool fin = tight_finite(x[u]);
      bool low = false, high = false;
      if (k0 + 64 * u + lane < d && fin) tight_bound(x[u], P.tol, low, high);
      badl = badl || !fin;
      T.n_low += __popcll(__ballot(low));
      T.n_high += __popcll(__ballot(high));
    }
  }
  bool bad = __ballot(badl) != 0ull;
  for (int64_t r0 = 0; r0 < P.sys.R && !bad; r0 += 64) {
    const TightRow w = tight_eval_chunk(P.sys, sol, d, P.tol, r0 + lane, r0 + lane < P.sys.R, lane);
    bad = __ballot(w.bad) != 0ull;
    for (int c = 0; c < 3; ++c) {
      const bool in = w.tight && w.sense == c;
      T.cnt[c] += __popcll(__ballot(in));
      T.ent[c] += wave_sum_u32(in ? (uint32_t)w.len : 0u);
    }
  }
  if (!bad && P.lazy_off) {
    T.lz_lo = P.lazy_off[b];
    T.lz_hi = P.lazy_off[b + 1];
    bad = T.lz_lo < 0 || T.lz_hi < T.lz_lo || T.lz_hi > P.lazy.R;
    for (int64_t r0 = T.lz_lo; r0 < T.lz_hi && !bad; r0 += 64) {
      const TightRow w = tight_eval_chunk(P.lazy, sol, d, P.tol, r0 + lane, r0 + lane < T.lz_hi, lane);
      bad = __ballot(w.bad) != 0ull;
      const uint32_t nr = w.tight ? (w.sense == 2 ? 2u : 1u) : 0u;
      T.lz_rows += wave_sum_u32(nr);
      T.lz_ent += wave_sum_u32(nr * (uint32_t)w.len);
    }
  }
  if (bad) T.status = CAVE_ST_BAD_INPUT;
  else if (T.rows() > kTightMaxRows) T.status = CAVE_ST_TOO_LARGE;
  return T;
}

// Write the rows of a chunk: a lane with `emit` writes its row as row number rnA at entry ebA with sign sgn and -- `twice`
// -- again, negated, as rnB at ebB.  key / val: the instance's window of `cap` entries.
__device__ inline void tight_emit_chunk(const TightSys& S, uint32_t* key, float* val, int64_t cap, const TightRow& w, bool emit, uint32_t rnA,
                                        int64_t ebA, bool neg, bool twice, uint32_t rnB, int64_t ebB, int lane) {
  if (emit && w.len <= kTightShort) {
    for (int32_t j0 = 0; j0 < w.len; j0 += 4) {
      uint32_t c[4];
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = j0 + u < w.len;
        c[u] = in ? (uint32_t)S.col[w.lo + j0 + u] : 0u;
        v[u] = in ? S.coef[w.lo + j0 + u] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int32_t j = j0 + u;
        if (j < w.len && ebA + j < cap) {
          key[ebA + j] = (rnA << 16) | c[u];
          val[ebA + j] = neg ? -v[u] : v[u];
        }
        if (j < w.len && twice && ebB + j < cap) {
          key[ebB + j] = (rnB << 16) | c[u];
          val[ebB + j] = neg ? v[u] : -v[u];
        }
      }
    }
  }
  uint64_t longm = __ballot(emit && w.len > kTightShort);
  while (longm) {  // long rows: four at a time, sixteen lanes each
    const TightFour F = tight_next_four(longm, lane);
    int64_t lo = 0, a = 0, b2 = 0;
    int32_t len = 0;
    uint32_t ra = 0u, rb = 0u, fl = 0u;
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (F.row[g] >= 0) {  // the row's figures, from the lane that owns it to its sixteen
        const int64_t tlo = tight_bcast_i64(w.lo, F.row[g]), ta = tight_bcast_i64(ebA, F.row[g]), tb = tight_bcast_i64(ebB, F.row[g]);
        const uint32_t tlen = tight_bcast_u32((uint32_t)w.len, F.row[g]);
        const uint32_t tra = tight_bcast_u32(rnA, F.row[g]), trb = tight_bcast_u32(rnB, F.row[g]);
        const uint32_t tfl = tight_bcast_u32((neg ? 1u : 0u) | (twice ? 2u : 0u), F.row[g]);
        if ((lane >> 4) == g) {
          lo = tlo; a = ta; b2 = tb; len = (int32_t)tlen; ra = tra; rb = trb; fl = tfl;
        }
      }
    for (int32_t e0 = lane & 15; e0 < len; e0 += 16 * kTightUnroll) {
      uint32_t c[kTightUnroll];
      float v[kTightUnroll];
#pragma unroll
      for (int u = 0; u < kTightUnroll; ++u) {
        const int32_t e = e0 + 16 * u;
        c[u] = e < len ? (uint32_t)S.col[lo + e] : 0u;
        v[u] = e < len ? S.coef[lo + e] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < kTightUnroll; ++u) {
        const int32_t e = e0 + 16 * u;
        if (e < len && a + e < cap) {
          key[a + e] = (ra << 16) | c[u];
          val[a + e] = (fl & 1u) ? -v[u] : v[u];
        }
        if (e < len && (fl & 2u) && b2 + e < cap) {
          key[b2 + e] = (rb << 16) | c[u];
          val[b2 + e] = (fl & 1u) ? v[u] : -v[u];
        }
      }
    }
  }
}

// the fill pass of an instance whose tally is T and whose window is T.entries() entries at key / val
__device__ inline void tight_emit(const TightConesParams& P, const TightTally& T, int64_t b, uint32_t* key, float* val, int lane) {
  const int32_t d = P.d;
  const float* sol = P.sol + (size_t)b * (size_t)d;
  const int64_t cap = T.entries();
  // classes 1..4: first row number and first entry of each, then running counts per sense
  const int64_t row0[4] = {0, T.cnt[0], T.cnt[0] + T.cnt[1], T.cnt[0] + T.cnt[1] + T.cnt[2]};
  const int64_t ent0[4] = {0, T.ent[0], T.ent[0] + T.ent[1], T.ent[0] + T.ent[1] + T.ent[2]};
  int64_t rrun[3] = {0, 0, 0}, erun[3] = {0, 0, 0};
  for (int64_t r0 = 0; r0 < P.sys.R; r0 += 64) {
    const TightRow w = tight_eval_chunk(P.sys, sol, d, P.tol, r0 + lane, r0 + lane < P.sys.R, lane);
    uint32_t rn = 0u;
    int64_t eb = 0;
    for (int c = 0; c < 3; ++c) {
      const bool in = w.tight && w.sense == c;
      const uint64_t m = __ballot(in);
      const uint32_t inc = wave_inclusive_scan_u32(in ? (uint32_t)w.len : 0u);
      if (in) {
        rn = (uint32_t)(row0[c] + rrun[c]) + mbcnt64(m);
        eb = ent0[c] + erun[c] + (int64_t)(inc - (uint32_t)w.len);
      }
      rrun[c] += __popcll(m);
      erun[c] += (int64_t)tight_bcast_u32(inc, 63);
    }
    const bool eq = w.sense == 2;
    tight_emit_chunk(P.sys, key, val, cap, w, w.tight, rn, eb, w.sense == 1, eq, rn + (uint32_t)T.cnt[2], eb + T.ent[2], lane);
  }
  int64_t rbase = row0[3] + T.cnt[2], ebase = ent0[3] + T.ent[2];
  for (int64_t r0 = T.lz_lo; r0 < T.lz_hi; r0 += 64) {
    const TightRow w = tight_eval_chunk(P.lazy, sol, d, P.tol, r0 + lane, r0 + lane < T.lz_hi, lane);
    const uint32_t nr = w.tight ? (w.sense == 2 ? 2u : 1u) : 0u;
    const uint32_t rinc = wave_inclusive_scan_u32(nr), einc = wave_inclusive_scan_u32(nr * (uint32_t)w.len);
    const uint32_t rn = (uint32_t)rbase + rinc - nr;
    const int64_t eb = ebase + (int64_t)(einc - nr * (uint32_t)w.len);
    tight_emit_chunk(P.lazy, key, val, cap, w, w.tight, rn, eb, w.sense == 1, w.sense == 2, rn + 1u, eb + w.len, lane);
    rbase += (int64_t)tight_bcast_u32(rinc, 63);
    ebase += (int64_t)tight_bcast_u32(einc, 63);
  }
  // rows 6 and 7: a ballot prefix over the bound flags
  int64_t lows = 0, highs = 0;
  for (int32_t k0 = 0; k0 < d; k0 += 64 * 4) {  // four chunks of sol in flight
    double x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = k0 + 64 * u + lane < d ? (double)sol[k0 + 64 * u + lane] : 0.5;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int32_t k = k0 + 64 * u + lane;
      bool low = false, high = false;
      if (k < d) tight_bound(x[u], P.tol, low, high);
      const uint64_t ml = __ballot(low), mh = __ballot(high);
      if (low || high) {
        const int64_t r = low ? lows + (int64_t)mbcnt64(ml) : T.n_low + highs + (int64_t)mbcnt64(mh);
        if (ebase + r < cap) {
          key[ebase + r] = ((uint32_t)(rbase + r) << 16) | (uint32_t)k;
          val[ebase + r] = low ? -1.0f : 1.0f;
        }
      }
      lows += __popcll(ml);
      highs += __popcll(mh);
    }
  }
}

// the two kernel bodies: one instance on one wave
__device__ inline void tight_cones_count_instance(const TightConesParams& P, int64_t b, int lane) {
  const TightTally T = tight_tally(P, b, lane);
  if (lane == 0) {
    const bool ok = T.status == CAVE_ST_OK;
    P.n_rows[b] = ok ? (int32_t)T.rows() : 0;
    P.n_ent[b] = ok ? T.entries() : 0;
    if (P.status) P.status[b] = T.status;
  }
}
__device__ inline void tight_cones_fill_instance(const TightConesParams& P, int64_t b, int lane) {
  const TightTally T = tight_tally(P, b, lane);
  int32_t st = T.status;
  if (st == CAVE_ST_OK) {
    const int64_t lo = P.ent_off[b], hi = P.ent_off[b + 1];
    if (lo < 0 || hi < lo || hi > P.ent_cap || hi - lo != T.entries()) st = CAVE_ST_BAD_INPUT;  // not the counted window
    else if (hi > lo) tight_emit(P, T, b, P.key + lo, P.val + lo, lane);
  }
  if (lane == 0 && P.status) P.status[b] = st;
}
#endif  // CAVE_GPU_CODE

#if defined(__HIPCC__) && !defined(CAVE_SIMT_EMUL)
// k_tight_cones.hip: grid workgroups of kTightWaves waves, no LDS
hipError_t launch_tight_cones(bool fill, unsigned grid, hipStream_t stream, const TightConesParams& P);
#endif

}  // namespace cave
