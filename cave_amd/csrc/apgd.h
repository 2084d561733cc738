// apgd.h — the reference's accelerated projected-gradient projector (`project_apgd`, src/qpsolver.py:11-110) on the
// device: cave_hip_cone_apgd (dense wire format) and cave_hip_cone_apgd_sparse (struct cave_sparse_cones).
//
// APGD iterates in the multiplier space of the ORIGINAL rows: duplicate +a/-a pairs, unit rows and zero padding stay as
// they are (a clamp on x+ and on x- under momentum is not the iteration of one free multiplier, and the power iteration
// for the step size sees the duplicates), so this kernel reads the two wire formats themselves, not the reduced cone of
// the stores.  Per instance, A is m_max x d as given (zero rows included), y = sign * pred, everything in fp64:
//   step size   v = 1/sqrt(m_max) in every row;  power_iter times  u = A^T v, v = A u, v /= max(||v||, 1e-8);
//               s = 1 / max(||A^T v||^2, 1e-8)
//   iterations  x_curr = x_prev = 0;  for k = k_start .. k_start + n_iter - 1, beta_k = (k-2)/(k+1), beta_0 = 0:
//               y_k = x_curr + beta_k (x_curr - x_prev);  g = A (A^T y_k - y);  x_prev = x_curr;  x_curr = max(y_k - s g, 0)
//   results     proj = A^T x_curr, rnorm = ||y - proj||, the CAVE_MODE_EXACT epilogue on proj, and the check quantity
//               max_i (x_i > 0 ? |g_i| : max(-g_i, 0)) with g = A (A^T x_curr - y)
//
// One workgroup per instance, of one wave (small instances) or four (apgd_waves: the host plan's choice from m_max, d
// and the entry capacity).  Two loaders feed one core: the dense loader scans the zero-padded block and compacts its
// non-zeros into LDS in (row, col) order (every wave counts its share of the block, then writes it behind the counts of
// the waves before it); the sparse loader copies the instance's entries after checking every one.  The core builds row
// pointers over the row-major entries and a stable counting sort by column beside them.  Thread t owns rows and columns
// t, t + NT, ...; every row sum and every column sum is accumulated by its owner alone, rows in ascending column order,
// columns in ascending row order, and every norm is summed in index order by every thread for itself: no atomics, no
// reduction tree, every multiply-add an explicit fma.  So a launch is bit-reproducible, an instance's result does not
// depend on its position in the batch, on its neighbours or on the workgroup size, and a chain of launches through the
// continuation state equals the single launch bit for bit.  No loop bound depends on the data beyond the entry counts.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cave_hip.h"
#include "cone_common.h"
#include "solver_entry.h"
#include "wave_prims.h"

namespace cave {

static constexpr int64_t kApgdMaxLds = 160 * 1024;
static constexpr int32_t kApgdMaxIter = 100000, kApgdMaxPower = 64;
static constexpr int64_t kApgdMaxK = (int64_t)1 << 30;  // k_start + n_iter stays an int32

// LDS offsets of the per-workgroup arrays (each rounded up to 16 bytes):
//   xc, xp, yk [m] f64 | res, yv [d] f64 | key [cap] u32 (row << 16 | col, row-major) | val [cap] f32 |
//   cval [cap] f32, crow [cap] u16 (the same entries sorted by column, rows ascending) | rowptr [m+1] u32 |
//   cptr [d+1] u32 | misc [16] u32 (0..3 the waves' entry counts, 8 bad-input flag)
struct ApgdLds {
  uint32_t xc, xp, yk, res, yv, key, val, cval, crow, rowptr, cptr, misc;
  int64_t bytes;
};
CAVE_HOSTDEV ApgdLds apgd_lds_layout(int64_t m, int64_t d, int64_t cap) {
  ApgdLds L;
  int64_t p = 0;
  auto take = [&p](int64_t n) { const int64_t at = p; p += (n + 15) & ~(int64_t)15; return (uint32_t)at; };
  L.xc = take(8 * m); L.xp = take(8 * m); L.yk = take(8 * m);
  L.res = take(8 * d); L.yv = take(8 * d);
  L.key = take(4 * cap); L.val = take(4 * cap); L.cval = take(4 * cap); L.crow = take(2 * cap);
  L.rowptr = take(4 * (m + 1)); L.cptr = take(4 * (d + 1));
  L.misc = take(64);
  L.bytes = p;
  return L;
}
CAVE_HOSTDEV bool apgd_shape_ok(int64_t m, int64_t d) { return m >= 1 && m <= 65535 && d >= 1 && d <= 65535; }
// the arena of one workgroup, or -1: the shape or the capacity is out of range, or the arena exceeds 160 KiB
CAVE_HOSTDEV int64_t apgd_lds_bytes(int64_t m, int64_t d, int64_t cap) {
  if (!apgd_shape_ok(m, d) || cap < 1 || cap > m * d) return -1;
  const int64_t b = apgd_lds_layout(m, d, cap).bytes;
  return b <= kApgdMaxLds ? b : -1;
}
// waves per instance: one while every array is short, else four
CAVE_HOSTDEV int apgd_waves(int64_t m, int64_t d, int64_t cap) { return (cap > 512 || m > 512 || d > 512) ? 4 : 1; }

struct ApgdParams {
  const float* ctrs;        // dense loader: [B, m, d]
  const int64_t* ent_off;   // sparse loader: [B+1]
  const uint32_t* key;
  const float* val;
  const float* pred;        // [B, d]
  int64_t B;
  int32_t m, d, mode;
  double sign;
  int32_t k_start, n_iter, power_iter;
  uint32_t cap;
  double* x_curr;           // [B, m] or null
  double* x_prev;           // [B, m] or null
  double* step;             // [B] or null
  float* proj;              // [B, d] or null
  float* rnorm;             // [B] or null
  float* target;            // [B, d] or null   (CAVE_MODE_EXACT)
  float* loss;              // [B] or null      (CAVE_MODE_EXACT)
  float* grad;              // [B, d] or null   (CAVE_MODE_EXACT)
  int32_t* status;          // [B] or null
  int32_t* iters;           // [B] or null
  double* pgrad;            // [B] or null
  ApgdLds L;
};

// cave_hip_cone_apgd (cones == null: `ctrs`, m_max, d) and cave_hip_cone_apgd_sparse (`cones`): the checks, the grid, the
// workgroup size and the parameter block.  -> CAVE_OK, *grid (0: B == 0) and *waves, or CAVE_E_INVALID and the message.
inline int32_t apgd_plan(bool sparse, const float* ctrs, const cave_sparse_cones* cones, const float* pred, int64_t B, int64_t m_max,
                         int64_t d, int32_t mode, float sign, int32_t k_start, int32_t n_iter, int32_t power_iter, int32_t nnz_cap,
                         double* x_curr, double* x_prev, double* step, float* proj, float* rnorm, float* target, float* loss,
                         float* grad, int32_t* status, int32_t* iters, double* pgrad, ApgdParams* P, int64_t* grid, int* waves,
                         char* msg) {
  const char* name = sparse ? "cone_apgd_sparse" : "cone_apgd";
  const char* what = nullptr;
  auto mis = [](const void* p, uintptr_t a) { return p == nullptr || ((uintptr_t)p & (a - 1u)) != 0u; };
  *grid = 0;
  *waves = 1;
  if (sparse && !cones) what = "cones is null";
  else {
    if (sparse) { B = cones->B; m_max = cones->m_max; d = cones->d; }
    const int n_state = (x_curr != nullptr) + (x_prev != nullptr) + (step != nullptr);
    if (B < 0) what = "bad B";
    else if (B == 0) return CAVE_OK;
    else if (!apgd_shape_ok(m_max, d)) what = "bad shape (need 1 <= m_max <= 65535, 1 <= d <= 65535)";
    else if (mode != CAVE_MODE_PROJECT && mode != CAVE_MODE_EXACT) what = "bad mode";
    else if (!(sign == 1.0f || sign == -1.0f)) what = "sign must be +1 or -1";
    else if (k_start < 0 || (int64_t)k_start > kApgdMaxK) what = "bad k_start (0 .. 2^30)";
    else if (n_iter < 0 || n_iter > kApgdMaxIter) what = "bad n_iter (0 .. 100000)";
    else if (power_iter < 0 || power_iter > kApgdMaxPower) what = "bad power_iter (0 .. 64)";
    else if (nnz_cap < 1 || (int64_t)nnz_cap > m_max * d) what = "bad nnz_cap (1 .. m_max * d)";
    else if (apgd_lds_bytes(m_max, d, nnz_cap) < 0) what = "the arena of this m_max, d and nnz_cap exceeds 160 KiB of LDS (cave_hip_apgd_lds_bytes)";
    else if (mis(pred, 4)) what = "null or misaligned pred";
    else if (!sparse && mis(ctrs, 4)) what = "null or misaligned ctrs";
    else if (sparse && (mis(cones->ent_off, 8) || mis(cones->key, 4) || mis(cones->val, 4))) what = "null or misaligned ent_off / key / val";
    else if (n_state != 0 && n_state != 3) what = "x_curr, x_prev and step go together";
    else if (k_start > 0 && n_state == 0) what = "a continuation (k_start > 0) needs x_curr, x_prev and step";
    else if (n_state == 3 && (mis(x_curr, 8) || mis(x_prev, 8) || mis(step, 8))) what = "misaligned x_curr / x_prev / step";
    else if (pgrad && mis(pgrad, 8)) what = "misaligned pgrad";
    else if (B >= (int64_t)1 << 31) what = "batch too large (B < 2^31)";
  }
  if (what) {
    snprintf(msg, kSolverMsg, "%s: %s", name, what);
    return CAVE_E_INVALID;
  }
  P->ctrs = sparse ? nullptr : ctrs;
  P->ent_off = sparse ? cones->ent_off : nullptr; P->key = sparse ? cones->key : nullptr; P->val = sparse ? cones->val : nullptr;
  P->pred = pred; P->B = B; P->m = (int32_t)m_max; P->d = (int32_t)d; P->mode = mode; P->sign = (double)sign;
  P->k_start = k_start; P->n_iter = n_iter; P->power_iter = power_iter; P->cap = (uint32_t)nnz_cap;
  P->x_curr = x_curr; P->x_prev = x_prev; P->step = step;
  P->proj = proj; P->rnorm = rnorm; P->target = target; P->loss = loss; P->grad = grad; P->status = status; P->iters = iters;
  P->pgrad = pgrad;
  P->L = apgd_lds_layout(m_max, d, nnz_cap);
  *grid = B;
  *waves = apgd_waves(m_max, d, nnz_cap);
  return CAVE_OK;
}

#if defined(CAVE_GPU_CODE)
__device__ __forceinline__ bool apgd_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

struct ApgdView {  // the arena of one workgroup
  double *xc, *xp, *yk, *res, *yv;
  uint32_t* key;
  float *val, *cval;
  uint16_t* crow;
  uint32_t *rowptr, *cptr, *misc;
};

// a failed instance: NaN in every float output given, nothing else
template <int NT>
__device__ inline void apgd_fail(const ApgdParams& P, int64_t b, int32_t st, int tid) {
  const float qnan = __builtin_nanf("");
  const size_t o = (size_t)b * (size_t)P.d;
  for (int c = tid; c < P.d; c += NT) {
    if (P.proj) P.proj[o + c] = qnan;
    if (P.target) P.target[o + c] = qnan;
    if (P.grad) P.grad[o + c] = qnan;
  }
  if (tid == 0) {
    if (P.rnorm) P.rnorm[b] = qnan;
    if (P.loss) P.loss[b] = qnan;
    if (P.pgrad) P.pgrad[b] = __builtin_nan("");
    if (P.status) P.status[b] = st;
    if (P.iters) P.iters[b] = 0;
  }
}

// res[c] = sum over the entries of column c, rows ascending, of a_ic v_i  (- sub[c] when sub is given)
template <int NT>
__device__ __forceinline__ void apgd_cols(const ApgdView& V, int d, const double* v, const double* sub, int tid) {
  for (int c = tid; c < d; c += NT) {
    double acc = 0.0;
    const uint32_t hi = V.cptr[c + 1];
    for (uint32_t e = V.cptr[c]; e < hi; ++e) acc = fma((double)V.cval[e], v[V.crow[e]], acc);
    V.res[c] = sub ? acc - sub[c] : acc;
  }
}
// the sum over the entries of row i, columns ascending, of a_ic (u_c - sub_c)
__device__ __forceinline__ double apgd_row(const ApgdView& V, int i, const double* u, const double* sub) {
  double acc = 0.0;
  const uint32_t hi = V.rowptr[i + 1];
  for (uint32_t e = V.rowptr[i]; e < hi; ++e) {
    const uint32_t c = V.key[e] & 0xffffu;
    acc = fma((double)V.val[e], sub ? u[c] - sub[c] : u[c], acc);
  }
  return acc;
}
// sum of squares in index order, by the calling thread for itself
__device__ __forceinline__ double apgd_sumsq(const double* a, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s = fma(a[i], a[i], s);
  return s;
}

// the dense loader: -> the entry count (beyond P.cap: nothing stored); bad input raises misc[8]
template <int NW>
__device__ inline uint32_t apgd_load_dense(const ApgdParams& P, const ApgdView& V, int64_t b, int tid) {
  constexpr int U = 4;
  const int lane = tid & 63, wave = tid >> 6;
  const uint32_t d = (uint32_t)P.d, n = (uint32_t)P.m * d;  // (m, d <= 65535: n + 64 U < 2^32)
  const float* A = P.ctrs + (size_t)b * (size_t)n;
  const uint32_t chunks = (n + 63u) / 64u, per = (chunks + (uint32_t)NW - 1u) / (uint32_t)NW;
  const uint64_t span = (uint64_t)per * 64u, first = (uint64_t)wave * span;
  const uint32_t lo = first < n ? (uint32_t)first : n;
  const uint32_t hi = first + span < n ? (uint32_t)(first + span) : n;
  uint32_t cnt = 0u;
  bool bad = false;
  for (uint32_t base = lo; base < hi; base += 64u * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = base + 64u * u + (uint32_t)lane;
      v[u] = i < hi ? A[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bad = bad || !apgd_finite((double)v[u]);
      cnt += (uint32_t)__popcll(__ballot(v[u] != 0.0f));
    }
  }
  if (lane == 0) V.misc[wave] = cnt;
  if (bad) V.misc[8] = 1u;
  __syncthreads();
  uint32_t off = 0u, total = 0u;
  for (int w = 0; w < NW; ++w) {
    const uint32_t c = V.misc[w];
    if (w < wave) off += c;
    total += c;
  }
  if (V.misc[8] != 0u || total > P.cap) return total;
  uint32_t cursor = off;
  for (uint32_t base = lo; base < hi; base += 64u * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = base + 64u * u + (uint32_t)lane;
      v[u] = i < hi ? A[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t i = base + 64u * u + (uint32_t)lane;
      const bool nz = v[u] != 0.0f;
      const uint64_t mk = __ballot(nz);
      const uint32_t pos = cursor + mbcnt64(mk);
      if (nz && pos < P.cap) {  // (pos < total <= cap while the block does not change under the launch)
        V.key[pos] = ((i / d) << 16) | (i % d);
        V.val[pos] = v[u];
      }
      cursor += (uint32_t)__popcll(mk);
    }
  }
  return total;
}

// the sparse loader: every key is checked before it is used
template <int NT>
__device__ inline uint32_t apgd_load_sparse(const ApgdParams& P, const ApgdView& V, int64_t b, int tid) {
  const int64_t lo = P.ent_off[b], hi = P.ent_off[b + 1];
  if (lo < 0 || hi < lo) {
    V.misc[8] = 1u;  // (every thread, the same value)
    return 0u;
  }
  if (hi - lo > (int64_t)P.cap) return P.cap + 1u;
  const uint32_t n = (uint32_t)(hi - lo);
  bool bad = false;
  for (uint32_t e = (uint32_t)tid; e < n; e += (uint32_t)NT) {
    const uint32_t k = P.key[lo + e];
    const float v = P.val[lo + e];
    const bool good = (k >> 16) < (uint32_t)P.m && (k & 0xffffu) < (uint32_t)P.d && (e == 0u || k > P.key[lo + e - 1]) &&
                      v != 0.0f && apgd_finite((double)v);
    bad = bad || !good;
    V.key[e] = good ? k : 0u;
    V.val[e] = good ? v : 0.0f;
  }
  if (bad) V.misc[8] = 1u;
  return n;
}

// one instance on one workgroup of NW waves; smem: the arena of apgd_lds_layout
template <int NW, bool SPARSE>
__device__ inline void apgd_block(const ApgdParams& P, unsigned char* smem) {
  constexpr int NT = 64 * NW;
  const int tid = (int)threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x;
  if (b >= P.B) return;
  const int m = P.m, d = P.d;
  ApgdView V;
  V.xc = (double*)(smem + P.L.xc); V.xp = (double*)(smem + P.L.xp); V.yk = (double*)(smem + P.L.yk);
  V.res = (double*)(smem + P.L.res); V.yv = (double*)(smem + P.L.yv);
  V.key = (uint32_t*)(smem + P.L.key); V.val = (float*)(smem + P.L.val); V.cval = (float*)(smem + P.L.cval);
  V.crow = (uint16_t*)(smem + P.L.crow); V.rowptr = (uint32_t*)(smem + P.L.rowptr); V.cptr = (uint32_t*)(smem + P.L.cptr);
  V.misc = (uint32_t*)(smem + P.L.misc);

  if (tid < 16) V.misc[tid] = 0u;
  __syncthreads();
  // ---- load: y = sign * pred, then the entries in (row, col) order
  {
    bool bad = false;
    for (int c = tid; c < d; c += NT) {
      const double y = P.sign * (double)P.pred[(size_t)b * (size_t)d + c];
      bad = bad || !apgd_finite(y);
      V.yv[c] = y;
    }
    if (bad) V.misc[8] = 1u;
  }
  uint32_t nnz;
  if (SPARSE) nnz = apgd_load_sparse<NT>(P, V, b, tid);
  else nnz = apgd_load_dense<NW>(P, V, b, tid);
  __syncthreads();
  if (V.misc[8] != 0u || nnz > P.cap) {  // (the same for every thread: read behind the barrier)
    apgd_fail<NT>(P, b, V.misc[8] != 0u ? CAVE_ST_BAD_INPUT : CAVE_ST_TOO_LARGE, tid);
    return;
  }
  // ---- build: row pointers (entry e opens the rows after its predecessor's up to its own), then the column side
  for (uint32_t e = (uint32_t)tid; e <= nnz; e += (uint32_t)NT) {
    const uint32_t r0 = e == 0u ? 0u : (V.key[e - 1] >> 16) + 1u;
    const uint32_t r1 = e == nnz ? (uint32_t)m : (V.key[e] >> 16);
    for (uint32_t r = r0; r <= r1; ++r) V.rowptr[r] = e;
  }
  for (int c = tid; c < d; c += NT) {  // entries of column c (its owner walks the list: no atomics)
    uint32_t cnt = 0u;
    for (uint32_t e = 0u; e < nnz; ++e) cnt += (V.key[e] & 0xffffu) == (uint32_t)c ? 1u : 0u;
    V.cptr[c + 1] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t acc = 0u;
    V.cptr[0] = 0u;
    for (int c = 1; c <= d; ++c) {
      acc += V.cptr[c];
      V.cptr[c] = acc;
    }
  }
  __syncthreads();
  for (int c = tid; c < d; c += NT) {  // stable: the entries of a column in list order, which is ascending rows
    uint32_t at = V.cptr[c];
    const uint32_t end = V.cptr[c + 1];
    for (uint32_t e = 0u; e < nnz && at < end; ++e)
      if ((V.key[e] & 0xffffu) == (uint32_t)c) {
        V.crow[at] = (uint16_t)(V.key[e] >> 16);
        V.cval[at] = V.val[e];
        ++at;
      }
  }
  __syncthreads();

  // ---- step size and start, or the state of the launch before
  double s;
  if (P.k_start == 0) {
    const double v0 = 1.0 / sqrt((double)m);
    for (int i = tid; i < m; i += NT) V.yk[i] = v0;
    __syncthreads();
    for (int it = 0; it < P.power_iter; ++it) {
      apgd_cols<NT>(V, d, V.yk, nullptr, tid);                                     // u = A^T v
      __syncthreads();
      for (int i = tid; i < m; i += NT) V.xc[i] = apgd_row(V, i, V.res, nullptr);  // v = A u
      __syncthreads();
      const double nrm = fmax(sqrt(apgd_sumsq(V.xc, m)), 1e-8);
      for (int i = tid; i < m; i += NT) V.yk[i] = V.xc[i] / nrm;
      __syncthreads();
    }
    apgd_cols<NT>(V, d, V.yk, nullptr, tid);
    __syncthreads();
    s = 1.0 / fmax(apgd_sumsq(V.res, d), 1e-8);
    for (int i = tid; i < m; i += NT) V.xc[i] = V.xp[i] = 0.0;
  } else {
    s = P.step[b];
    for (int i = tid; i < m; i += NT) {
      V.xc[i] = P.x_curr[(size_t)b * (size_t)m + i];
      V.xp[i] = P.x_prev[(size_t)b * (size_t)m + i];
    }
  }
  // (xc / xp of a row are touched by its owner alone until the results)

  // ---- iterations: two barriers each
  for (int it = 0; it < P.n_iter; ++it) {
    const int k = P.k_start + it;
    const double beta = k == 0 ? 0.0 : (double)(k - 2) / (double)(k + 1);
    for (int i = tid; i < m; i += NT) V.yk[i] = fma(beta, V.xc[i] - V.xp[i], V.xc[i]);
    __syncthreads();
    apgd_cols<NT>(V, d, V.yk, V.yv, tid);  // res = A^T y_k - y
    __syncthreads();
    for (int i = tid; i < m; i += NT) {
      const double g = apgd_row(V, i, V.res, nullptr);
      V.xp[i] = V.xc[i];
      V.xc[i] = fmax(fma(-s, g, V.yk[i]), 0.0);
    }
  }

  // ---- results
  if (P.x_curr) {
    for (int i = tid; i < m; i += NT) {
      P.x_curr[(size_t)b * (size_t)m + i] = V.xc[i];
      P.x_prev[(size_t)b * (size_t)m + i] = V.xp[i];
    }
    if (tid == 0) P.step[b] = s;
  }
  __syncthreads();
  apgd_cols<NT>(V, d, V.xc, nullptr, tid);  // res = proj = A^T x_curr
  __syncthreads();
  if (P.pgrad) {
    for (int i = tid; i < m; i += NT) {
      const double g = apgd_row(V, i, V.res, V.yv);
      V.yk[i] = V.xc[i] > 0.0 ? fabs(g) : fmax(-g, 0.0);
    }
    __syncthreads();
    if (tid == 0) {
      double mx = 0.0;
      for (int i = 0; i < m; ++i) mx = fmax(mx, V.yk[i]);
      P.pgrad[b] = mx;
    }
  }
  const size_t o = (size_t)b * (size_t)d;
  double ss = 0.0, pp = 0.0, rr = 0.0;
  for (int c = 0; c < d; ++c) {
    const double y = V.yv[c], p = V.res[c], r = y - p;
    ss = fma(y, y, ss);
    pp = fma(p, p, pp);
    rr = fma(r, r, rr);
  }
  if (tid == 0) {
    if (P.rnorm) P.rnorm[b] = (float)sqrt(rr);
    if (P.status) P.status[b] = CAVE_ST_OK;
    if (P.iters) P.iters[b] = P.n_iter;
  }
  if (P.mode == CAVE_MODE_PROJECT) {
    if (P.proj) for (int c = tid; c < d; c += NT) P.proj[o + c] = (float)V.res[c];
    return;
  }
  // the epilogue of CAVE_MODE_EXACT (cone_core.h epilogue): target = proj / max(||proj||, 1e-8) as a float32 vector,
  // loss = 1 - cos(y, target), grad = d loss / d pred
  __syncthreads();  // (every thread has read res)
  const double ns = sqrt(ss), ns_c = fmax(ns, kNormClamp), np_c = fmax(sqrt(pp), kNormClamp);
  for (int c = tid; c < d; c += NT) {
    const double p = V.res[c];
    if (P.proj) P.proj[o + c] = (float)p;
    V.res[c] = (double)(float)(p / np_c);  // (from the fp64 projection: one rounding)
  }
  __syncthreads();
  double tt = 0.0, st = 0.0;
  for (int c = 0; c < d; ++c) {
    const double t = V.res[c];
    tt = fma(t, t, tt);
    st = fma(V.yv[c], t, st);
  }
  const double nt_c = fmax(sqrt(tt), kNormClamp);
  const double inv = 1.0 / (ns_c * nt_c);
  const double radial = ns > kNormClamp ? st / (ns_c * ns_c * ns * nt_c) : 0.0;
  if (tid == 0 && P.loss) P.loss[b] = (float)(1.0 - st / (ns_c * nt_c));
  for (int c = tid; c < d; c += NT) {
    if (P.target) P.target[o + c] = (float)V.res[c];
    if (P.grad) P.grad[o + c] = (float)(-P.sign * (V.res[c] * inv - radial * V.yv[c]));
  }
}
#endif  // CAVE_GPU_CODE

#if defined(__HIPCC__) && !defined(CAVE_SIMT_EMUL)
// k_apgd_w1.hip / k_apgd_w4.hip: B workgroups of `waves` waves, the arena of P.L as dynamic LDS
hipError_t launch_apgd_w1(bool sparse, unsigned grid, hipStream_t stream, const ApgdParams& P);
hipError_t launch_apgd_w4(bool sparse, unsigned grid, hipStream_t stream, const ApgdParams& P);
#endif

}  // namespace cave
