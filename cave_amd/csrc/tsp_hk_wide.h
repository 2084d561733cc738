// tsp_hk_wide.h — Held-Karp on the device for 13 <= n <= 20: the tier of tsp_hk.h written for a table that lives in HBM
// (cave_hip_tsp_hk_wide_solve; cave_amd/tight.py tsp_solve_hip_wide).  Outputs, semantics and the recurrence are those of
// tsp_hk.h (tight.tsp_solve restated; m = n - 1, node j+1 is bit j, node 0 the depot):
//     dp[{j}, j] = D[0][j+1]
//     dp[S, j]   = min over k in S \ {j}, ascending, of dp[S \ {j}, k] + D[k+1][j+1]    (one fp64 addition per candidate; a
//                  candidate replaces the minimum only when strictly smaller: the lowest k wins a tie)
//     obj        = min over j, ascending, first minimum, of dp[full, j] + D[j+1][0]
// and the walk back recomputes the same argmins.  Nothing is re-associated: bit for bit the host's results.
//
// Table: index(S, j) = j 2^(m-1) + T,  T = S with bit j squeezed out, m 2^(m-1) doubles per slot (tsp_hk.h's layout; 39.8 MB
// at n = 20).  One 512-thread workgroup per instance, workgroups striding over the batch, one slot of the caller's
// workspace per workgroup; only its own workgroup touches a slot, a cardinality's plain stores are read after
// __syncthreads(); no atomics, no cross-workgroup traffic, no state between calls.
//
// Sweep, predecessor-major.  tsp_hk.h's work item is an entry (S, j), which gathers its |S| - 1 candidates: about
// m^2 2^(m-2) eight-byte loads for m 2^(m-1) entries.  Here the work item of cardinality c is a predecessor set S' of
// c - 1 customers: it loads each of its entries dp[S', k] ONCE (k ascending) and folds it into the running minima of all
// m successors dp[S' + {j}, j] at once -- for every j the candidates arrive in ascending k, each one addition and one
// strict comparison, starting from +inf (every candidate is finite: |dp| <= 19 * 3.5e38): the additions and comparisons
// of the entry-major form in the same order, so the same bits.  The minima of the j already in S' are computed and
// dropped (the loop over j is unrolled for the registers' sake; M is a template parameter).  Every table entry is read
// once and written once per instance.  The matrix rows D[k+1][.] come from LDS, m doubles with an odd row stride: the
// lanes of a wave hold different k, and with an odd stride their 8-byte reads fall into different bank pairs.
//
// The sets of a cardinality come from a popcount-sorted list of the m-bit numbers (u32: class offsets reach 2^16 at
// n = 17, so tsp_hk.h's 16-bit types do not carry over), 2^m entries in a header region in front of the slots.  It is
// built once per call by a kernel of its own in front of the sweep (same stream), each number placed by its rank in the
// combinatorial number system: no atomics, no order dependence, never in LDS.
#pragma once
#include "tsp_hk.h"

namespace cave {

static constexpr int kTspHkWideMinN = 13, kTspHkWideMaxN = 20;
static constexpr int kTspHkWideThreads = 512;
static constexpr int kTspHkWideListThreads = 256;
static constexpr int64_t kTspHkWideMaxSlots = 512;                   // default workspace: at most this many slots ...
static constexpr int64_t kTspHkWideMaxBytes = (int64_t)8 << 30;      // ... and at most 8 GiB of them

CAVE_HOSTDEV bool tsp_hk_wide_valid_n(int64_t n) { return n >= kTspHkWideMinN && n <= kTspHkWideMaxN; }
// bytes of one slot: the table, (n-1) 2^(n-2) doubles
CAVE_HOSTDEV int64_t tsp_hk_wide_slot_bytes(int64_t n) { return tsp_hk_table_bytes(n); }
// bytes of the header region: the list, 2^(n-1) u32
CAVE_HOSTDEV int64_t tsp_hk_wide_header_bytes(int64_t n) { return 4 * ((int64_t)1 << (n - 1)); }
// slots of the default workspace: min(512, floor(8 GiB / slot_bytes))
CAVE_HOSTDEV int64_t tsp_hk_wide_default_slots(int64_t n) {
  const int64_t s = kTspHkWideMaxBytes / tsp_hk_wide_slot_bytes(n);
  return s < kTspHkWideMaxSlots ? s : kTspHkWideMaxSlots;
}
// LDS offsets of the per-workgroup arrays (each rounded up to 16 bytes), in this order:
//   D [n n] f64 | Dm [m (m|1)] f64, Dm[k (m|1) + j] = D[k+1][j+1] | cand [32] f64 | priced edges [32] f64 |
//   class offsets [32] u32 | state [16] i32 (0 bad flag, 1 remaining set, 2 current node) | tour [32] i32 |
//   staged costs [d] f32 | sol [d] f32
struct TspHkWideLds {
  uint32_t D, Dm, cand, evl, off, state, tour, cst, sol, end;
};
CAVE_HOSTDEV TspHkWideLds tsp_hk_wide_lds_layout(int64_t n) {
  TspHkWideLds L;
  const int64_t m = n - 1;
  uint32_t p = 0u;
  L.D = p;     p += tsp_hk_r16((uint32_t)(8 * n * n));
  L.Dm = p;    p += tsp_hk_r16((uint32_t)(8 * m * (m | 1)));
  L.cand = p;  p += 256u;
  L.evl = p;   p += 256u;
  L.off = p;   p += 128u;
  L.state = p; p += 64u;
  L.tour = p;  p += 128u;
  L.cst = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.sol = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.end = p;
  return L;
}
CAVE_HOSTDEV uint32_t tsp_hk_wide_lds_bytes(int64_t n) { return tsp_hk_wide_lds_layout(n).end; }
static constexpr uint32_t kTspHkWideListLds = 4u * 20u * 20u;  // the list kernel: Pascal's triangle, bin[p 20 + i] = C(p, i)

// cave_hip_tsp_hk_wide_solve: its checks, its grid and its parameter block (solver_entry.h)
inline int32_t tsp_hk_wide_plan(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                                double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                                TspHkParams* P, int64_t* grid, char* msg) {
  const bool valid = tsp_hk_wide_valid_n(n);
  const int64_t slot = valid ? tsp_hk_wide_slot_bytes(n) : 0, header = valid ? tsp_hk_wide_header_bytes(n) : 0;
  const int32_t rc = solver_plan("tsp_hk_wide_solve", valid ? nullptr : "need 13 <= n <= 20", eval && !eval_costs, N, nullptr, header,
                                 slot, "needs an 8-byte aligned workspace of the header region and at least one slot "
                                 "(cave_hip_tsp_hk_wide_workspace_bytes)",
                                 workspace, workspace_bytes, costs ? nullptr : "costs is null", kTspHkLdsGrid, grid, msg);
  if (rc != CAVE_OK || *grid == 0) return rc;
  tsp_hk_fill(P, costs, eval_costs, N, n, sol, obj, eval, status, workspace, header, slot);
  P->tour = tour; P->list = static_cast<uint32_t*>(workspace);
  return CAVE_OK;
}

#if defined(CAVE_GPU_CODE)
// The list kernel's workgroup: the m-bit numbers blockIdx.x blockDim.x + threadIdx.x, + gridDim.x blockDim.x, ..., each
// placed behind the numbers of fewer bits (class offset) at its rank among the numbers of its popcount.
// lds: kTspHkWideListLds bytes.
__device__ inline void tsp_hk_wide_list_block(uint32_t* list, int m, unsigned char* lds) {
  uint32_t* bin = reinterpret_cast<uint32_t*>(lds);
  if (threadIdx.x == 0) {
    for (int p = 0; p < 20; ++p)
      for (int i = 0; i < 20; ++i) bin[p * 20 + i] = i == 0 ? 1u : (p == 0 ? 0u : bin[(p - 1) * 20 + i - 1] + bin[(p - 1) * 20 + i]);
  }
  __syncthreads();
  const uint32_t total = 1u << m, stride = (uint32_t)gridDim.x * (uint32_t)blockDim.x;
  for (uint32_t T = (uint32_t)blockIdx.x * (uint32_t)blockDim.x + (uint32_t)threadIdx.x; T < total; T += stride) {
    int i;
    const uint32_t rank = hk_rank(T, bin, 20, &i);
    uint32_t base = 0u;  // numbers of m bits with fewer than i bits set
    for (int c = 0; c < i; ++c) base += bin[m * 20 + c];
    list[base + rank] = T;
  }
}

// The table, cardinality by cardinality, predecessor-major.  tab: this workgroup's slot (global memory); Dm in LDS, row
// stride M | 1; off[c]: numbers of M bits with fewer than c bits set.  Ends with a barrier: the table is complete.
template <int M>
__device__ __forceinline__ void tsp_hk_wide_sweep(double* __restrict__ tab, const double* D, const double* Dm,
                                                  const uint32_t* __restrict__ list, const uint32_t* off, int tid, int nt) {
  constexpr uint32_t half = 1u << (M - 1);
  constexpr int ms = M | 1;
  if (tid < M) tab[(size_t)tid * half] = D[tid + 1];  // cardinality 1: dp[{j}, j] = D[0][j+1], T = 0
  __syncthreads();
  for (int c = 2; c <= M; ++c) {
    const uint32_t base = off[c - 1], cnt = off[c] - base;  // the C(M, c-1) predecessor sets
    for (uint32_t it = (uint32_t)tid; it < cnt; it += (uint32_t)nt) {
      const uint32_t Sp = list[base + it];
      // the c - 1 entries of S', k ascending: every lane holds as many (the guards are workgroup-uniform), so all the
      // loads are issued before the first is used
      double x[M - 1];
      int kq[M - 1];
      uint32_t bits = Sp;
#pragma unroll
      for (int i = 0; i < M - 1; ++i)
        if (i < c - 1) {
          const int k = __builtin_ctz(bits);
          bits &= bits - 1u;
          kq[i] = k;
          x[i] = tab[(size_t)k * half + tsp_hk_squeeze(Sp, k)];
        }
      double acc[M];
#pragma unroll
      for (int j = 0; j < M; ++j) acc[j] = __builtin_inf();
#pragma unroll
      for (int i = 0; i < M - 1; ++i)
        if (i < c - 1) {
          const double* Dk = Dm + kq[i] * ms;  // Dk[j] = D[k+1][j+1]
#pragma unroll
          for (int j = 0; j < M; ++j) {
            const double cd = x[i] + Dk[j];
            if (cd < acc[j]) acc[j] = cd;  // strict: the lowest k wins a tie
          }
        }
#pragma unroll
      for (int j = 0; j < M; ++j)
        if (!((Sp >> j) & 1u)) tab[(size_t)j * half + tsp_hk_squeeze(Sp, j)] = acc[j];
    }
    __syncthreads();
  }
}

// the whole workgroup: instances blockIdx.x, blockIdx.x + gridDim.x, ...; lds: tsp_hk_wide_lds_bytes(P.n) bytes, 16-byte
// aligned; P.n == M + 1; P.list complete (the list kernel ran before this one).
template <int M>
__device__ inline void tsp_hk_wide_block(const TspHkParams& P, unsigned char* lds) {
  constexpr int n = M + 1, m = M, ms = M | 1;
  constexpr uint32_t half = 1u << (M - 1);
  const int d = P.d;
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const TspHkWideLds L = tsp_hk_wide_lds_layout(n);
  double* D = reinterpret_cast<double*>(lds + L.D);
  double* Dm = reinterpret_cast<double*>(lds + L.Dm);
  double* cand = reinterpret_cast<double*>(lds + L.cand);
  double* evl = reinterpret_cast<double*>(lds + L.evl);
  uint32_t* off = reinterpret_cast<uint32_t*>(lds + L.off);
  int32_t* state = reinterpret_cast<int32_t*>(lds + L.state);
  int32_t* tourl = reinterpret_cast<int32_t*>(lds + L.tour);
  float* cst = reinterpret_cast<float*>(lds + L.cst);
  float* sol = reinterpret_cast<float*>(lds + L.sol);
  double* tab = P.ws + (size_t)blockIdx.x * (size_t)P.slot_doubles;  // 64-bit: slot offsets pass 4 GiB

  // ---- once per workgroup: the class offsets, off[c] = C(m, 0) + ... + C(m, c-1)
  if (tid == 0) {
    uint64_t b = 1u;  // C(m, c)
    uint32_t acc = 0u;
    for (int c = 0; c <= m + 1; ++c) {
      off[c] = acc;
      acc += (uint32_t)b;
      b = c < m ? b * (uint64_t)(m - c) / (uint64_t)(c + 1) : 0u;
    }
  }

  for (int64_t b = (int64_t)blockIdx.x; b < P.N; b += (int64_t)gridDim.x) {
    const size_t row0 = (size_t)b * (size_t)d;
    if (tid == 0) state[0] = 0;
    __syncthreads();  // the instance before is out of the LDS; the class offsets are complete

    // ---- stage the costs, reject non-finite ones
    bool badl = false;
    for (int k = tid; k < d; k += nt) {
      const float v = CAVE_NT_LOAD_F32(P.costs + row0 + k);
      cst[k] = v;
      sol[k] = 0.0f;
      badl = badl || !(fabsf(v) <= 3.4028234663852886e38f);
    }
    if (badl) state[0] = 1;
    __syncthreads();
    const bool bad = state[0] != 0;
    for (int e = tid; e < n * n; e += nt) {
      const int a = e / n, c = e - a * n;
      const double v = a == c ? 0.0 : (double)cst[tsp_hk_eid(a, c, n)];
      D[e] = v;
      if (a >= 1 && c >= 1) Dm[(a - 1) * ms + c - 1] = v;
    }
    __syncthreads();

    double objv = __builtin_nan("");
    if (!bad) {  // (workgroup-uniform)
      // ---- the table, cardinality by cardinality
      tsp_hk_wide_sweep<M>(tab, D, Dm, P.list, off, tid, nt);
      // ---- closing edge, then the walk back: the minimum over the remaining set's end nodes, recomputed
      if (tid == 0) {
        state[1] = (int32_t)((1u << m) - 1u);
        state[2] = 0;
        tourl[0] = 0;
      }
      __syncthreads();
      for (int pos = m; pos >= 1; --pos) {
        const uint32_t S = (uint32_t)state[1];
        const int jn = state[2];  // the node the path continues to (0: the depot, the closing edge)
        if (tid < m && ((S >> tid) & 1u))
          cand[tid] = tab[(size_t)tid * half + tsp_hk_squeeze(S, tid)] + D[(tid + 1) * n + jn];
        __syncthreads();
        if (tid == 0) {
          uint32_t bits = S;
          int best = __builtin_ctz(bits);
          bits &= bits - 1u;
          double v = cand[best];
          while (bits) {
            const int k = __builtin_ctz(bits);
            bits &= bits - 1u;
            if (cand[k] < v) {
              v = cand[k];
              best = k;
            }
          }
          if (pos == m) objv = v;
          tourl[pos] = best + 1;
          state[1] = (int32_t)(S & ~(1u << best));
          state[2] = best + 1;
        }
        __syncthreads();
      }
      // ---- the tour's n edges: the 0/1 solution, and the edges priced in tour order
      if (tid < n) {
        const int k = tsp_hk_eid(tourl[tid], tourl[tid + 1 < n ? tid + 1 : 0], n);
        sol[k] = 1.0f;
        if (P.eval) evl[tid] = (double)CAVE_NT_LOAD_F32(P.eval_costs + row0 + k);
      }
      __syncthreads();
    }

    // ---- outputs
    if (P.sol)
      for (int k = tid; k < d; k += nt) P.sol[row0 + k] = sol[k];
    if (P.tour && tid < n) P.tour[(size_t)b * (size_t)n + tid] = bad ? -1 : tourl[tid];
    if (tid == 0) {
      if (P.obj) P.obj[b] = objv;
      if (P.eval) {
        double acc = __builtin_nan("");
        if (!bad) {
          acc = 0.0;
          for (int i = 0; i < n; ++i) acc += evl[i];  // left to right, closing edge last
        }
        P.eval[b] = acc;
      }
      if (P.status) P.status[b] = bad ? CAVE_ST_BAD_INPUT : CAVE_ST_OK;
    }
  }
}
#endif  // CAVE_GPU_CODE

#if defined(__HIPCC__) && !defined(CAVE_SIMT_EMUL)
// k_tsp_hk_wide.hip: the list kernel, then grid workgroups of kTspHkWideThreads threads, tsp_hk_wide_lds_bytes(P.n) bytes of LDS
hipError_t launch_tsp_hk_wide(unsigned grid, hipStream_t stream, const TspHkParams& P);
#endif

}  // namespace cave
