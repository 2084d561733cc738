// tsp_hk.h — Held-Karp on the device: optimal tour, 0/1 edge indicator, objective and the tour priced under a second cost
// tensor, one 256-thread workgroup per instance (cave_hip_tsp_hk_solve; cave_amd/tight.py tsp_solve_hip).
//
// The symmetric TSP of cave_amd.synth.tsp_edges: edges in lexicographic (i<j) order, d = n (n-1) / 2,
//     eid(i,j) = i n - i (i+1) / 2 + j - i - 1,        D[a][b] = (double)cost[eid(a,b)],        3 <= n <= 14.
// tight.tsp_solve restated (m = n - 1, node j+1 is bit j, node 0 the depot):
//     dp[{j}, j] = D[0][j+1]                                               (no addition)
//     dp[S, j]   = min over k in S \ {j}, ascending, of dp[S \ {j}, k] + D[k+1][j+1]    (one fp64 addition per candidate; a
//                  candidate replaces the minimum only when strictly smaller: the lowest k wins a tie, np.argmin's rule)
//     obj        = min over j, ascending, first minimum, of dp[full, j] + D[j+1][0]
// and the tour is walked back through the same argmins, which are recomputed (the additions and comparisons of the
// forward sweep again: the same bits, the same k) instead of stored.  Nothing is re-associated: tours, sols and
// objectives equal the host's bit for bit.
//
// Table.  Only entries with j in S exist:  index(S, j) = j 2^(m-1) + T,  T = S with bit j squeezed out (m-1 bits),
// m 2^(m-1) doubles.  An entry has exactly one predecessor set, so the entries of one cardinality are independent: the
// table is swept cardinality by cardinality with a workgroup barrier between cardinalities.  A cardinality c is the
// work items (j, T) with popcount(T) = c - 1: m C(m-1, c-1) of them, T taken from a popcount-sorted list of the m-1 bit
// numbers that the workgroup builds once (each number placed by its rank in the combinatorial number system: no
// atomics, no order dependence).  Items are dealt to the threads round robin, whatever their count.
//
// Two tiers (tsp_hk_slot_bytes): up to n = 12 the table (90 112 B) lies in LDS beside D and the list; for n = 13, 14
// (196 608 B, 425 984 B) it lies in a slot of a caller-owned global workspace.  Only its own workgroup reads and writes
// a slot: a cardinality's plain stores are read after __syncthreads() (workgroup-scope release / acquire, one compute
// unit, one L1), there is no cross-workgroup traffic, no atomics and no state between calls.  gridDim.x workgroups
// stride over the instances, so the workspace does not grow with N and a slot is reused by later instances.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cave_hip.h"
#include "cone_common.h"
#include "solver_entry.h"

namespace cave {

struct TspHkParams {
  const float* costs;       // [N, d]
  const float* eval_costs;  // [N, d] or null
  int64_t N;
  int32_t n, d;
  float* sol;               // [N, d] or null
  double* obj;              // [N] or null
  double* eval;             // [N] or null
  int32_t* tour;            // [N, n] or null
  int32_t* status;          // [N] or null
  uint32_t* list;           // wide tier (tsp_hk_wide.h): the popcount-sorted list in the workspace's header region; else null
  double* ws;               // global tier: gridDim.x slots of slot_doubles doubles; LDS tier: null
  int64_t slot_doubles;
};

static constexpr uint32_t kTspHkMaxLds = 160u * 1024u;
static constexpr int kTspHkMinN = 3, kTspHkMaxN = 14;
static constexpr int kTspHkThreads = 256;
static constexpr int64_t kTspHkDefaultSlots = 512;  // global tier: workgroups (= slots) of the default workspace
static constexpr int64_t kTspHkLdsGrid = 2048;      // LDS tier: at most this many workgroups stride over the batch

CAVE_HOSTDEV uint32_t tsp_hk_r16(uint32_t x) { return (x + 15u) & ~15u; }
CAVE_HOSTDEV int64_t tsp_hk_edges(int64_t n) { return n * (n - 1) / 2; }
CAVE_HOSTDEV int64_t tsp_hk_table_bytes(int64_t n) { return 8 * (n - 1) * ((int64_t)1 << (n - 2)); }
// LDS offsets of the per-workgroup arrays (each rounded up to 16 bytes), in this order:
//   D [n n] f64 | cand [16] f64 | priced edges [16] f64 | binomials [14 14] u16 | class offsets [16] u16 |
//   state [16] i32 (0 bad flag, 1 remaining set, 2 current node) | tour [16] i32 | staged costs [d] f32 | sol [d] f32 |
//   popcount-sorted list [2^(m-1)] u16 | (LDS tier) the table
struct TspHkLds {
  uint32_t D, cand, evl, bin, off, state, tour, cst, sol, list, tab;
};
CAVE_HOSTDEV TspHkLds tsp_hk_lds_layout(int64_t n) {
  TspHkLds L;
  uint32_t p = 0u;
  L.D = p;     p += tsp_hk_r16((uint32_t)(8 * n * n));
  L.cand = p;  p += 128u;
  L.evl = p;   p += 128u;
  L.bin = p;   p += tsp_hk_r16(2u * 14u * 14u);
  L.off = p;   p += 32u;
  L.state = p; p += 64u;
  L.tour = p;  p += 64u;
  L.cst = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.sol = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.list = p;  p += tsp_hk_r16((uint32_t)(2 * ((int64_t)1 << (n - 2))));
  L.tab = p;
  return L;
}
CAVE_HOSTDEV bool tsp_hk_valid_n(int64_t n) { return n >= kTspHkMinN && n <= kTspHkMaxN; }
// the table lies in LDS when it fits beside the other arrays
CAVE_HOSTDEV bool tsp_hk_in_lds(int64_t n) {
  return (int64_t)tsp_hk_lds_layout(n).tab + tsp_hk_table_bytes(n) <= (int64_t)kTspHkMaxLds;
}
// bytes of one workspace slot: 0 in the LDS tier
CAVE_HOSTDEV int64_t tsp_hk_slot_bytes(int64_t n) { return tsp_hk_in_lds(n) ? 0 : tsp_hk_table_bytes(n); }
// LDS of one workgroup
CAVE_HOSTDEV uint32_t tsp_hk_lds_bytes(int64_t n) {
  return tsp_hk_lds_layout(n).tab + (tsp_hk_in_lds(n) ? (uint32_t)tsp_hk_table_bytes(n) : 0u);
}

// The fields both Held-Karp tiers and the CVRP fill alike: the tensors, the sizes and the workspace behind its header
template <class Params>
inline void tsp_hk_fill(Params* P, const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                        double* eval, int32_t* status, void* workspace, int64_t header, int64_t slot) {
  P->costs = costs; P->eval_costs = eval_costs; P->N = N; P->n = (int32_t)n; P->d = (int32_t)tsp_hk_edges(n);
  P->sol = sol; P->obj = obj; P->eval = eval; P->status = status;
  P->ws = slot > 0 ? reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + header) : nullptr;
  P->slot_doubles = slot / 8;
}
// cave_hip_tsp_hk_solve: its checks, its grid and its parameter block (solver_entry.h)
inline int32_t tsp_hk_plan(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj, double* eval,
                           int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes, TspHkParams* P, int64_t* grid,
                           char* msg) {
  const bool valid = tsp_hk_valid_n(n);
  const int64_t slot = valid ? tsp_hk_slot_bytes(n) : 0;
  const int32_t rc = solver_plan("tsp_hk_solve", valid ? nullptr : "need 3 <= n <= 14", eval && !eval_costs, N, nullptr, 0, slot,
                                 "this n needs an 8-byte aligned workspace of at least one slot (cave_hip_tsp_hk_slot_bytes)",
                                 workspace, workspace_bytes, costs ? nullptr : "costs is null", kTspHkLdsGrid, grid, msg);
  if (rc != CAVE_OK || *grid == 0) return rc;
  tsp_hk_fill(P, costs, eval_costs, N, n, sol, obj, eval, status, workspace, 0, slot);
  P->tour = tour; P->list = nullptr;
  return CAVE_OK;
}

#if defined(CAVE_GPU_CODE)
__device__ inline int tsp_hk_eid(int a, int b, int n) {  // a != b
  const int i = a < b ? a : b, j = a < b ? b : a;
  return i * n - i * (i + 1) / 2 + j - i - 1;
}
// S with bit k (set or not) squeezed out
__device__ inline uint32_t tsp_hk_squeeze(uint32_t S, int k) { return (S & ((1u << k) - 1u)) | ((S >> (k + 1)) << k); }

// Combinatorial number system: the rank of T among the numbers with its popcount (-> *pop); bin[p stride + i] = C(p, i)
// (shared with tsp_hk_wide.h, whose binomials are wider)
template <class B>
__device__ __forceinline__ uint32_t hk_rank(uint32_t T, const B* bin, int stride, int* pop) {
  uint32_t rank = 0u;
  int i = 0;
  while (T) {
    const int p = __builtin_ctz(T);
    T &= T - 1u;
    ++i;
    rank += bin[p * stride + i];
  }
  *pop = i;
  return rank;
}

// Once per workgroup (shared with vrp_dp.h): Pascal's triangle bin[p 14 + i] = C(p, i), the class offsets off[c] (numbers
// of m-1 bits with fewer than c bits set) and the popcount-sorted list of the m-1 bit numbers.  Ends without a barrier:
// the list is complete after the caller's next __syncthreads().
__device__ __forceinline__ void tsp_hk_build_list(uint16_t* bin, uint16_t* off, uint16_t* list, int m, int tid, int nt) {
  const uint32_t half = 1u << (m - 1);
  if (tid == 0) {
    for (int p = 0; p < 14; ++p)
      for (int i = 0; i < 14; ++i)
        bin[p * 14 + i] = (uint16_t)(i == 0 ? 1 : (p == 0 ? 0 : bin[(p - 1) * 14 + i - 1] + bin[(p - 1) * 14 + i]));
    uint32_t acc = 0u;
    for (int c = 0; c <= m; ++c) {
      off[c] = (uint16_t)acc;
      if (c < m) acc += bin[(m - 1) * 14 + c];
    }
  }
  __syncthreads();
  for (uint32_t T = (uint32_t)tid; T < half; T += (uint32_t)nt) {
    int i;
    const uint32_t rank = hk_rank(T, bin, 14, &i);
    list[off[i] + rank] = (uint16_t)T;
  }
}

// The table, cardinality by cardinality (shared with vrp_dp.h); tab in LDS or global memory, its address space known
// where this is inlined.  Ends with a barrier: the table is complete.
__device__ __forceinline__ void tsp_hk_sweep(double* tab, const double* D, const uint16_t* list, const uint16_t* off, int n,
                                             int tid, int nt) {
  const int m = n - 1;
  const uint32_t half = 1u << (m - 1);
  for (int c = 1; c <= m; ++c) {
    const int base = (int)off[c - 1], cnt = (int)off[c] - base;  // C(m-1, c-1)
    const int items = m * cnt;
    for (int it = tid; it < items; it += nt) {
      const int j = it / cnt;
      const uint32_t T = list[base + it - j * cnt];
      double v;
      if (c == 1) {
        v = D[j + 1];
      } else {
        uint32_t Sp = (T & ((1u << j) - 1u)) | ((T >> j) << (j + 1));  // S \ {j}, m bits
        const double* Dj = D + (j + 1) * n + 1;                        // Dj[k] = D[j+1][k+1] = D[k+1][j+1]
        int k = __builtin_ctz(Sp);
        const uint32_t S0 = Sp;
        Sp &= Sp - 1u;
        v = tab[(uint32_t)k * half + tsp_hk_squeeze(S0, k)] + Dj[k];
        while (Sp) {
          k = __builtin_ctz(Sp);
          Sp &= Sp - 1u;
          const double cd = tab[(uint32_t)k * half + tsp_hk_squeeze(S0, k)] + Dj[k];
          if (cd < v) v = cd;  // strict: the lowest k wins a tie
        }
      }
      tab[(uint32_t)j * half + T] = v;
    }
    __syncthreads();
  }
}

// the whole workgroup: instances blockIdx.x, blockIdx.x + gridDim.x, ...; lds: tsp_hk_lds_bytes(P.n) bytes, 16-byte aligned.
// kWs: the table lies in this workgroup's workspace slot (a template parameter, so that the table's address space is
// known at compile time: LDS or global instructions, not flat ones)
template <bool kWs>
__device__ inline void tsp_hk_block(const TspHkParams& P, unsigned char* lds) {
  const int n = P.n, d = P.d, m = n - 1;
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const uint32_t half = 1u << (m - 1);
  const TspHkLds L = tsp_hk_lds_layout(n);
  double* D = reinterpret_cast<double*>(lds + L.D);
  double* cand = reinterpret_cast<double*>(lds + L.cand);
  double* evl = reinterpret_cast<double*>(lds + L.evl);
  uint16_t* bin = reinterpret_cast<uint16_t*>(lds + L.bin);  // bin[p 14 + i] = C(p, i)
  uint16_t* off = reinterpret_cast<uint16_t*>(lds + L.off);  // off[c]: numbers of m-1 bits with fewer than c bits set
  int32_t* state = reinterpret_cast<int32_t*>(lds + L.state);
  int32_t* tourl = reinterpret_cast<int32_t*>(lds + L.tour);
  float* cst = reinterpret_cast<float*>(lds + L.cst);
  float* sol = reinterpret_cast<float*>(lds + L.sol);
  uint16_t* list = reinterpret_cast<uint16_t*>(lds + L.list);
  double* tab = kWs ? P.ws + (size_t)blockIdx.x * (size_t)P.slot_doubles : reinterpret_cast<double*>(lds + L.tab);

  // ---- once per workgroup: Pascal's triangle, the class offsets, the popcount-sorted list
  tsp_hk_build_list(bin, off, list, m, tid, nt);

  for (int64_t b = (int64_t)blockIdx.x; b < P.N; b += (int64_t)gridDim.x) {
    const size_t row0 = (size_t)b * (size_t)d;
    if (tid == 0) state[0] = 0;
    __syncthreads();  // the instance before is out of the LDS; the list is complete

    // ---- stage the costs (a row starts wherever b d puts it: dword loads), reject non-finite ones
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
      D[e] = a == c ? 0.0 : (double)cst[tsp_hk_eid(a, c, n)];
    }
    __syncthreads();

    double objv = __builtin_nan("");
    if (!bad) {  // (workgroup-uniform)
      // ---- the table, cardinality by cardinality
      tsp_hk_sweep(tab, D, list, off, n, tid, nt);
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
        if (tid < m && ((S >> tid) & 1u)) cand[tid] = tab[(uint32_t)tid * half + tsp_hk_squeeze(S, tid)] + D[(tid + 1) * n + jn];
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
// k_tsp_hk.hip: grid workgroups of kTspHkThreads threads, tsp_hk_lds_bytes(P.n) bytes of LDS
hipError_t launch_tsp_hk(unsigned grid, hipStream_t stream, const TspHkParams& P);
#endif

}  // namespace cave
