// vrp_dp.h — the CVRP dynamic program on the device: optimal routes, 0/1 edge indicator, objective and the routes priced
// under a second cost tensor, one 256-thread workgroup per instance (cave_hip_vrp_dp_solve; cave_amd/tight.py
// vrp_solve_hip).
//
// The instance of the reference's vrpModel on the edges of tsp_hk.h: n nodes, node 0 the depot, m = n - 1 customers
// (customer j+1 is bit j) with demands q_j shared by the batch, at most K routes of at least two customers each, every
// route's load <= capacity.  tight.vrp_solve restated (3 <= n <= 14, 1 <= K <= 8, K' = min(K, m / 2)):
//     dp[S, j]  the Held-Karp table of tsp_hk.h (tsp_hk_sweep: the same code)
//     load(S)   = the fp64 sum of q_j over j in S, ascending j, from 0.0;  S feasible: popcount(S) >= 2, load(S) <= capacity
//     r(S)      = min over j in S, ascending, first minimum, of dp[S, j] + D[j+1][0] for feasible S, else +inf
//     g_1 = r;  g_k(S) = min over R, lowbit(S) in R, R a proper subset of S, ascending numeric order of R, first minimum,
//                        of r(R) + g_{k-1}(S \ R)                (one fp64 addition per pair; inf + x = inf never wins)
//     obj       = min over k = 1..K', ascending, first minimum, of g_k(full);  all +inf: CAVE_ST_INFEASIBLE
// and the routes are walked back from (full, k*): R is the argmin of g_k(S), recomputed, its node order the Held-Karp
// walk back through R (closing edge first: the route reads depot -> reversed walk -> depot), then S <- S \ R, k <- k - 1;
// the last route is S itself.  "First minimum in ascending order" is the lexicographic minimum of (value, index), so a
// set whose candidates are spread over the threads (the full set of every layer, the walk back) is reduced in parallel
// on that pair.  Nothing is re-associated: routes, sols and objectives equal the host's bit for bit.
//
// Tables.  The Held-Karp table (m 2^(m-1) doubles) and, for K' >= 2, the partition tables: r and the layers g_2 ..
// g_{K'-1}, (K' - 1) 2^m doubles (layer K' is needed at the full set only; g_k(full) of every layer is reduced in
// parallel and kept in LDS, never stored in a table).  Layers are swept one after the other with a workgroup barrier
// between them; within a layer the sets are independent.  A thread's trip count is 2^(popcount(S) - 1), so the sets are
// dealt in popcount order (the sorted list of tsp_hk.h, once per value of the top bit): the lanes of a wave run equal loops.
//
// Three tiers (vrp_dp_tier): 0 both tables in LDS; 1 the Held-Karp table in the workgroup's slot of a caller-owned
// global workspace, the partition tables -- the randomly read ones -- in LDS; 2 both in the slot.  The tier is a template
// parameter: tables are addressed with LDS or global instructions, not flat ones.  Only its own workgroup reads and
// writes a slot; plain stores of one phase are read after __syncthreads(); no atomics, no cross-workgroup traffic, no
// state between calls.  gridDim.x workgroups stride over the instances, so the workspace does not grow with N.
#pragma once
#include "tsp_hk.h"

namespace cave {

struct VrpDpParams {
  const float* costs;       // [N, d]
  const float* eval_costs;  // [N, d] or null
  const float* demands;     // [m]
  double capacity;
  int64_t N;
  int32_t n, d, K;
  float* sol;               // [N, d] or null
  double* obj;              // [N] or null
  double* eval;             // [N] or null
  int32_t* routes;          // [N, n + K] or null
  int32_t* status;          // [N] or null
  double* ws;               // tiers 1, 2: gridDim.x slots of slot_doubles doubles; tier 0: null
  int64_t slot_doubles;
};

static constexpr int kVrpDpMaxK = 8;
static constexpr int kVrpDpThreads = 256;

CAVE_HOSTDEV bool vrp_dp_valid(int64_t n, int64_t K) { return tsp_hk_valid_n(n) && K >= 1 && K <= kVrpDpMaxK; }
CAVE_HOSTDEV int64_t vrp_dp_kmax(int64_t n, int64_t K) { return K < (n - 1) / 2 ? K : (n - 1) / 2; }
// r and the stored layers g_2 .. g_{K'-1}
CAVE_HOSTDEV int64_t vrp_dp_part_bytes(int64_t n, int64_t K) { return 8 * (vrp_dp_kmax(n, K) - 1) * ((int64_t)1 << (n - 1)); }
// LDS offsets of the per-workgroup arrays (each rounded up to 16 bytes), in this order:
//   D [n n] f64 | cand [16] f64 | priced edges [32] f64 | demands [16] f64 | g_k(full) [16] f64 | reduction values [256]
//   f64 | reduction indices [256] u32 | binomials [14 14] u16 | class offsets [16] u16 | state [16] i32 (0 bad flag,
//   1 remaining set, 2 current node, 3 routes left, 4 route set, 5 entries of the route list) | route list [32] i32 |
//   staged costs [d] f32 | sol [d] f32 | popcount-sorted list [2^(m-1)] u16 | the tables that lie in LDS
struct VrpDpLds {
  uint32_t D, cand, evl, q, gf, redv, redi, bin, off, state, rt, cst, sol, list, tab;
};
CAVE_HOSTDEV VrpDpLds vrp_dp_lds_layout(int64_t n) {
  VrpDpLds L;
  uint32_t p = 0u;
  L.D = p;     p += tsp_hk_r16((uint32_t)(8 * n * n));
  L.cand = p;  p += 128u;
  L.evl = p;   p += 256u;
  L.q = p;     p += 128u;
  L.gf = p;    p += 128u;
  L.redv = p;  p += 8u * (uint32_t)kVrpDpThreads;
  L.redi = p;  p += 4u * (uint32_t)kVrpDpThreads;
  L.bin = p;   p += tsp_hk_r16(2u * 14u * 14u);
  L.off = p;   p += 32u;
  L.state = p; p += 64u;
  L.rt = p;    p += 128u;
  L.cst = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.sol = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.list = p;  p += tsp_hk_r16((uint32_t)(2 * ((int64_t)1 << (n - 2))));
  L.tab = p;
  return L;
}
// 0: both tables in LDS; 1: the Held-Karp table in the workspace slot; 2: both in the slot
CAVE_HOSTDEV int vrp_dp_tier(int64_t n, int64_t K) {
  const int64_t fixed = (int64_t)vrp_dp_lds_layout(n).tab, hk = tsp_hk_table_bytes(n), part = vrp_dp_part_bytes(n, K);
  if (fixed + hk + part <= (int64_t)kTspHkMaxLds) return 0;
  if (fixed + part <= (int64_t)kTspHkMaxLds) return 1;
  return 2;
}
// bytes of one workspace slot: 0 in tier 0
CAVE_HOSTDEV int64_t vrp_dp_slot_bytes(int64_t n, int64_t K) {
  const int t = vrp_dp_tier(n, K);
  return (t >= 1 ? tsp_hk_table_bytes(n) : 0) + (t == 2 ? vrp_dp_part_bytes(n, K) : 0);
}
// LDS of one workgroup
CAVE_HOSTDEV uint32_t vrp_dp_lds_bytes(int64_t n, int64_t K) {
  const int t = vrp_dp_tier(n, K);
  return vrp_dp_lds_layout(n).tab + (uint32_t)((t == 0 ? tsp_hk_table_bytes(n) : 0) + (t <= 1 ? vrp_dp_part_bytes(n, K) : 0));
}


// cave_hip_vrp_dp_solve: its checks, its grid and its parameter block (solver_entry.h)
inline int32_t vrp_dp_plan(const float* costs, const float* eval_costs, const float* demands, double capacity, int64_t K, int64_t N,
                           int64_t n, float* sol, double* obj, double* eval, int32_t* routes, int32_t* status, void* workspace,
                           int64_t workspace_bytes, VrpDpParams* P, int64_t* grid, char* msg) {
  const bool valid = vrp_dp_valid(n, K);
  const int64_t slot = valid ? vrp_dp_slot_bytes(n, K) : 0;
  const int32_t rc = solver_plan(
      "vrp_dp_solve", valid ? nullptr : "need 3 <= n <= 14 and 1 <= K <= 8", eval && !eval_costs, N,
      capacity > 0.0 && capacity <= 1.7976931348623157e308 ? nullptr : "capacity must be finite and positive", 0, slot,
      "this (n, K) needs an 8-byte aligned workspace of at least one slot (cave_hip_vrp_dp_slot_bytes)", workspace, workspace_bytes,
      costs && demands ? nullptr : "costs or demands is null", kTspHkLdsGrid, grid, msg);
  if (rc != CAVE_OK || *grid == 0) return rc;
  tsp_hk_fill(P, costs, eval_costs, N, n, sol, obj, eval, status, workspace, 0, slot);
  P->demands = demands; P->capacity = capacity; P->K = (int32_t)K; P->routes = routes;
  return CAVE_OK;
}

#if defined(CAVE_GPU_CODE)
// The lexicographic minimum of the threads' (v, idx) pairs: afterwards redv[0], redi[0] (every thread may read them until
// the next call).  nt is a power of two.  Called by the whole workgroup.
__device__ inline void vrp_dp_argmin(double v, uint32_t idx, double* redv, uint32_t* redi, int tid, int nt) {
  __syncthreads();  // readers of the reduction before are done
  redv[tid] = v;
  redi[tid] = idx;
  __syncthreads();
  for (int s = nt >> 1; s > 0; s >>= 1) {
    if (tid < s) {
      const double w = redv[tid + s];
      const uint32_t wi = redi[tid + s];
      if (w < redv[tid] || (w == redv[tid] && wi < redi[tid])) {
        redv[tid] = w;
        redi[tid] = wi;
      }
    }
    __syncthreads();
  }
}

// the i-th (ascending) subset of T: the bits of i deposited at the set bits of T
__device__ inline uint32_t vrp_dp_deposit(uint32_t i, uint32_t T) {
  uint32_t r = 0u;
  while (i) {
    const uint32_t b = T & (0u - T);
    if (i & 1u) r |= b;
    T ^= b;
    i >>= 1;
  }
  return r;
}

// g_k(S) with its argmin R (the candidates of S spread over the threads) -> redv[0], redi[0]; prev = g_{k-1}.
// popcount(S) >= 2.  Called by the whole workgroup.
__device__ __forceinline__ void vrp_dp_split(uint32_t S, const double* rtab, const double* prev, double* redv, uint32_t* redi,
                                             int tid, int nt) {
  const uint32_t low = S & (0u - S), T = S ^ low;
  const uint32_t cnt = (1u << (__builtin_popcount(T))) - 1u;  // the subsets of T but T itself (R = S)
  double v = __builtin_inf();
  uint32_t best = 0xFFFFFFFFu;
  for (uint32_t i = (uint32_t)tid; i < cnt; i += (uint32_t)nt) {  // ascending in i: ascending in R
    const uint32_t R = vrp_dp_deposit(i, T) | low;
    const double cd = rtab[R] + prev[S ^ R];
    if (cd < v) {
      v = cd;
      best = R;
    }
  }
  vrp_dp_argmin(v, best, redv, redi, tid, nt);
}

// the whole workgroup: instances blockIdx.x, blockIdx.x + gridDim.x, ...; lds: vrp_dp_lds_bytes(P.n, P.K) bytes, 16-byte
// aligned.  kTier: vrp_dp_tier(P.n, P.K)
template <int kTier>
__device__ inline void vrp_dp_block(const VrpDpParams& P, unsigned char* lds) {
  const int n = P.n, d = P.d, m = n - 1, K = P.K;
  const int kmax = (int)vrp_dp_kmax(n, K);
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const uint32_t half = 1u << (m - 1), nset = 1u << m, full = nset - 1u;
  const VrpDpLds L = vrp_dp_lds_layout(n);
  double* D = reinterpret_cast<double*>(lds + L.D);
  double* cand = reinterpret_cast<double*>(lds + L.cand);
  double* evl = reinterpret_cast<double*>(lds + L.evl);
  double* q = reinterpret_cast<double*>(lds + L.q);
  double* gf = reinterpret_cast<double*>(lds + L.gf);  // gf[k] = g_k(full), k = 1..kmax
  double* redv = reinterpret_cast<double*>(lds + L.redv);
  uint32_t* redi = reinterpret_cast<uint32_t*>(lds + L.redi);
  uint16_t* bin = reinterpret_cast<uint16_t*>(lds + L.bin);
  uint16_t* off = reinterpret_cast<uint16_t*>(lds + L.off);
  int32_t* state = reinterpret_cast<int32_t*>(lds + L.state);
  int32_t* rt = reinterpret_cast<int32_t*>(lds + L.rt);
  float* cst = reinterpret_cast<float*>(lds + L.cst);
  float* sol = reinterpret_cast<float*>(lds + L.sol);
  uint16_t* list = reinterpret_cast<uint16_t*>(lds + L.list);
  double* slot = kTier >= 1 ? P.ws + (size_t)blockIdx.x * (size_t)P.slot_doubles : nullptr;
  const size_t hk_doubles = (size_t)m * (size_t)half;
  double* tab = kTier >= 1 ? slot : reinterpret_cast<double*>(lds + L.tab);
  double* part = kTier == 2 ? slot + hk_doubles : reinterpret_cast<double*>(lds + L.tab) + (kTier == 0 ? hk_doubles : 0);
  // part + (k - 1) nset: g_k, k = 1 (r) .. kmax - 1
  const int nrt = n + K;  // entries of an instance's route list

  // ---- once per workgroup: the list of tsp_hk.h, the demands (a negative or non-finite one fails every instance)
  tsp_hk_build_list(bin, off, list, m, tid, nt);
  if (tid < m) q[tid] = (double)P.demands[tid];
  __syncthreads();
  bool badq = false;
  for (int j = 0; j < m; ++j) badq = badq || !(q[j] >= 0.0 && q[j] <= 1.7976931348623157e308);

  for (int64_t b = (int64_t)blockIdx.x; b < P.N; b += (int64_t)gridDim.x) {
    const size_t row0 = (size_t)b * (size_t)d;
    if (tid == 0) state[0] = 0;
    __syncthreads();  // the instance before is out of the LDS; the list is complete

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
    const bool bad = badq || state[0] != 0;
    for (int e = tid; e < n * n; e += nt) {
      const int a = e / n, c = e - a * n;
      D[e] = a == c ? 0.0 : (double)cst[tsp_hk_eid(a, c, n)];
    }
    __syncthreads();

    double objv = __builtin_nan("");
    int kstar = 0;  // routes of the optimum; 0: none (workgroup-uniform after the layers)
    if (!bad) {  // (workgroup-uniform)
      // ---- the Held-Karp table
      tsp_hk_sweep(tab, D, list, off, n, tid, nt);

      if (kmax >= 2) {
        // ---- r(S), one work item per S
        for (uint32_t S = (uint32_t)tid; S < nset; S += (uint32_t)nt) {
          double v = __builtin_inf();
          if (__builtin_popcount(S) >= 2) {
            double load = 0.0;
            for (uint32_t bits = S; bits; bits &= bits - 1u) load += q[__builtin_ctz(bits)];
            if (load <= P.capacity) {
              uint32_t bits = S;
              int j = __builtin_ctz(bits);
              bits &= bits - 1u;
              v = tab[(uint32_t)j * half + tsp_hk_squeeze(S, j)] + D[(j + 1) * n];
              while (bits) {
                j = __builtin_ctz(bits);
                bits &= bits - 1u;
                const double cd = tab[(uint32_t)j * half + tsp_hk_squeeze(S, j)] + D[(j + 1) * n];
                if (cd < v) v = cd;  // strict: the lowest j wins a tie
              }
            }
          }
          part[S] = v;
        }
        __syncthreads();
        if (tid == 0) gf[1] = part[full];
        // ---- the layers: g_k over all sets but the full one for k < kmax, g_k(full) for every k
        for (int k = 2; k <= kmax; ++k) {
          const double* prev = part + (size_t)(k - 2) * nset;  // g_{k-1}
          if (k < kmax) {
            double* cur = part + (size_t)(k - 1) * nset;
            for (uint32_t it = (uint32_t)tid; it < nset - 1u; it += (uint32_t)nt) {  // (the full set is the last item)
              const uint32_t h = it >= half ? 1u : 0u;
              const uint32_t S = (uint32_t)list[it - h * half] | (h << (m - 1));
              double v = __builtin_inf();
              if (__builtin_popcount(S) >= 2 * k) {  // fewer customers than 2 k: no partition, every pair is infinite
                const uint32_t low = S & (0u - S), T = S ^ low;
                for (uint32_t sub = 0u; sub != T; sub = (sub - T) & T) {  // the subsets of T but T itself, ascending
                  const uint32_t R = sub | low;
                  const double cd = part[R] + prev[S ^ R];
                  if (cd < v) v = cd;  // strict: the lowest R wins a tie
                }
              }
              cur[S] = v;
            }
          }
          vrp_dp_split(full, part, prev, redv, redi, tid, nt);
          if (tid == 0) gf[k] = redv[0];
          __syncthreads();  // layer k is complete
        }
      }
      // ---- the number of routes: the first minimum over k (K' = 1: the closing edge below gives the objective)
      if (tid == 0) {
        int ks = kmax >= 2 ? 0 : 1;
        double v = __builtin_inf();
        for (int k = 1; k <= kmax && kmax >= 2; ++k)
          if (gf[k] < v) {
            v = gf[k];
            ks = k;
          }
        state[3] = ks;
        state[1] = (int32_t)full;
        state[5] = 1;
        rt[0] = 0;
        evl[0] = v;
      }
      __syncthreads();
      kstar = state[3];
      if (kmax >= 2) objv = evl[0];
      if (kmax < 2) {  // one route: feasible when the load of all customers fits (m >= 2 always)
        double load = 0.0;
        for (int j = 0; j < m; ++j) load += q[j];
        if (!(load <= P.capacity)) kstar = 0;
      }
      __syncthreads();  // evl is free again

      // ---- the walk back: route by route, each the Held-Karp walk back through its set
      for (int k = kstar; k >= 1; --k) {
        const uint32_t S = (uint32_t)state[1];
        uint32_t R = S;
        if (k > 1) {
          vrp_dp_split(S, part, part + (size_t)(k - 2) * nset, redv, redi, tid, nt);
          R = redi[0];
          if (R & ~S) R = S;  // (never: g_k(S) is finite on this path, so a pair was found)
        }
        __syncthreads();
        if (tid == 0) {
          state[1] = (int32_t)(S ^ R);
          state[4] = (int32_t)R;
          state[2] = 0;
        }
        __syncthreads();
        const int len = __builtin_popcount(R);
        for (int pos = len; pos >= 1; --pos) {
          const uint32_t Q = (uint32_t)state[4];
          const int jn = state[2];  // the node the path continues to (0: the depot, the closing edge)
          if (tid < m && ((Q >> tid) & 1u)) cand[tid] = tab[(uint32_t)tid * half + tsp_hk_squeeze(Q, tid)] + D[(tid + 1) * n + jn];
          __syncthreads();
          if (tid == 0) {
            uint32_t bits = Q;
            int best = __builtin_ctz(bits);
            bits &= bits - 1u;
            double v = cand[best];
            while (bits) {
              const int c = __builtin_ctz(bits);
              bits &= bits - 1u;
              if (cand[c] < v) {
                v = cand[c];
                best = c;
              }
            }
            if (kmax < 2 && pos == len) evl[0] = v;  // K' = 1: the objective is the closed path
            rt[state[5] + pos - 1] = best + 1;       // the route reads depot -> reversed walk -> depot
            state[4] = (int32_t)(Q & ~(1u << best));
            state[2] = best + 1;
          }
          __syncthreads();
        }
        if (tid == 0) {
          rt[state[5] + len] = 0;
          state[5] += len + 1;
        }
        __syncthreads();
      }
      if (kstar > 0 && kmax < 2) objv = evl[0];
      __syncthreads();
      // ---- the routes' m + k* edges: the 0/1 solution, and the edges priced in route order
      if (kstar > 0 && tid < m + kstar) {
        const int e = tsp_hk_eid(rt[tid], rt[tid + 1], n);
        sol[e] = 1.0f;
        if (P.eval) evl[tid] = (double)CAVE_NT_LOAD_F32(P.eval_costs + row0 + e);
      }
      __syncthreads();
    }
    const bool ok = kstar > 0;

    // ---- outputs
    if (P.sol)
      for (int k = tid; k < d; k += nt) P.sol[row0 + k] = sol[k];
    if (P.routes && tid < nrt) P.routes[(size_t)b * (size_t)nrt + tid] = ok && tid < m + kstar + 1 ? rt[tid] : -1;
    if (tid == 0) {
      if (P.obj) P.obj[b] = ok ? objv : __builtin_nan("");
      if (P.eval) {
        double acc = __builtin_nan("");
        if (ok) {
          acc = 0.0;
          for (int i = 0; i < m + kstar; ++i) acc += evl[i];  // route by route, each from the depot out and back
        }
        P.eval[b] = acc;
      }
      if (P.status) P.status[b] = bad ? CAVE_ST_BAD_INPUT : (ok ? CAVE_ST_OK : CAVE_ST_INFEASIBLE);
    }
  }
}
#endif  // CAVE_GPU_CODE

#if defined(__HIPCC__) && !defined(CAVE_SIMT_EMUL)
// k_vrp_dp.hip: grid workgroups of kVrpDpThreads threads, vrp_dp_lds_bytes(P.n, P.K) bytes of LDS
hipError_t launch_vrp_dp(unsigned grid, hipStream_t stream, const VrpDpParams& P);
#endif

}  // namespace cave
