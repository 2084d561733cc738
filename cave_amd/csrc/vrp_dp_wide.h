// vrp_dp_wide.h — the CVRP dynamic program on the device for 13 <= n <= 20: the tier of vrp_dp.h written for tables that
// live in HBM (cave_hip_vrp_dp_wide_solve; cave_amd/tight.py vrp_solve_hip_wide).  Outputs, semantics and the recurrences
// are those of vrp_dp.h (tight.vrp_solve restated; m = n - 1, customer j+1 is bit j, node 0 the depot, 1 <= K <= 8,
// K' = min(K, m / 2)):
//     dp[S, j]  the Held-Karp table of tsp_hk_wide.h (tsp_hk_wide_sweep<M>: the same code)
//     load(S)   = the fp64 sum of q_j over j in S, ascending j, from 0.0;  S feasible: popcount(S) >= 2, load(S) <= capacity
//     r(S)      = min over j in S, ascending, first minimum, of dp[S, j] + D[j+1][0] for feasible S, else +inf
//     g_1 = r;  g_k(S) = min over R, lowbit(S) in R, R a proper subset of S, ascending numeric order of R, first minimum,
//                        of r(R) + g_{k-1}(S \ R)
//     obj       = min over k = 1..K', ascending, first minimum, of g_k(full);  all +inf: CAVE_ST_INFEASIBLE
// and the routes are walked back from (full, k*) with the argmins recomputed.  Nothing is re-associated: at n = 13, 14 this
// entry and cave_hip_vrp_dp_solve write the same bytes, and beyond them what tight.vrp_solve would return.
//
// Workspace: tsp_hk_wide.h's header region (the popcount-sorted u32 list of the m-bit numbers, written by the list kernel
// in front of this one on the same stream), then one slot per workgroup: the Held-Karp table, m 2^(m-1) doubles, then r and
// the stored layers g_2 .. g_{K'-1}, (K' - 1) 2^m doubles (nothing for K' = 1).  One 512-thread workgroup per instance,
// workgroups striding over the batch.  Only its own workgroup touches a slot; plain stores of one phase are read after
// __syncthreads(); no atomics, no cross-workgroup traffic, no waiting on another workgroup, no state between calls.
// Set arithmetic is 32-bit (class offsets reach 2^16 at n = 17, a set has 19 bits at n = 20), slot offsets are 64-bit.
//
// The candidates of a set.  A pair (S, R) costs two 8-byte reads at random places of two 2^m-double tables and one
// addition; the reads are the cost.  Every scan of candidates (vrp_dp_wide_scan) walks the subsets sub of a mask in
// ascending order, four at a time, so that eight reads are in flight per lane.  It walks ALL 2^p subsets, the mask itself
// too -- the candidate R = S, which the recurrence excludes: its pair is r(S) + g_{k-1}(empty) = x + inf = +inf (r is
// finite or +inf, never -inf or NaN), which is not strictly below any minimum, so neither a value nor an argmin changes.
//
// How the sets of a layer are dealt.  A set of popcount c costs 2^(c-1) pairs.  The sets are taken in popcount order from
// the header's list, one set per thread, so the lanes of a wave run equal loops -- except the classes that have fewer sets
// than the workgroup has threads AND at least 8 x 512 pairs per set (c >= 13 with C(m, c) < 512: c = 17, 18 at n = 20).
// One thread per set would leave most of the workgroup idle behind a few lanes running up to 2^17 trips each; these sets
// go to the whole workgroup one after the other, their candidates spread over the threads and reduced on (value, R) as
// the full set's are (vrp_dp_wide_split).  The lexicographic minimum of (value, R) IS the first minimum in ascending R,
// so both ways give the same bits.
#pragma once
#include "tsp_hk_wide.h"
#include "vrp_dp.h"

namespace cave {

struct VrpDpWideParams {
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
  uint32_t* list;           // the popcount-sorted list in the workspace's header region
  double* ws;               // gridDim.x slots of slot_doubles doubles
  int64_t slot_doubles;
};

static constexpr int kVrpDpWideThreads = 512;
#ifndef CAVE_VRP_DP_WIDE_GROUP_PAIRS  // (an A/B build of tools/diag/build_variant.sh sets it: 0x80000000u = one set per thread throughout)
#define CAVE_VRP_DP_WIDE_GROUP_PAIRS (8u * 512u)
#endif
static constexpr uint32_t kVrpDpWideGroupPairs = CAVE_VRP_DP_WIDE_GROUP_PAIRS;  // a class goes to the whole workgroup from this many pairs per set

CAVE_HOSTDEV bool vrp_dp_wide_valid(int64_t n, int64_t K) { return tsp_hk_wide_valid_n(n) && K >= 1 && K <= kVrpDpMaxK; }
// r and the stored layers g_2 .. g_{K'-1}
CAVE_HOSTDEV int64_t vrp_dp_wide_part_bytes(int64_t n, int64_t K) { return 8 * (vrp_dp_kmax(n, K) - 1) * ((int64_t)1 << (n - 1)); }
// bytes of one slot: the Held-Karp table, then the partition tables
CAVE_HOSTDEV int64_t vrp_dp_wide_slot_bytes(int64_t n, int64_t K) { return tsp_hk_table_bytes(n) + vrp_dp_wide_part_bytes(n, K); }
// slots of the default workspace: min(512, floor(8 GiB / slot_bytes))
CAVE_HOSTDEV int64_t vrp_dp_wide_default_slots(int64_t n, int64_t K) {
  const int64_t s = kTspHkWideMaxBytes / vrp_dp_wide_slot_bytes(n, K);
  return s < kTspHkWideMaxSlots ? s : kTspHkWideMaxSlots;
}
// LDS offsets of the per-workgroup arrays (each rounded up to 16 bytes), in this order:
//   D [n n] f64 | Dm [m (m|1)] f64 (tsp_hk_wide.h) | cand [32] f64 | priced edges [32] f64 | demands [32] f64 |
//   g_k(full) [16] f64 | reduction values [512] f64 | reduction indices [512] u32 | class offsets [32] u32 | state [16] i32
//   (0 bad flag, 1 remaining set, 2 current node, 3 routes left, 4 route set, 5 entries of the route list) |
//   route list [32] i32 | staged costs [d] f32 | sol [d] f32
struct VrpDpWideLds {
  uint32_t D, Dm, cand, evl, q, gf, redv, redi, off, state, rt, cst, sol, end;
};
CAVE_HOSTDEV VrpDpWideLds vrp_dp_wide_lds_layout(int64_t n) {
  VrpDpWideLds L;
  const int64_t m = n - 1;
  uint32_t p = 0u;
  L.D = p;     p += tsp_hk_r16((uint32_t)(8 * n * n));
  L.Dm = p;    p += tsp_hk_r16((uint32_t)(8 * m * (m | 1)));
  L.cand = p;  p += 256u;
  L.evl = p;   p += 256u;
  L.q = p;     p += 256u;
  L.gf = p;    p += 128u;
  L.redv = p;  p += 8u * (uint32_t)kVrpDpWideThreads;
  L.redi = p;  p += 4u * (uint32_t)kVrpDpWideThreads;
  L.off = p;   p += 128u;
  L.state = p; p += 64u;
  L.rt = p;    p += 128u;
  L.cst = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.sol = p;   p += tsp_hk_r16((uint32_t)(4 * tsp_hk_edges(n)));
  L.end = p;
  return L;
}
CAVE_HOSTDEV uint32_t vrp_dp_wide_lds_bytes(int64_t n) { return vrp_dp_wide_lds_layout(n).end; }

// cave_hip_vrp_dp_wide_solve: its checks, its grid and its parameter block (solver_entry.h)
inline int32_t vrp_dp_wide_plan(const float* costs, const float* eval_costs, const float* demands, double capacity, int64_t K,
                                int64_t N, int64_t n, float* sol, double* obj, double* eval, int32_t* routes, int32_t* status,
                                void* workspace, int64_t workspace_bytes, VrpDpWideParams* P, int64_t* grid, char* msg) {
  const bool valid = vrp_dp_wide_valid(n, K);
  const int64_t slot = valid ? vrp_dp_wide_slot_bytes(n, K) : 0, header = valid ? tsp_hk_wide_header_bytes(n) : 0;
  const int32_t rc = solver_plan(
      "vrp_dp_wide_solve", valid ? nullptr : "need 13 <= n <= 20 and 1 <= K <= 8", eval && !eval_costs, N,
      capacity > 0.0 && capacity <= 1.7976931348623157e308 ? nullptr : "capacity must be finite and positive", header, slot,
      "needs an 8-byte aligned workspace of the header region and at least one slot (cave_hip_vrp_dp_wide_workspace_bytes)",
      workspace, workspace_bytes, costs && demands ? nullptr : "costs or demands is null", kTspHkLdsGrid, grid, msg);
  if (rc != CAVE_OK || *grid == 0) return rc;
  tsp_hk_fill(P, costs, eval_costs, N, n, sol, obj, eval, status, workspace, header, slot);
  P->demands = demands; P->capacity = capacity; P->K = (int32_t)K; P->routes = routes;
  P->list = static_cast<uint32_t*>(workspace);
  return CAVE_OK;
}

#if defined(CAVE_GPU_CODE)
// The candidates R = sub | B of S, sub over ALL subsets of the mask Tm in ascending order (B: the bits every R holds),
// folded into the running first minimum (v, best): r(R) + prev(S \ R), one addition and one strict comparison each.
__device__ __forceinline__ void vrp_dp_wide_scan(uint32_t Tm, uint32_t B, uint32_t S, const double* __restrict__ rtab,
                                                 const double* __restrict__ prev, double& v, uint32_t& best) {
  const uint32_t cnt = 1u << __builtin_popcount(Tm);
  uint32_t sub = 0u;
  if (cnt >= 4u) {
    for (uint32_t i = 0u; i < cnt; i += 4u) {  // (after the mask itself the walk wraps to 0: cnt is a multiple of 4)
      const uint32_t R0 = sub | B;
      sub = (sub - Tm) & Tm;
      const uint32_t R1 = sub | B;
      sub = (sub - Tm) & Tm;
      const uint32_t R2 = sub | B;
      sub = (sub - Tm) & Tm;
      const uint32_t R3 = sub | B;
      sub = (sub - Tm) & Tm;
      const double a0 = rtab[R0], a1 = rtab[R1], a2 = rtab[R2], a3 = rtab[R3];
      const double b0 = prev[S ^ R0], b1 = prev[S ^ R1], b2 = prev[S ^ R2], b3 = prev[S ^ R3];
      const double c0 = a0 + b0, c1 = a1 + b1, c2 = a2 + b2, c3 = a3 + b3;
      if (c0 < v) { v = c0; best = R0; }  // strict: the lowest R wins a tie
      if (c1 < v) { v = c1; best = R1; }
      if (c2 < v) { v = c2; best = R2; }
      if (c3 < v) { v = c3; best = R3; }
    }
  } else {
    for (uint32_t i = 0u; i < cnt; ++i) {
      const uint32_t R = sub | B;
      sub = (sub - Tm) & Tm;
      const double cd = rtab[R] + prev[S ^ R];
      if (cd < v) { v = cd; best = R; }
    }
  }
}

// g_k(S) with its argmin R (the candidates of S spread over the threads) -> redv[0], redi[0]; prev = g_{k-1}.  Thread tid
// takes the subsets number tid, tid + nt, ... of T = S \ lowbit(S): its number's low log2(nt) bits are deposited once at
// the lowest set bits of T, the rest walks the subsets of the remaining bits -- ascending in the number, so ascending in
// R.  popcount(S) >= 2; nt is a power of two.  Called by the whole workgroup.
__device__ __forceinline__ void vrp_dp_wide_split(uint32_t S, const double* __restrict__ rtab, const double* __restrict__ prev,
                                                  double* redv, uint32_t* redi, int tid, int nt) {
  const uint32_t low = S & (0u - S), T = S ^ low;
  uint32_t Thi = T;
  for (int i = __builtin_ctz((uint32_t)nt); i > 0 && Thi; --i) Thi &= Thi - 1u;
  const uint32_t Tlo = T ^ Thi;
  double v = __builtin_inf();
  uint32_t best = 0xFFFFFFFFu;
  if ((uint32_t)tid < (1u << __builtin_popcount(Tlo)))
    vrp_dp_wide_scan(Thi, vrp_dp_deposit((uint32_t)tid, Tlo) | low, S, rtab, prev, v, best);
  vrp_dp_argmin(v, best, redv, redi, tid, nt);
}

// the whole workgroup: instances blockIdx.x, blockIdx.x + gridDim.x, ...; lds: vrp_dp_wide_lds_bytes(P.n) bytes, 16-byte
// aligned; P.n == M + 1; P.list complete (the list kernel ran before this one).
template <int M>
__device__ inline void vrp_dp_wide_block(const VrpDpWideParams& P, unsigned char* lds) {
  constexpr int n = M + 1, m = M, ms = M | 1;
  constexpr uint32_t half = 1u << (M - 1), nset = 1u << M, full = nset - 1u;
  const int d = P.d, K = P.K;
  const int kmax = (int)vrp_dp_kmax(n, K);
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const VrpDpWideLds L = vrp_dp_wide_lds_layout(n);
  double* D = reinterpret_cast<double*>(lds + L.D);
  double* Dm = reinterpret_cast<double*>(lds + L.Dm);
  double* cand = reinterpret_cast<double*>(lds + L.cand);
  double* evl = reinterpret_cast<double*>(lds + L.evl);
  double* q = reinterpret_cast<double*>(lds + L.q);
  double* gf = reinterpret_cast<double*>(lds + L.gf);  // gf[k] = g_k(full), k = 1..kmax
  double* redv = reinterpret_cast<double*>(lds + L.redv);
  uint32_t* redi = reinterpret_cast<uint32_t*>(lds + L.redi);
  uint32_t* off = reinterpret_cast<uint32_t*>(lds + L.off);  // off[c]: numbers of m bits with fewer than c bits set
  int32_t* state = reinterpret_cast<int32_t*>(lds + L.state);
  int32_t* rt = reinterpret_cast<int32_t*>(lds + L.rt);
  float* cst = reinterpret_cast<float*>(lds + L.cst);
  float* sol = reinterpret_cast<float*>(lds + L.sol);
  double* tab = P.ws + (size_t)blockIdx.x * (size_t)P.slot_doubles;  // 64-bit: slot offsets pass 4 GiB
  double* part = tab + (size_t)m * (size_t)half;                     // part + (k - 1) nset: g_k, k = 1 (r) .. kmax - 1
  const uint32_t* __restrict__ list = P.list;
  const int nrt = n + K;  // entries of an instance's route list

  // ---- once per workgroup: the class offsets, the demands (a negative or non-finite one fails every instance)
  if (tid == 0) {
    uint64_t b = 1u;  // C(m, c)
    uint32_t acc = 0u;
    for (int c = 0; c <= m + 1; ++c) {
      off[c] = acc;
      acc += (uint32_t)b;
      b = c < m ? b * (uint64_t)(m - c) / (uint64_t)(c + 1) : 0u;
    }
  }
  if (tid < m) q[tid] = (double)P.demands[tid];
  __syncthreads();
  bool badq = false;
  for (int j = 0; j < m; ++j) badq = badq || !(q[j] >= 0.0 && q[j] <= 1.7976931348623157e308);

  for (int64_t b = (int64_t)blockIdx.x; b < P.N; b += (int64_t)gridDim.x) {
    const size_t row0 = (size_t)b * (size_t)d;
    if (tid == 0) state[0] = 0;
    __syncthreads();  // the instance before is out of the LDS

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
      const double v = a == c ? 0.0 : (double)cst[tsp_hk_eid(a, c, n)];
      D[e] = v;
      if (a >= 1 && c >= 1) Dm[(a - 1) * ms + c - 1] = v;
    }
    __syncthreads();

    double objv = __builtin_nan("");
    int kstar = 0;  // routes of the optimum; 0: none (workgroup-uniform after the layers)
    if (!bad) {  // (workgroup-uniform)
      // ---- the Held-Karp table
      tsp_hk_wide_sweep<M>(tab, D, Dm, list, off, tid, nt);

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
            // the first class that goes to the whole workgroup (m: none; classes only get smaller behind the middle one)
            int cg = m;
            while (cg - 1 >= 2 * k && cg - 1 > m / 2 && off[cg] - off[cg - 1] < (uint32_t)nt &&
                   (1u << (cg - 2)) >= kVrpDpWideGroupPairs)
              --cg;
            const uint32_t own_end = off[cg];  // the list below it: a set per thread (the full set is the list's last entry)
            for (uint32_t it = (uint32_t)tid; it < own_end; it += (uint32_t)nt) {
              const uint32_t S = list[it];
              double v = __builtin_inf();
              if (__builtin_popcount(S) >= 2 * k) {  // fewer customers than 2 k: no partition, every pair is infinite
                const uint32_t low = S & (0u - S);
                uint32_t unused = 0u;
                vrp_dp_wide_scan(S ^ low, low, S, part, prev, v, unused);
              }
              cur[S] = v;
            }
            for (uint32_t it = own_end; it < nset - 1u; ++it) {  // (workgroup-uniform)
              const uint32_t S = list[it];
              vrp_dp_wide_split(S, part, prev, redv, redi, tid, nt);
              if (tid == 0) cur[S] = redv[0];
            }
          }
          vrp_dp_wide_split(full, part, prev, redv, redi, tid, nt);
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
      if (kmax < 2) {  // one route: feasible when the load of all customers fits
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
          vrp_dp_wide_split(S, part, part + (size_t)(k - 2) * nset, redv, redi, tid, nt);
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
// k_vrp_dp_wide.hip: the list kernel, then grid workgroups of kVrpDpWideThreads threads, vrp_dp_wide_lds_bytes(P.n) bytes of LDS
hipError_t launch_vrp_dp_wide(unsigned grid, hipStream_t stream, const VrpDpWideParams& P);
#endif

}  // namespace cave
