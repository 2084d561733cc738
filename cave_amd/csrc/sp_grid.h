// sp_grid.h — grid shortest path on the device: solve, backtrack, regret numerator and the tight cone in the sparse
// wire format, one 64-lane wave per instance (cave_hip_sp_grid_solve; cave_amd/tight.py sp_solve_hip / sp_cones_hip).
//
// The h x w grid DAG of cave_amd.synth.sp_arcs: per grid row i its w-1 right arcs, then (i < h-1) its w down arcs, so
//     right arc (i,j) -> (i,j+1):  k = i (2w-1) + j            down arc (i,j) -> (i+1,j):  k = i (2w-1) + (w-1) + j
// and d = h (w-1) + (h-1) w.  tight.sp_solve relaxes the arcs in index order with a strict "<" on fp64 distances; the
// down arc into a node has the lower index, hence   dist(i,j) = (right < down) ? right : down   with
// right = dist(i,j-1) + (double)c[right arc], down = dist(i-1,j) + (double)c[down arc].  The kernel performs exactly
// these additions and comparisons on an ANTI-DIAGONAL sweep: lane l owns column c0 + l of a 64-column strip and is at
// row t - l in step t; its own previous value is dist(i-1,j), the previous value of lane l-1 (one DPP shift) is
// dist(i,j-1).  Strips run left to right; the last column of a strip is handed to the next through LDS.  Any number of
// rows is a longer sweep.  Nothing is re-associated: paths and objectives equal the host's bit for bit.
//
// Per wave, in LDS (sp_grid_wave_lds_bytes): the d costs (staged with coalesced dword loads; after the sweep the same
// array holds the 0/1 solution), one predecessor byte per node (1: entered by its right arc), and for w > 64 the h
// fp64 distances of a strip's last column.  Lane 0 backtracks h + w - 2 dependent LDS reads.  No atomics, no global
// scratch, no state between calls; workgroups of 4 (2, 1 for very large grids) independent waves, no barrier.
//
// Tight cone of the vertex, the entries SparseCones.from_ragged([tight.sp_tight_normals(sol, h, w)]) produces: rows
// [N; -N; -e_k for arcs at 0; +e_k for arcs at 1], N = +1 on an arc's head node and -1 on its tail node,
// key = (row << 16) | col strictly increasing, 5 d entries per instance.  The 4 d entries of N and -N do not depend on
// the instance: node (i,j)'s row holds, in column order, its down-in, right-in, right-out and down-out arc, and starts
// at entry  2 i (w-1) + w i + w max(i-1, 0) + j ([i>0] + [i<h-1]) + max(j-1, 0) + j.  The unit rows need the ranks of
// the 0-arcs and 1-arcs: a ballot prefix over the solution flags.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cave_hip.h"
#include "cone_common.h"
#include "solver_entry.h"
#include "wave_prims.h"

namespace cave {

struct SpGridParams {
  const float* costs;       // [N, d]
  const float* eval_costs;  // [N, d] or null
  int64_t N;
  int32_t h, w, d;
  uint32_t wave_lds;        // sp_grid_wave_lds_bytes(h, w)
  float* sol;               // [N, d] or null
  double* obj;              // [N] or null
  double* eval;             // [N] or null
  int32_t* status;          // [N] or null
  uint32_t* key;            // [N, 5 d] or null (with val)
  float* val;
};

static constexpr uint32_t kSpGridMaxLds = 160u * 1024u;

CAVE_HOSTDEV uint32_t sp_grid_r16(uint32_t x) { return (x + 15u) & ~15u; }
CAVE_HOSTDEV int64_t sp_grid_arcs(int64_t h, int64_t w) { return h * (w - 1) + (h - 1) * w; }
// LDS of one instance (= one wave), or 0 for a shape the kernel does not take
CAVE_HOSTDEV uint32_t sp_grid_wave_lds_bytes(int64_t h, int64_t w) {
  if (h < 1 || w < 1 || h * w < 2 || h > 65535 || w > 65535 || h * w > (int64_t)kSpGridMaxLds) return 0u;
  const int64_t d = sp_grid_arcs(h, w);
  const int64_t need = (int64_t)sp_grid_r16((uint32_t)(4 * d)) + (w > 64 ? (int64_t)sp_grid_r16((uint32_t)(8 * h)) : 0) +
                       (int64_t)sp_grid_r16((uint32_t)(h * w));
  return need <= (int64_t)kSpGridMaxLds ? (uint32_t)need : 0u;
}
// waves (= instances) per workgroup: 4 where the LDS allows
CAVE_HOSTDEV int sp_grid_waves(uint32_t wave_lds) {
  int wpb = 4;
  while (wpb > 1 && (uint32_t)wpb * wave_lds > kSpGridMaxLds) wpb >>= 1;
  return wpb;
}

// cave_hip_sp_grid_solve: its checks, its grid, the waves per workgroup and its parameter block (solver_entry.h)
inline int32_t sp_grid_plan(const float* costs, const float* eval_costs, int64_t N, int64_t h, int64_t w, float* sol, double* obj,
                            double* eval, int32_t* status, uint32_t* key, float* val, SpGridParams* P, int64_t* grid, int* waves,
                            char* msg) {
  const bool shape = h >= 1 && w >= 1 && h * w >= 2;
  const uint32_t wave_lds = shape ? sp_grid_wave_lds_bytes(h, w) : 0u;
  const int64_t d = shape ? sp_grid_arcs(h, w) : 0;
  const char* bad = nullptr;
  if (!shape) bad = "bad shape (need h, w >= 1 and h*w >= 2)";
  else if (wave_lds == 0u) bad = "the grid does not fit the LDS (cave_hip_sp_grid_lds_bytes)";
  else if ((key == nullptr) != (val == nullptr)) bad = "key and val go together";
  else if (key && (d > 65535 || 2 * h * w + d > 65535)) bad = "cone output needs d <= 65535 and 2*h*w + d <= 65535 (16-bit rows and columns)";
  const int32_t rc = solver_plan("sp_grid_solve", bad, eval && !eval_costs, N, nullptr, 0, 0, nullptr, nullptr, 0,
                                 costs ? nullptr : "costs is null", 1, grid, msg);
  if (rc != CAVE_OK || *grid == 0) return rc;
  *waves = sp_grid_waves(wave_lds);  // one wave per instance: the grid is the batch's workgroups, not the shared rule's
  *grid = (N + *waves - 1) / *waves;
  if (*grid >= (int64_t)1 << 31) {
    snprintf(msg, kSolverMsg, "sp_grid_solve: batch too large");
    return CAVE_E_INVALID;
  }
  P->costs = costs; P->eval_costs = eval_costs; P->N = N; P->h = (int32_t)h; P->w = (int32_t)w; P->d = (int32_t)d;
  P->wave_lds = wave_lds; P->sol = sol; P->obj = obj; P->eval = eval; P->status = status; P->key = key; P->val = val;
  return CAVE_OK;
}

#if defined(CAVE_GPU_CODE)
// one instance on one wave; lds: this wave's P.wave_lds bytes (16-byte aligned)
__device__ inline void sp_grid_instance(const SpGridParams& P, unsigned char* lds, int64_t b, int lane) {
  const int h = P.h, w = P.w, d = P.d;
  const int rs = 2 * w - 1;  // arcs per grid row
  float* cost = reinterpret_cast<float*>(lds);
  double* bnd = reinterpret_cast<double*>(lds + sp_grid_r16(4u * (uint32_t)d));
  uint8_t* pred = lds + sp_grid_r16(4u * (uint32_t)d) + (w > 64 ? sp_grid_r16(8u * (uint32_t)h) : 0u);
  const size_t row0 = (size_t)b * (size_t)d;

  // ---- stage the costs (a row starts wherever b d puts it: dword loads), reject non-finite ones
  bool badl = false;
  for (int k = lane; k < d; k += 64) {
    const float v = CAVE_NT_LOAD_F32(P.costs + row0 + k);
    cost[k] = v;
    badl = badl || !(fabsf(v) <= 3.4028234663852886e38f);
  }
  const bool bad = __ballot(badl) != 0ull;
  CAVE_WAVE_ORDER();

  // ---- anti-diagonal sweep, strip by strip
  double objv = __builtin_nan("");
  if (!bad) {
    const int nstrips = (w + 63) >> 6;
    double cur = 0.0;
    for (int s = 0; s < nstrips; ++s) {
      const int c0 = s << 6;
      const int nc = w - c0 < 64 ? w - c0 : 64;
      const int j = c0 + lane;
      const bool col = lane < nc;
      const bool hand = lane == nc - 1 && s + 1 < nstrips;
      const int steps = h + nc - 1;
      cur = 0.0;
      for (int t = 0; t < steps; ++t) {
        double left = dpp_f64<0x138, 0xf>(0.0, cur);  // wave_shr:1: dist(i, j-1), lane l-1's value of the step before
        const int i = t - lane;
        if (col && i >= 0 && i < h) {
          if (lane == 0 && s > 0) left = bnd[i];
          double v;
          uint32_t pr = 0u;
          if (j == 0) {
            v = i == 0 ? 0.0 : cur + (double)cost[(i - 1) * rs + (w - 1)];
          } else {
            const double r = left + (double)cost[i * rs + j - 1];
            if (i == 0) {
              v = r;
              pr = 1u;
            } else {
              const double dn = cur + (double)cost[(i - 1) * rs + (w - 1) + j];
              pr = r < dn ? 1u : 0u;  // strict: the down arc has the lower index and wins ties
              v = pr ? r : dn;
            }
          }
          cur = v;
          pred[i * w + j] = (uint8_t)pr;
          if (hand) bnd[i] = v;
        }
      }
      CAVE_WAVE_ORDER();
    }
    objv = readlane_f64(cur, (w - 1) & 63);
  }

  // ---- the cost array becomes the 0/1 solution; lane 0 walks back from the sink
  for (int k = lane; k < d; k += 64) cost[k] = 0.0f;
  CAVE_WAVE_ORDER();
  if (!bad && lane == 0) {
    int i = h - 1, j = w - 1;
    while ((i | j) != 0) {
      int k;
      if (pred[i * w + j]) {
        k = i * rs + j - 1;
        --j;
      } else {
        k = (i - 1) * rs + (w - 1) + j;
        --i;
      }
      cost[k] = 1.0f;
    }
  }
  CAVE_WAVE_ORDER();

  // ---- outputs
  if (P.sol)
    for (int k = lane; k < d; k += 64) P.sol[row0 + k] = cost[k];
  if (P.eval && P.eval_costs) {
    double acc = 0.0;
    for (int k = lane; k < d; k += 64) {
      const float e = CAVE_NT_LOAD_F32(P.eval_costs + row0 + k);
      if (cost[k] != 0.0f) acc += (double)e;
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) P.eval[b] = bad ? __builtin_nan("") : acc;
  }
  if (lane == 0) {
    if (P.obj) P.obj[b] = objv;
    if (P.status) P.status[b] = bad ? CAVE_ST_BAD_INPUT : CAVE_ST_OK;
  }
  if (P.key) {
    uint32_t* key = P.key + (size_t)b * 5u * (size_t)d;
    float* val = P.val + (size_t)b * 5u * (size_t)d;
    const uint32_t n = (uint32_t)(h * w);
    // N and -N: one node per lane
    for (int i = 0; i < h; ++i) {
      const int up = i > 0, dn = i < h - 1;
      const uint32_t rowbase = (uint32_t)(2 * i * (w - 1) + w * i + w * (i > 0 ? i - 1 : 0));
      for (int j = lane; j < w; j += 64) {
        uint32_t e = rowbase + (uint32_t)(j * (up + dn) + (j > 0 ? j - 1 : 0) + j);
        const uint32_t v = (uint32_t)(i * w + j);
        const uint32_t kp = v << 16, km = (n + v) << 16;
        if (up) {
          const uint32_t c = (uint32_t)((i - 1) * rs + (w - 1) + j);
          key[e] = kp | c; val[e] = 1.0f;
          key[2 * d + e] = km | c; val[2 * d + e] = -1.0f;
          ++e;
        }
        if (j > 0) {
          const uint32_t c = (uint32_t)(i * rs + j - 1);
          key[e] = kp | c; val[e] = 1.0f;
          key[2 * d + e] = km | c; val[2 * d + e] = -1.0f;
          ++e;
        }
        if (j < w - 1) {
          const uint32_t c = (uint32_t)(i * rs + j);
          key[e] = kp | c; val[e] = -1.0f;
          key[2 * d + e] = km | c; val[2 * d + e] = 1.0f;
          ++e;
        }
        if (dn) {
          const uint32_t c = (uint32_t)(i * rs + (w - 1) + j);
          key[e] = kp | c; val[e] = -1.0f;
          key[2 * d + e] = km | c; val[2 * d + e] = 1.0f;
        }
      }
    }
    // unit rows: -e_k for the arcs at 0 (ascending k), then +e_k for the arcs at 1
    const uint32_t n1 = bad ? 0u : (uint32_t)(h + w - 2), n0 = (uint32_t)d - n1;
    uint32_t ones = 0u;  // arcs at 1 below this chunk
    for (int k0 = 0; k0 < d; k0 += 64) {
      const int k = k0 + lane;
      const bool live = k < d;
      const bool one = live && cost[k] != 0.0f;
      const uint64_t mask = __ballot(one);
      const uint32_t r1 = ones + mbcnt64(mask);
      ones += (uint32_t)__popcll(mask);
      if (live) {
        const uint32_t r = one ? n0 + r1 : (uint32_t)k - r1;
        key[4 * d + r] = ((2u * n + r) << 16) | (uint32_t)k;
        val[4 * d + r] = one ? 1.0f : -1.0f;
      }
    }
  }
}
#endif  // CAVE_GPU_CODE

#if defined(__HIPCC__) && !defined(CAVE_SIMT_EMUL)
// k_sp_grid.hip: grid workgroups of `waves` waves, waves * P.wave_lds bytes of LDS
hipError_t launch_sp_grid(unsigned grid, int waves, hipStream_t stream, const SpGridParams& P);
#endif

}  // namespace cave
