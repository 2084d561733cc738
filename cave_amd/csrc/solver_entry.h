// solver_entry.h — the host side the exact-solver entry points share (cave_hip_sp_grid_solve, cave_hip_tsp_hk_solve,
// cave_hip_vrp_dp_solve, cave_hip_tsp_hk_wide_solve, cave_hip_vrp_dp_wide_solve): the argument checks, the grid rule and
// the default workspace.  Plain host code: the C ABI (cave_hip.hip) and the emulation drivers (tests/emul/simt_*.cpp, g++)
// call the same functions, so the CPU tier runs the checks the library runs.  Each entry's own plan function
// (sp_grid_plan, tsp_hk_plan, vrp_dp_plan, tsp_hk_wide_plan, vrp_dp_wide_plan, beside its layout functions) states what
// is its own -- the shape rule, its messages, its sizes -- and fills its parameter block.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "../../include/cave_hip.h"

namespace cave {

static constexpr int kSolverMsg = 256;  // bytes of a plan function's message buffer

static constexpr int64_t kSolverMaxGrid = (int64_t)1 << 20;  // workgroups of any entry at the most

// The checks, in the order every entry makes them; the entry's own findings arrive as messages (null: passed):
//   shape_bad | eval without eval_costs | N < 0 | args_bad | N == 0: nothing to do | the workspace (header bytes, then
//   slots of slot bytes; 8-byte aligned; at least one slot) | null_bad
// and the grid rule: one workgroup per slot the workspace holds (lds_grid for an entry without slots), at most N, at most 2^20.
// -> CAVE_OK and *grid (0: N == 0), or CAVE_E_INVALID and "<name>: <what>" in msg [kSolverMsg].
inline int32_t solver_plan(const char* name, const char* shape_bad, bool eval_without_costs, int64_t N, const char* args_bad,
                           int64_t header, int64_t slot, const char* ws_bad, const void* workspace, int64_t workspace_bytes,
                           const char* null_bad, int64_t lds_grid, int64_t* grid, char* msg) {
  const char* what = nullptr;
  *grid = 0;
  if (shape_bad) what = shape_bad;
  else if (eval_without_costs) what = "eval needs eval_costs";
  else if (N < 0) what = "bad N";
  else if (args_bad) what = args_bad;
  else if (N == 0) return CAVE_OK;
  else if (header + slot > 0 && (!workspace || workspace_bytes < header + slot || ((uintptr_t)workspace & 7u) != 0u)) what = ws_bad;
  else if (null_bad) what = null_bad;
  if (what) {
    snprintf(msg, kSolverMsg, "%s: %s", name, what);
    return CAVE_E_INVALID;
  }
  int64_t g = slot > 0 ? (workspace_bytes - header) / slot : lds_grid;
  if (g > N) g = N;
  if (g > kSolverMaxGrid) g = kSolverMaxGrid;
  *grid = g;
  return CAVE_OK;
}

// bytes of the default workspace: the header, then min(N, slots) slots
inline int64_t solver_workspace_bytes(int64_t header, int64_t slot, int64_t N, int64_t slots) {
  return header + slot * (N < slots ? N : slots);
}

}  // namespace cave
