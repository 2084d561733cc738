// k_step_sparse_ipm.hip -- the interior-point variant (MODE_IPM: cone_core.h lite_solve_ipm) of the fused step kernel
// whose pack half reads the sparse wire format: k_step_sparse.hip with the solve half of k_step_ipm.hip, in a
// translation unit of its own.  Pack waves at the priority of k_step_sparse.hip (0: its short pack half, measured there);
// no tail priority (see k_step_ipm.hip).
#ifndef CAVE_STEP_PACK_PRIO
#define CAVE_STEP_PACK_PRIO 0
#endif
#include "kernels.h"

namespace cave {
using CtxStep = BlockCtx<2, true>;  // pack half: two waves per instance, 256-register budget
static constexpr auto cone_step_sparse_ipm_kernel = cone_step_sparse_kernel<CtxStep, false, true>;
CAVE_DEFINE_LAUNCH(launch_step_sparse_ipm, StepSparseParams, cone_step_sparse_ipm_kernel, CtxStep::NT)
}  // namespace cave
