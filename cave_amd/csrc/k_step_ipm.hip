// k_step_ipm.hip -- the interior-point variant of the fused step kernel (MODE_IPM: cone_core.h lite_solve_ipm): the kernel
// of k_step.hip with the truncated interior-point steps in its solve half, built in a translation unit of its own so
// that the cold and warm kernels' code objects do not change.  Pack waves at the priority of k_step.hip; no tail
// priority (CAVE_LITE_TAIL_PRIO_IT is keyed to Newton rounds: every instance here runs the same number of steps).
#ifndef CAVE_STEP_PACK_PRIO
#define CAVE_STEP_PACK_PRIO 2
#endif
#include "kernels.h"

namespace cave {
using CtxStep = BlockCtx<2, true>;  // pack half: two waves per instance, 256-register budget
static constexpr auto cone_step_ipm_kernel = cone_step_kernel<CtxStep, false, true>;
CAVE_DEFINE_LAUNCH(launch_step_ipm, StepParams, cone_step_ipm_kernel, CtxStep::NT)
}  // namespace cave
