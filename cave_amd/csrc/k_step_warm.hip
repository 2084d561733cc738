// k_step_warm.hip — the warm variant of the fused step kernel (multiplier cache, cone_step.h StepWarm): the same kernel
// as k_step.hip with the cache probe / write-back in its solve half, built in a translation unit of its own so that the
// cold kernel's code object does not change.  The wave priorities are those of k_step.hip (see the measurements there).
#ifndef CAVE_LITE_TAIL_PRIO_IT
#define CAVE_LITE_TAIL_PRIO_IT 5
#endif
#ifndef CAVE_STEP_PACK_PRIO
#define CAVE_STEP_PACK_PRIO 2
#endif
#include "kernels.h"

namespace cave {
using CtxStep = BlockCtx<2, true>;  // pack half: two waves per instance, 256-register budget
static constexpr auto cone_step_warm_kernel = cone_step_kernel<CtxStep, true>;
CAVE_DEFINE_LAUNCH(launch_step_warm, StepParamsWarm, cone_step_warm_kernel, CtxStep::NT)
}  // namespace cave
