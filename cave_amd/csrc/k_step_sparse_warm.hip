// k_step_sparse_warm.hip — the warm variant (multiplier cache, cone_step.h StepWarm) of the fused step kernel whose pack
// half reads the sparse wire format: k_step_sparse.hip with the cache probe / write-back of k_step_warm.hip in its solve
// half, in a translation unit of its own.  Wave priorities: k_step.hip's.  Measured as in k_step_sparse.hip, warm chain with
// fixed predictions (every instance hits, one iteration): pack waves at priority 2: 64.65 / 65.21 us per step, at 1:
// 64.89 / 64.69, at 0: 65.28 / 66.71 -- no difference beyond the run-to-run spread, the value stays.
#ifndef CAVE_LITE_TAIL_PRIO_IT
#define CAVE_LITE_TAIL_PRIO_IT 6
#endif
#ifndef CAVE_STEP_PACK_PRIO
#define CAVE_STEP_PACK_PRIO 2
#endif
#include "kernels.h"

namespace cave {
using CtxStep = BlockCtx<2, true>;  // pack half: two waves per instance, 256-register budget
static constexpr auto cone_step_sparse_warm_kernel = cone_step_sparse_kernel<CtxStep, true>;
CAVE_DEFINE_LAUNCH(launch_step_sparse_warm, StepSparseParamsWarm, cone_step_sparse_warm_kernel, CtxStep::NT)
}  // namespace cave
