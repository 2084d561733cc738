// k_step_sparse.hip — the fused step kernel whose pack half reads the sparse wire format (kernels.h
// cone_step_sparse_kernel), cold variant.  A translation unit of its own: the code objects of k_step.hip / k_step_warm.hip
// stay as they were.
// Wave priorities (measured, one box, TSP-20 B = 1024 + 1024, tools/diag/sparse_step.py on builds of
// tools/diag/build_variant.sh, the three builds alternating twice, us per step of the sparse fused chain, spread of three
// repetitions <= 0.23): pack waves at priority 2 (k_step.hip's value, tuned for its 66 us dense pack half) 119.57 / 119.97,
// at 1: 119.63 / 119.78, at 0: 115.75 / 115.37.  This pack half is short (31.9 us alone): it ends long before the solves
// do however it is scheduled, and at the solve waves' own priority it does not hold them up.  The solve tail's priority
// round is k_step.hip's (not varied here).
#ifndef CAVE_LITE_TAIL_PRIO_IT
#define CAVE_LITE_TAIL_PRIO_IT 6
#endif
#ifndef CAVE_STEP_PACK_PRIO
#define CAVE_STEP_PACK_PRIO 0
#endif
#include "kernels.h"

namespace cave {
using CtxStep = BlockCtx<2, true>;  // pack half: two waves per instance, 256-register budget
CAVE_DEFINE_LAUNCH(launch_step_sparse, StepSparseParams, cone_step_sparse_kernel<CtxStep>, CtxStep::NT)
}  // namespace cave
