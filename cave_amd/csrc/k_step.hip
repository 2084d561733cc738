// k_step.hip — one kernel shape and its launch function (see kernels.h)
// Wave priorities inside the fused launch (measured, one box per line, TSP-20 B = 1024 + 1024; tools/diag/build_variant.sh):
// pack waves above the solve waves from their start (without: 132 us per step -- the second round of pack workgroups is
// the tail), and a solve still iterating after a few Newton rounds -- by then the tail of the launch -- at priority 3
// from there on.  Before the solver's exchange loop and its one-round-trip prologue: never 121.4, from round 4 119.9, from
// round 5 118.9, from round 6 120.4.  With them (the solves are 10 % shorter, fewer of them are still running when the
// pack half ends): from round 3 123.5, 4 121.0, 5 117.9, 6 115.9 - 116.4, 7 117.0, never 116.6; pack waves at priority 2
// instead of 1: 116.0 with round 6.
// Re-tuned with the row scan of the pack half (ctx_block.h scan_rows: pack-only launch 63.5 us against 66.5, fused step
// 115.0 - 116.0 against the flat scan's 116.2 - 117.3 on the same box with the settings above); fused chain, us per step,
// two passes over twelve A/B builds:
//   pack priority    tail from round 4      round 5         round 6         never
//        0            127.8 / 127.9      127.8 / 127.7   127.9 / 127.8   127.8 / 128.0
//        1            114.8 / 114.7      114.0 / 114.4   115.7 / 115.7   115.9 / 116.2
//        2            115.3 / 115.1      114.2 / 114.3   115.7 / 115.8   116.1 / 116.0
// The pack waves still have to run above the solve waves (0: the second round of pack workgroups is the tail again); 1
// and 2 are the same within the noise, so 2 stays.  The shorter pack half ends earlier, and the solves that are still
// iterating gain from the raised priority one round sooner: the tail priority starts at round 5.
#ifndef CAVE_LITE_TAIL_PRIO_IT
#define CAVE_LITE_TAIL_PRIO_IT 5
#endif
#ifndef CAVE_STEP_PACK_PRIO
#define CAVE_STEP_PACK_PRIO 2
#endif
#include "kernels.h"

namespace cave {
using CtxStep = BlockCtx<2, true>;  // pack half: two waves per instance, 256-register budget
CAVE_DEFINE_LAUNCH(launch_step, StepParams, cone_step_kernel<CtxStep>, CtxStep::NT)
// (the warm variant, multiplier cache: k_step_warm.hip -- a code object of its own, the cold one stays as it was)
CAVE_DEFINE_LAUNCH(launch_lite_from_packed, LiteFromPackedParams, lite_from_packed_kernel<Ctx2>, Ctx2::NT)
}  // namespace cave
