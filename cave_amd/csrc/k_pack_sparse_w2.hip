// k_pack_sparse_w2.hip — one kernel shape and its launch function (see kernels.h)
#include "kernels.h"

namespace cave {
CAVE_DEFINE_LAUNCH(launch_pack_sparse_w2, SparsePackParams, cone_pack_sparse_kernel<Ctx2>, Ctx2::NT)
}  // namespace cave
