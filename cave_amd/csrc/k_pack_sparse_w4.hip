// k_pack_sparse_w4.hip — one kernel shape and its launch function (see kernels.h)
#include "kernels.h"

namespace cave {
CAVE_DEFINE_LAUNCH(launch_pack_sparse_w4, SparsePackParams, cone_pack_sparse_kernel<Ctx4>, Ctx4::NT)
}  // namespace cave
