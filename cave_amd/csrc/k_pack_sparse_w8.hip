// k_pack_sparse_w8.hip — one kernel shape and its launch function (see kernels.h)
#include "kernels.h"

namespace cave {
CAVE_DEFINE_LAUNCH(launch_pack_sparse_w8, SparsePackParams, cone_pack_sparse_kernel<CtxW>, CtxW::NT)
}  // namespace cave
