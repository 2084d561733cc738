// k_large_pack_sparse.hip — one kernel shape and its launch function (see kernels.h)
#include "kernels.h"

namespace cave {
CAVE_DEFINE_LAUNCH_LARGE(launch_pack_sparse_large, SparsePackParams, cone_pack_sparse_large_kernel<CtxL>, CtxL::NT)
}  // namespace cave
