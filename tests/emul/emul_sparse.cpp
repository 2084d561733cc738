// emul_sparse.cpp — serial gcc build of the sparse pack pass (TEST INFRASTRUCTURE ONLY).
// Exports cave_emul_*_sparse with the signatures of include/cave_hip.h minus the stream (and, on the large path, minus
// the workspace: a heap slice); all pointers are HOST pointers.  Beside emul_abi.cpp, which holds the dense entry
// points; never loaded by cave_amd.
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "ctx_serial.h"
#include "../../cave_amd/csrc/cone_core.h"
#include "../../cave_amd/csrc/cone_instance.h"
#include "../../cave_amd/csrc/cone_entry.h"

using namespace cave;

static bool sparse_ok(const cave_sparse_cones* s) {
  return s && s->B >= 0 && s->m_max >= 0 && s->m_max <= 65535 && s->d > 0 && s->d <= 65535 &&
         (s->B == 0 || (s->ent_off && s->key && s->val));
}

extern "C" {

int32_t cave_emul_pack_count_sparse(const cave_sparse_cones* cones, int32_t nnz_cap, int32_t lds_bytes, int32_t* n_rows,
                                    int32_t* n_nnz, int32_t* status) {
  if (!sparse_ok(cones) || !resolve_limits(cones->m_max, cones->d, nnz_cap, lds_bytes)) return CAVE_E_INVALID;
  const SparsePackParams P = sparse_pack_fill(cones, nnz_cap, lds_bytes, n_rows, n_nnz, status, nullptr, 0);
  std::vector<unsigned char> smem((size_t)lds_bytes);  // exact size: ASan catches arena overruns
  SerialCtx c;
  for (int64_t b = 0; b < P.B; ++b) run_pack_sparse_instance(c, smem.data(), P, b);
  return CAVE_OK;
}

int32_t cave_emul_pack_fill_sparse(const cave_sparse_cones* cones, int32_t nnz_cap, int32_t lds_bytes,
                                   const cave_cone_store* store, int64_t slot0, int32_t* status) {
  if (!sparse_ok(cones) || !resolve_limits(cones->m_max, cones->d, nnz_cap, lds_bytes)) return CAVE_E_INVALID;
  if (!store || !store_slot_ok(store, cones->d, slot0, cones->B)) return CAVE_E_INVALID;
  const SparsePackParams P = sparse_pack_fill(cones, nnz_cap, lds_bytes, nullptr, nullptr, status, store, slot0);
  std::vector<unsigned char> smem((size_t)lds_bytes);
  SerialCtx c;
  for (int64_t b = 0; b < P.B; ++b) run_pack_sparse_instance(c, smem.data(), P, b);
  return CAVE_OK;
}

int32_t cave_emul_pack_large_sparse(const cave_sparse_cones* cones, int64_t nnz_cap, int64_t slice_bytes, int32_t* n_rows,
                                    int32_t* n_nnz, const cave_cone_store* store, int64_t slot0, int32_t* status) {
  if (!sparse_ok(cones) || nnz_cap <= 0 || slice_bytes <= 0 || slice_bytes >= ((int64_t)1 << 32)) return CAVE_E_INVALID;
  if (store && !store_slot_ok(store, cones->d, slot0, cones->B)) return CAVE_E_INVALID;
  const SparsePackParams P = sparse_pack_fill(cones, nnz_cap, 1024, n_rows, n_nnz, status, store, slot0);
  std::vector<unsigned char> smem(1024), ws((size_t)slice_bytes);
  SerialCtx c;
  for (int64_t b = 0; b < P.B; ++b) run_pack_sparse_instance<SerialCtx, true>(c, smem.data(), P, b, ws.data(), (uint32_t)slice_bytes);
  return CAVE_OK;
}

}  // extern "C"
