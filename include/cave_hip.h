/* cave_hip.h — C ABI of the MI355X (gfx950) cone-projection backend for CaVE.
 *
 * This is the drop-in boundary: plain pointers and sizes, no
 * torch types.  Every pointer is a DEVICE pointer owned by the caller; inputs
 * are never written; all work is enqueued asynchronously on `stream`
 * (a hipStream_t passed as void*, NULL = default stream); nothing here
 * synchronises with the host.  Functions return CAVE_OK or a negative
 * CAVE_E_* code and never throw; per-instance solver outcomes are data
 * (`status[B]`, codes CAVE_ST_*), mirroring how the reference reports
 * Clarabel failures per instance (src/cave.py:293-294) while bad configuration
 * is rejected up front (src/cave.py:111-117,183-190).
 *
 * Reference interfaces replaced (paths relative to /root/reference):
 *   cave_hip_cone_dense  mode PROJECT   _batch_project(..., solver='nnls') + _project_nnls
 *                                       src/cave.py:231-264, 298-309
 *                        mode EXACT     abstractConeAlignedCosine.forward + exact _get_projection
 *                                       src/cave.py:55-73, 121-129 (and its autograd backward)
 *                        mode INNER     innerConeAlignedCosine QP branch, nnls push-inside
 *                                       src/cave.py:206-219
 *                        mode HEURISTIC innerConeAlignedCosine heuristic branch  src/cave.py:201-204
 *                        mode AVG       _average_ctrs                            src/cave.py:222-228
 *   cave_hip_pack_*  / cave_hip_cone_packed
 *                                       optDatasetConstrs.ctrs storage + collate_fn padding
 *                                       src/dataset.py:72, 133-144 (device-resident replacement)
 *   cave_hip_cone_step                  one training step's worth of both on the dense wire format, in ONE launch:
 *                                       the forward / backward of the CURRENT batch (src/cave.py:55-73) from a
 *                                       transient store + the collate-side work on the NEXT batch the DataLoader
 *                                       has already produced (src/dataset.py:133-144)
 *   cave_hip_*_large                    the same three operators for cones whose reduced system does
 *                                       not fit registers / LDS (TSP-100, 30x30 shortest path: the
 *                                       reference runs them through the same _project_nnls,
 *                                       src/cave.py:298-309); caller-owned global workspace
 */
#ifndef CAVE_HIP_H
#define CAVE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAVE_HIP_ABI_VERSION 10

/* return codes */
#define CAVE_OK 0
#define CAVE_E_INVALID (-1)  /* bad argument (null pointer, size out of range) */
#define CAVE_E_LAUNCH (-2)   /* HIP launch / attribute error, see cave_hip_last_error() */
#define CAVE_E_NO_DEVICE (-3)

/* per-instance status */
#define CAVE_ST_OK 0
#define CAVE_ST_NOT_CONVERGED 1 /* iteration cap reached (SciPy raises RuntimeError, src/cave.py:307) */
#define CAVE_ST_TOO_LARGE 2     /* cone did not fit this launch's LDS arena; retry with larger limits */
#define CAVE_ST_BAD_INPUT 3     /* non-finite values; sparse wire format: an entry that breaks its contract */
#define CAVE_ST_INFEASIBLE 4    /* cave_hip_vrp_dp[_wide]_solve: the instance has no feasible solution */

/* modes */
#define CAVE_MODE_PROJECT 0
#define CAVE_MODE_EXACT 1
#define CAVE_MODE_INNER 2
#define CAVE_MODE_HEURISTIC 3
#define CAVE_MODE_AVG 4
/* CaVE+ with a truncated interior-point projection (src/cave.py:213-214, 267-295: the reference runs Clarabel
 * with max_iter = 3 and uses the strictly interior iterate, normalised, as the target).  Here: `max_iter`
 * steps (<= 0: 3) of a primal path-following method on  min 1/2 ||y - A^T lam||^2 - tau * sum log lam_i  with
 * tau shrinking every step; the multipliers of the signed-unit rows are eliminated in closed form, which turns
 * their clip into its Chen-Harker-Kanzow-Smale smoothing.  Every multiplier of the iterate is > 0; proj / rnorm
 * are those of the iterate and tend to the exact projection as max_iter grows.  An emulation: Clarabel's own
 * iterates are not reproduced (no Clarabel in the image: parity unpinned).  Since v8 also on the large-cone path
 * (cave_hip_cone_dense_large / cave_hip_cone_packed_large): one band or dense LDL^T per interior-point step. */
#define CAVE_MODE_INNER_IPM 5

int32_t cave_hip_version(void);
/* thread-local, valid until the next failing call on this thread */
const char* cave_hip_last_error(void);
/* number of HIP devices visible (0 if none); does not create a context on failure */
int32_t cave_hip_device_count(void);

/* Launch limits.  nnz_cap: per-instance capacity for non-zero entries of the
 * dense block; lds_bytes: dynamic LDS per workgroup (<= 160 KiB).  Pass 0 for
 * either to let the library choose (cave_hip_default_limits reports the
 * choice so a caller can grow it after CAVE_ST_TOO_LARGE).
 * waves: wavefronts cooperating on one instance (workgroup = `waves` x 64 threads).
 *   0 = library default (2);  1 or 2: reduced systems up to 64 rows;  4: up to 32 rows;  8: four waves with
 *   the full register budget (up to 64 rows; for launches whose LDS arena leaves one workgroup per CU) (an instance with
 *   more reports CAVE_ST_TOO_LARGE: the host layer tries 4 first, then 2, and remembers per shape).
 * More waves shorten the per-instance critical path (useful while B is about the number of SIMDs,
 * 1024 on MI355X: TSP-20, B = 1024 takes 187 / 212 / 236 us with 4 / 2 / 1 waves); one wave per
 * instance maximises instances in flight (best throughput beyond ~1300 instances).
 * One workgroup per instance: B < 2^31. */
int32_t cave_hip_default_limits(int64_t m_max, int64_t d, int32_t* nnz_cap, int32_t* lds_bytes);

/* Fused per-instance operator on the reference's dense wire format.
 *   ctrs  [B, m_max, d] float32 row-major, zero-padded rows  (src/dataset.py:143)
 *   pred  [B, d]        float32; the kernel works on y = sign * pred
 *   mode  CAVE_MODE_*;  sign  -1 (EPO.MINIMIZE) / +1 (EPO.MAXIMIZE); for PROJECT pass +1
 *   inner_ratio  weight of the average normal (INNER, HEURISTIC)
 *   max_iter     Newton iteration cap (<=0: default 100); CAVE_MODE_INNER_IPM: interior-point steps (<=0: 3)
 * Outputs (any may be NULL):
 *   proj   [B, d]  projection of y onto cone{lam @ ctrs_b : lam >= 0}
 *   rnorm  [B]     ||y - proj||_2 (un-squared, nnls convention)
 *   target [B, d]  the constant target of the cosine loss (unit / pushed / heuristic; AVG: the average)
 *   loss   [B]     1 - cos(y, target)
 *   grad   [B, d]  d loss_b / d pred_b
 *   status [B]     CAVE_ST_*
 *   iters  [B]     Newton iterations used
 */
int32_t cave_hip_cone_dense(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d,
                            int32_t mode, float sign, float inner_ratio, int32_t max_iter,
                            int32_t nnz_cap, int32_t lds_bytes, int32_t waves,
                            float* proj, float* rnorm, float* target, float* loss, float* grad,
                            int32_t* status, int32_t* iters, void* stream);

/* ---- device-resident packed cone store (replaces per-step dense padding) ---- */

/* Pass 1: per instance, count reduced rows and their non-zeros.
 *   n_rows [B], n_nnz [B], status [B] */
int32_t cave_hip_pack_count(const float* ctrs, int64_t B, int64_t m_max, int64_t d,
                            int32_t nnz_cap, int32_t lds_bytes, int32_t waves,
                            int32_t* n_rows, int32_t* n_nnz, int32_t* status, void* stream);

/* Packed store: structure-of-arrays, all device pointers, filled by cave_hip_pack_fill.
 *   row_off [n+1], nnz_off [n+1]  exclusive prefix sums of the pass-1 counts (int64)
 *   n_valid [n]        rows kept by the projection (0 = empty cone)
 *   flags   [n]        bit0: every reduced-row entry is +-1 (kernels then keep signs in the indices);
 *                      bit1 (set by the HOST on stores of the large-cone path, which reads them in place): ccol / cvar of
 *                      this instance already carry the sign in bit 15 (d, rows < 32768), cval / cvalc are not read
 *   usign   [n*d]      bit0: a +e_k row exists, bit1: a -e_k row exists
 *   avg     [n*d]      _average_ctrs of the instance (static, precomputed)
 *   vkind   [R]        1 = free multiplier (a +a/-a pair), 0 = non-negative     R = row_off[n]
 *   rlo,rhi [R]        CSR extent of each reduced row, relative to nnz_off[i]
 *   ccol, cval [Z]     CSR entries                                              Z = nnz_off[n]
 *   cptr    [n*(d+1)]  CSC column pointers, relative to nnz_off[i]
 *   cvar, cvalc [Z]    CSC entries (reduced-row index, value)
 */
typedef struct cave_cone_store {
  int64_t n;
  int32_t d;
  int32_t reserved;
  const int64_t* row_off;
  const int64_t* nnz_off;
  int32_t* n_valid;
  uint8_t* flags;
  uint8_t* usign;
  float* avg;
  uint8_t* vkind;
  uint32_t* rlo;
  uint32_t* rhi;
  uint16_t* ccol;
  float* cval;
  uint32_t* cptr;
  uint16_t* cvar;
  float* cvalc;
  /* Slot mode (both NULL in an exact-fit store).  When set, row_off / nnz_off only give each slot its
   * CAPACITY window (e.g. slot * max_rows, slot * max_nnz) and the actual sizes are n_rows[slot] / n_nnz[slot]:
   * cave_hip_pack_fill then needs no count pass (an instance that does not fit its window reports
   * CAVE_ST_TOO_LARGE and sets n_rows[slot] = -1, which cave_hip_cone_packed reports as CAVE_ST_TOO_LARGE too), which is how the dense operator runs small cones as
   * "pack into a transient slot store, then cave_hip_cone_packed" in one pass over the dense bytes. */
  int32_t* n_rows;
  int32_t* n_nnz;
  /* Warm start (both NULL: off).  warm_theta [R] float32, aligned with the reduced rows, holds the multipliers the
   * last converged projection of each instance ended with; warm_state [n] is 1 where that is valid (the caller
   * zeroes it to reset).  cave_hip_cone_packed(_large) then starts the Newton iteration there and refreshes both.
   * Cones are static per instance and predictions drift slowly during training (src/dataset.py:72); the
   * projection is unique, so results are the same as from a cold start (to the solver's tolerance). */
  float* warm_theta;
  uint8_t* warm_state;
  /* Red-black cache (v10; NULL: off).  rb_cache [n * rb_stride] bytes, ZEROED by the caller, rb_stride from
   * cave_hip_packed_large_rb_bytes(max_rows).  cave_hip_cone_packed_large keeps there, per instance, what its red-black
   * reduction of the band systems (grid shortest-path cones) derives from the STATIC cone alone -- the independent set
   * of reduced rows, the recipes of the Schur complement -- so that only the first projection of an instance builds
   * it (cones are static per instance, src/dataset.py:72).  Results do not depend on it. */
  uint8_t* rb_cache;
  int64_t rb_stride;
} cave_cone_store;

/* Pass 2: fill the store for instances [0, B) of `ctrs` at store slots [slot0, slot0+B). */
int32_t cave_hip_pack_fill(const float* ctrs, int64_t B, int64_t m_max, int64_t d,
                           int32_t nnz_cap, int32_t lds_bytes, int32_t waves,
                           const cave_cone_store* store, int64_t slot0, int32_t* status, void* stream);

/* Same operator as cave_hip_cone_dense, reading cones from the store:
 *   ids [B] int64 store slots (the collate_fn replacement hands these out). */
int32_t cave_hip_cone_packed(const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B,
                             int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t lds_bytes,
                             int32_t waves, float* proj, float* rnorm, float* target, float* loss, float* grad,
                             int32_t* status, int32_t* iters, void* stream);

/* LDS bytes cave_hip_cone_packed needs for the largest instance of a store
 * (max_rows / max_nnz over instances, from the pass-1 counts).  all_pm1 != 0: every instance has
 * flags bit0 set, so no value arrays are staged (smaller arena -> more workgroups per CU).  all_pm1 == 1 also
 * reserves room for the index structures of the one-wave solver for small cones (d <= 256, <= 32 rows), which
 * launches of up to 2048 instances use; all_pm1 == 2: +-1 cones without that room (large batches: more
 * workgroups per CU matter more there); all_pm1 == 3 (v9): the "diet" layout of +-1 cones with more than 32 reduced
 * rows (TSP-50: 107 KB -> 76 KB, two workgroups per compute unit instead of one): H as a packed lower triangle, the
 * CSC entries and the average normal read in place from the store.  It is taken, per instance, by
 * cave_hip_cone_packed(waves = 8) when the instance's ordinary arena exceeds the lds_bytes of the launch and the
 * store carries the signs in its indices (flags bit 1). */
int32_t cave_hip_packed_lds_bytes(int64_t d, int32_t max_rows, int32_t max_nnz, int32_t all_pm1);

/* ------------------------------------------------------------------ large-cone path
 * Same operators, same per-instance semantics and outputs, for cones beyond the fast path's limits
 * (more than 64 reduced rows, or more non-zeros than 160 KiB of LDS holds).  Persistent workgroups
 * (4 waves; cave_hip_cone_packed_large takes 2-wave workgroups when the batch needs more than two
 * workgroups per CU and four fit the LDS); each works in its own slice of a caller-owned, 16-byte aligned device `workspace` of
 * n_slots * slice_bytes bytes (n_slots = number of workgroups launched, at most B are used; a few per
 * CU is enough).  The Newton systems are kept as symmetric bands (band = reduced rows x (half
 * bandwidth + 1) entries) and solved by an LDL^T band elimination (narrow bands -- half bandwidth
 * 4 .. 34, grid shortest-path cones -- four pivots per step on one or two waves).  An instance that does not fit its
 * slice reports CAVE_ST_TOO_LARGE: retry with a larger slice.
 *   nnz_cap       non-zeros kept per instance
 *   band_entries  expected rows x (bandwidth + 1) of the reduced system (sizing hint)
 *   lds_bytes     LDS per workgroup used for the small hot arrays, 0 = 64 KiB */
int64_t cave_hip_large_slice_bytes(int64_t m_max, int64_t d, int64_t nnz_cap, int64_t band_entries);
int64_t cave_hip_packed_large_slice_bytes(int64_t d, int64_t max_rows, int64_t band_entries);
/* LDS per workgroup that keeps the hot arrays of the band solver (ring window, staging, two row vectors, flags)
 * on chip for reduced systems of up to max_rows rows and half bandwidth max_bw (v7).  Narrow bands
 * (max_bw <= 34) are eliminated by ONE wave per instance; the figure returned for them is the exact need, so that
 * four workgroups share a CU (the 2- and 1-wave forms of cave_hip_cone_packed_large are chosen from it). */
int32_t cave_hip_packed_large_lds_bytes(int32_t max_rows, int32_t max_bw);
/* Bytes per instance of cave_cone_store.rb_cache for reduced systems of up to max_rows rows (v10); 0: such cones never
 * take the red-black reduction. */
int64_t cave_hip_packed_large_rb_bytes(int64_t max_rows);

int32_t cave_hip_cone_dense_large(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d,
                                  int32_t mode, float sign, float inner_ratio, int32_t max_iter, int64_t nnz_cap,
                                  int32_t lds_bytes, void* workspace, int64_t slice_bytes, int32_t n_slots, float* proj,
                                  float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                                  int32_t* iters, void* stream);

/* store == NULL: count pass (n_rows / n_nnz per instance, as cave_hip_pack_count);
 * store != NULL: fill pass into slots [slot0, slot0 + B) (as cave_hip_pack_fill; n_rows / n_nnz unused). */
int32_t cave_hip_pack_large(const float* ctrs, int64_t B, int64_t m_max, int64_t d, int64_t nnz_cap, void* workspace,
                            int64_t slice_bytes, int32_t n_slots, int32_t* n_rows, int32_t* n_nnz,
                            const cave_cone_store* store, int64_t slot0, int32_t* status, void* stream);

/* reads the cones in place from the store; the workspace only holds the solver's work arrays.
 *   waves (v8)  wavefronts per workgroup: 1, 2 or 4; 0 = library default (4, or 2 when the batch needs more than
 *               two workgroups per compute unit and four workgroups fit the LDS).  The library reads no
 *               environment variable and keeps no state between calls. */
int32_t cave_hip_cone_packed_large(const cave_cone_store* store, const int64_t* ids, const float* pred, int64_t B,
                                   int32_t mode, float sign, float inner_ratio, int32_t max_iter, int32_t lds_bytes,
                                   int32_t waves, void* workspace, int64_t slice_bytes, int32_t n_slots, float* proj,
                                   float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                                   int32_t* iters, void* stream);

/* ------------------------------------------------------------------ fused step (v9)
 * Small +-1 cones on the dense wire format (TSP-20, small grids: d <= 256, <= 32 reduced rows in the order
 * [free | <= 8 bound rows], <= 8 entries per column, <= 1536 non-zeros -- what the one-wave solver takes).
 * One more condition ties the bound rows to the rows: the active-set loop needs p nI + nI (nI | 1) + 4 nI + 1 doubles of
 * scratch for p reduced rows of which nI have bounds; they come from a d-vector that is idle during the solve when that
 * is big enough, else from what the p-sized arrays leave of their 32-row figures in the arena of a solve-only launch.
 * A cone for which neither holds is refused like one beyond the limits above (slot state -1, pack status
 * CAVE_ST_TOO_LARGE), so a slot whose state is 1 is solved by every launch form.  At d = 256 this admits 32 rows with
 * up to 5 bound rows, 31 with 6, 28 with 7, 27 with 8 (TSP-20: 20 + <= 5).
 *
 * A step on the dense format is  (a) stream the dense block + build the reduced cone  ->  (b) Newton solve + loss +
 * gradient.  (a) depends on the cones only, and the training loop has the cones of batch i+1 before it has the
 * prediction of batch i+1 (the DataLoader collates ahead), so cave_hip_cone_step runs (b) of the CURRENT batch and (a)
 * of the NEXT batch in one grid: B one-wave solve instances first in the block order, then B_next four-wave pack
 * workgroups, which fill what the solve waves leave of each compute unit.  One stream, no events.
 *
 * cave_lite_store: transient per-batch store in the layout the one-wave solver reads (caller-owned device arrays):
 *   hdr    [n*8]    int32: state (1 = holds a cone, -1 = the cone does not qualify, 0 = never packed), reduced rows p,
 *                   non-zeros, free rows nF (rows [0, nF) have free multipliers), rows kept by the projection,
 *                   longest column, CSR entries per lane (8 / 16 / 24), spare
 *   usign  [n*d]    bit0: a +e_k row exists, bit1: a -e_k row exists
 *   avg    [n*d]    _average_ctrs of the instance
 *   rowptr [n*33]   CSR row pointers of the reduced rows
 *   ell    [n*4*d]  uint32: the column of coordinate k as eight 16-bit entries (reduced row | sign << 15; unused: row 32)
 *   csr16  [n*768]  uint32: CSR entries as 16-bit words (column | sign << 15 | row-end marks), lane-major groups of 8
 *   rl     [n*32]   lane holding the last entry of reduced row i
 * (ell / csr16 need 16-byte aligned bases.) */
typedef struct cave_lite_store {
  int64_t n;
  int32_t d;
  int32_t reserved;
  int32_t* hdr;
  uint8_t* usign;
  float* avg;
  uint32_t* rowptr;
  uint32_t* ell;
  uint32_t* csr16;
  uint8_t* rl;
} cave_lite_store;

/* dynamic LDS per workgroup of cave_hip_cone_step for dense batches of shape (m_max, d); <= 0: the shape does not
 * qualify: d > 256, or SIX workgroups of that size (four solve blocks + two pack blocks) would not fit the 160 KiB of a
 * compute unit -- use the general operators.  m_max = 0 asks for a launch without a pack half (the lite slots of a
 * device-resident store), which needs four.  At d = 256 the solve half alone takes 28672 bytes, so from d = 229 on
 * there is no fused launch whatever m_max: such cones reach the one-wave solver through cave_hip_lite_from_packed and
 * the solve-only launch. */
int32_t cave_hip_step_lds_bytes(int64_t m_max, int64_t d);

/* Solve half: B instances of `solve` -- slot ids[b], or slot b when ids is NULL (a transient per-batch store packed
 *   by an earlier call) -- with predictions pred [B, d]; outputs as cave_hip_cone_dense (modes PROJECT / EXACT / INNER /
 *   HEURISTIC / AVG; an instance whose slot holds no cone reports CAVE_ST_TOO_LARGE, a slot out of range
 *   CAVE_ST_BAD_INPUT).  B = 0 (solve may be NULL): pack only.
 * Pack half: instances [0, B_next) of next_ctrs [B_next, m_max, d] into slots [0, B_next) of `next` (a different
 *   store than `solve`); pack_status [B_next] or NULL.  B_next = 0 (next_ctrs / next may be NULL): solve only.
 * cu_tickets: 4096 uint32 of device memory, zeroed once by the caller, shared by the launches of one device (per
 *   compute-unit counters that spread the solve waves over the SIMDs; the library keeps no state of its own). */
#define CAVE_STEP_ZERO_FAILED 1 /* flags: an instance whose status is not CAVE_ST_OK gets loss 0 and a zero gradient (a
                                * training loop that examines `status` a step later must not feed NaN to its optimizer) */
int32_t cave_hip_cone_step(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode, float sign,
                           float inner_ratio, int32_t max_iter, int32_t flags, float* proj, float* rnorm, float* target, float* loss,
                           float* grad, int32_t* status, int32_t* iters, const float* next_ctrs, int64_t B_next,
                           int64_t m_max, int64_t d, const cave_lite_store* next, int32_t* pack_status,
                           uint32_t* cu_tickets, void* stream);

/* ------------------------------------------------------------------ warm start of the fused step (additive to v10)
 * Cones are static per instance and predictions drift slowly during training, so the multipliers a solve of a cone
 * ended with are a good starting point for the next solve of the same cone (TSP-20: ~2.6 instead of ~5.2 Newton
 * iterations).  cave_warm_cache: caller-owned device memory, a set-associative table of min(4, n_entries) ways per
 * set; entry e holds key[e] and the 32 multipliers theta[32 e .. 32 e + 31].  Keys: the caller's keys[b] (>= 0, e.g. the
 * store slot of a device-resident store), or, when keys is NULL, the content of the cone (a fingerprint of its row
 * pointers, csr16 words, sign bytes and count of rows kept -- the same cone gives the same value at any batch position
 * and any m_max -- with p, nF and the non-zero count; formed by the solve half, hdr[7] stays spare): dense batches
 * need no ids and may be shuffled.  The two key spaces carry different tag
 * bits.  Entries are read and written with plain loads and stores: cached multipliers are only a starting point, so a
 * stale or torn entry costs iterations, never correctness (the projection is unique). */
typedef struct cave_warm_cache {
  int64_t n_entries; /* power of two */
  uint64_t* key;     /* [n_entries], 0 = empty; zeroed by the caller (zeroing it resets the cache) */
  float* theta;      /* [n_entries * 32], 16-byte aligned */
} cave_warm_cache;

/* cave_hip_cone_step with a multiplier cache; the parameters of cave_hip_cone_step in the same order, with
 *   warm      the cache, or NULL: exactly cave_hip_cone_step
 *   keys      [B] cache keys (>= 0; a negative key: no cache for that instance), or NULL: keys from the cone content
 *   warm_hit  [B] or NULL: 1 where the instance started from cached multipliers, else 0
 * inserted before cu_tickets.  Modes PROJECT / EXACT / INNER look up and write back (after CAVE_ST_OK: the final
 * multipliers; after any other status the entry the instance matched is cleared); HEURISTIC / AVG do not touch the
 * cache.  An instance that does not hit computes exactly what cave_hip_cone_step computes (outputs, status, iters).
 * A cache whose n_entries is not a power of two, with a NULL array or a theta that is not 16-byte aligned:
 * CAVE_E_INVALID. */
int32_t cave_hip_cone_step_warm(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode,
                                float sign, float inner_ratio, int32_t max_iter, int32_t flags, float* proj, float* rnorm,
                                float* target, float* loss, float* grad, int32_t* status, int32_t* iters,
                                const float* next_ctrs, int64_t B_next, int64_t m_max, int64_t d, const cave_lite_store* next,
                                int32_t* pack_status, const cave_warm_cache* warm, const int64_t* keys, uint8_t* warm_hit,
                                uint32_t* cu_tickets, void* stream);

/* ------------------------------------------------------------------ sparse wire format (additive to v10)
 * The dense wire format is almost all zeros (TSP-100: 33 447 non-zeros in a 102 MB block).  A batch of cones in
 * coordinate form, device pointers, caller-owned, read-only:
 *   ent_off [B+1]  entry offsets of the instances, ent_off[0] = 0, non-decreasing
 *   key     [Z]    (row << 16) | col, STRICTLY increasing within an instance (= row-major order)
 *   val     [Z]    non-zero, finite
 * (key and val 4-byte aligned; 16-byte loads are used when the two bases are congruent modulo 16.)
 * Checked on the device, per instance, in the pass that reads the entries: a key that is not greater than its
 * predecessor, a row >= m_max, a column >= d, a zero or a non-finite value give CAVE_ST_BAD_INPUT for that instance
 * (nothing is read or written out of range); more than nnz_cap entries give CAVE_ST_TOO_LARGE.  An instance without
 * entries is the empty cone.  m_max, d <= 65535; the dense route's m_max * d < 2^32 does not apply. */
typedef struct cave_sparse_cones {
  int64_t B;
  int32_t m_max, d;
  const int64_t* ent_off;
  const uint32_t* key;
  const float* val;
} cave_sparse_cones;

/* cave_hip_pack_count / cave_hip_pack_fill / cave_hip_pack_large from the sparse wire format: same arguments with
 * `ctrs, B, m_max, d` replaced by the batch, same launch limits, same stores (exact-fit and slot mode), and -- the
 * reduced cone being built by the same code from the same entries -- the same bits in the store as the dense route
 * writes for the densified batch.  waves: 0 (= 2), 2, 4 or 8; there is no one-wave sparse pack shape (waves = 1:
 * CAVE_E_INVALID). */
int32_t cave_hip_pack_count_sparse(const cave_sparse_cones* cones, int32_t nnz_cap, int32_t lds_bytes, int32_t waves,
                                   int32_t* n_rows, int32_t* n_nnz, int32_t* status, void* stream);
int32_t cave_hip_pack_fill_sparse(const cave_sparse_cones* cones, int32_t nnz_cap, int32_t lds_bytes, int32_t waves,
                                  const cave_cone_store* store, int64_t slot0, int32_t* status, void* stream);
int32_t cave_hip_pack_large_sparse(const cave_sparse_cones* cones, int64_t nnz_cap, void* workspace, int64_t slice_bytes,
                                   int32_t n_slots, int32_t* n_rows, int32_t* n_nnz, const cave_cone_store* store,
                                   int64_t slot0, int32_t* status, void* stream);

/* The fused step with the NEXT batch on the sparse wire format (additive to v10): cave_hip_cone_step_warm with
 * `next_ctrs, B_next, m_max, d` replaced by the batch -- 24 parameters.  The solve half is the same code reading the
 * same lite store (it does not matter which route packed `solve`, so a chain may alternate dense and sparse batches);
 * the pack half copies the coordinate list of each instance of `next_cones` instead of scanning a dense block, with
 * the limits of the dense pack half (cave_hip_step_lds_bytes of next_cones->m_max, next_cones->d; the same non-zero
 * capacity, the same arena): `next` and `pack_status` get the bits the dense route writes for the densified batch.
 *   warm == NULL                                     the cold kernel
 *   next_cones == NULL or next_cones->B == 0         solve only: exactly cave_hip_cone_step(_warm) without a pack half
 *                                                    (the same kernel; d is solve->d)
 *   B == 0                                           pack only
 * Per instance of the pack half: an entry that breaks the contract above gives pack_status CAVE_ST_BAD_INPUT and
 * slot state -1; more entries than the pack half keeps, or a cone the one-wave solver does not take, CAVE_ST_TOO_LARGE
 * and slot state -1; an instance without entries is the empty cone (state 1).
 * CAVE_E_INVALID before any launch: null or misaligned ent_off / key / val with next_cones->B > 0; next_cones->d
 * different from a store's d; `next` the same store as `solve`; cu_tickets NULL; a shape the fused step does not take
 * (cave_hip_step_lds_bytes < 0, or m_max = 0); a bad cache (as for cave_hip_cone_step_warm). */
int32_t cave_hip_cone_step_sparse(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, int32_t mode,
                                  float sign, float inner_ratio, int32_t max_iter, int32_t flags, float* proj, float* rnorm,
                                  float* target, float* loss, float* grad, int32_t* status, int32_t* iters,
                                  const cave_sparse_cones* next_cones, const cave_lite_store* next, int32_t* pack_status,
                                  const cave_warm_cache* warm, const int64_t* keys, uint8_t* warm_hit, uint32_t* cu_tickets,
                                  void* stream);

/* ------------------------------------------------------------------ interior-point fused step (additive to v10)
 * CAVE_MODE_INNER_IPM on the fused step: cave_hip_cone_step / cave_hip_cone_step_sparse without `mode`, `inner_ratio`
 * and the cache arguments -- 22 and 19 parameters.  The solve half runs max_iter (<= 0: 3) interior-point steps per
 * instance on one wave (the iterates of cave_hip_cone_dense in that mode, up to the order of the sums; `iters` = steps
 * run, 0 for a cone without reduced rows) and the fused loss / gradient of the mode; always cold (the interior iterate
 * is not a starting point).  Everything else -- the pack half and its limits, the stores, ids, B = 0 (pack only),
 * B_next = 0 / next_cones == NULL (solve only), pack_status, CAVE_STEP_ZERO_FAILED, cu_tickets, the CAVE_E_INVALID
 * cases -- is as for the sibling.  cave_hip_cone_step and cave_hip_cone_step_sparse keep refusing the mode. */
int32_t cave_hip_cone_step_ipm(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, float sign,
                               int32_t max_iter, int32_t flags, float* proj, float* rnorm, float* target, float* loss,
                               float* grad, int32_t* status, int32_t* iters, const float* next_ctrs, int64_t B_next,
                               int64_t m_max, int64_t d, const cave_lite_store* next, int32_t* pack_status,
                               uint32_t* cu_tickets, void* stream);
int32_t cave_hip_cone_step_sparse_ipm(const cave_lite_store* solve, const int64_t* ids, const float* pred, int64_t B, float sign,
                                      int32_t max_iter, int32_t flags, float* proj, float* rnorm, float* target, float* loss,
                                      float* grad, int32_t* status, int32_t* iters, const cave_sparse_cones* next_cones,
                                      const cave_lite_store* next, int32_t* pack_status, uint32_t* cu_tickets, void* stream);

/* Device-resident stores: cones are static per instance (src/dataset.py:72), so a packed store whose cones qualify
 * builds the lite slots of ALL its instances once (slot i of `dst` from slot i of `src`, dst->n >= src->n) and then
 * serves batches of ids through the solve half of cave_hip_cone_step (no pack half).  status [src->n] or NULL:
 * CAVE_ST_OK, or CAVE_ST_TOO_LARGE for a cone the one-wave solver does not take (its slot is marked so). */
int32_t cave_hip_lite_from_packed(const cave_cone_store* src, const cave_lite_store* dst, int32_t* status, void* stream);

/* ------------------------------------------------------------------ grid shortest path (additive to v10)
 * The h x w grid DAG of PyEPO's shortest-path model (arcs go right or down; arc order: per grid row its w-1 right arcs,
 * then its w down arcs; d = h (w-1) + (h-1) w), N instances, one wave each, in ONE launch:
 *   costs      [N, d] fp32   the costs the path is optimal for
 *   eval_costs [N, d] fp32   or NULL: a second cost tensor the path is priced under (the regret numerator)
 *   sol        [N, d] fp32   or NULL: 0/1 arc indicator of the shortest source->sink path
 *   obj        [N]    fp64   or NULL: its length under `costs`
 *   eval       [N]    fp64   or NULL: sum_k eval_costs[b, k] sol[b, k] in fp64 (needs eval_costs)
 *   status     [N]           or NULL: CAVE_ST_OK, or CAVE_ST_BAD_INPUT for a non-finite cost (zero sol, NaN obj / eval;
 *                            the other instances are unaffected)
 *   key, val   [N, 5 d]      or both NULL: the tight cone of each vertex on the sparse wire format -- rows
 *                            [A; -A; -e_k for arcs at 0; +e_k for arcs at 1] with A the node-arc matrix (+1 head, -1
 *                            tail), 2 h w + d rows and exactly 5 d entries per instance, so
 *                            ent_off[b] = 5 d b, m_max = 2 h w + d (a bad instance gets the cone of the zero vector)
 * Distances are fp64 sums of the fp32 costs along the path, a candidate replaces a distance only when strictly
 * smaller, arcs in index order (at a tie the down arc into a node wins): paths and objectives do not depend on the
 * batch, the launch or the device.  No workspace, no state between calls.  N == 0: nothing to do, CAVE_OK.
 * CAVE_E_INVALID before any launch: h or w < 1, h w < 2; a grid whose instance does not fit the LDS (the size query
 * below is negative); with key / val, d > 65535 or 2 h w + d > 65535; key without val; eval without eval_costs.
 * The size query returns the LDS bytes one instance needs (at most 163840), or CAVE_E_INVALID. */
int32_t cave_hip_sp_grid_lds_bytes(int64_t h, int64_t w);
int32_t cave_hip_sp_grid_solve(const float* costs, const float* eval_costs, int64_t N, int64_t h, int64_t w, float* sol,
                               double* obj, double* eval, int32_t* status, uint32_t* key, float* val, void* stream);

/* ------------------------------------------------------------------ Held-Karp TSP (additive to v10)
 * The symmetric TSP on n nodes, 3 <= n <= 14 (edges in lexicographic (i<j) order, d = n (n-1) / 2,
 * eid(i,j) = i n - i (i+1) / 2 + j - i - 1), N instances, one 256-thread workgroup each, in ONE launch:
 *   costs      [N, d] fp32   the costs the tour is optimal for
 *   eval_costs [N, d] fp32   or NULL: a second cost tensor the tour is priced under (the regret numerator)
 *   sol        [N, d] fp32   or NULL: 0/1 edge indicator of the optimal tour
 *   obj        [N]    fp64   or NULL: its length under `costs`
 *   eval       [N]    fp64   or NULL: the fp64 sum of eval_costs[b, eid(t_i, t_i+1)] over the tour's n edges in tour order,
 *                            left to right, the closing edge last (needs eval_costs)
 *   tour       [N, n] int32  or NULL: the tour, starting at node 0
 *   status     [N]           or NULL: CAVE_ST_OK, or CAVE_ST_BAD_INPUT for a non-finite cost (zero sol, NaN obj / eval, a
 *                            tour of -1; the other instances are unaffected)
 *   workspace                n <= 12: unused, may be NULL (the table of the dynamic program lies in LDS).  n = 13, 14: a
 *                            device buffer of workspace_bytes bytes, 8-byte aligned, at least one slot; the launch uses
 *                            min(N, workspace_bytes / slot_bytes) workgroups, which stride over the instances, each
 *                            keeping its table, (n-1) 2^(n-2) doubles, in its own slot.  Its contents on entry do not
 *                            matter and mean nothing afterwards.
 * The Held-Karp recurrence in fp64 on the exactly converted fp32 costs: one addition per candidate, candidates in
 * ascending node order, a candidate replaces the minimum only when strictly smaller (the lowest node wins a tie), the
 * closing edge likewise: tours and objectives do not depend on the batch, the launch, the workspace size or the device.
 * No state between calls.  N == 0: nothing to do, CAVE_OK (no workspace needed).
 * CAVE_E_INVALID before any launch: n < 3 or n > 14; eval without eval_costs; for n = 13, 14 and N > 0 a NULL or
 * misaligned workspace or one smaller than one slot.
 * cave_hip_tsp_hk_slot_bytes: 0 where the table lies in LDS (n <= 12), else the bytes of one slot (196608, 425984).
 * cave_hip_tsp_hk_workspace_bytes: slot_bytes * min(N, 512), the default workspace (0 for n <= 12).  Both return
 * CAVE_E_INVALID for an n out of range (the second also for N < 0). */
int64_t cave_hip_tsp_hk_slot_bytes(int64_t n);
int64_t cave_hip_tsp_hk_workspace_bytes(int64_t n, int64_t N);
int32_t cave_hip_tsp_hk_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                              double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                              void* stream);

/* ------------------------------------------------------------------ CVRP dynamic program (additive to v10)
 * The capacitated vehicle routing problem of the reference's vrpModel on the edges of the Held-Karp section above: n
 * nodes, 3 <= n <= 14, node 0 the depot, customers 1 .. n-1 with demands shared by the batch, at most K routes,
 * 1 <= K <= 8, each depot-anchored, of at least two customers and of load <= capacity, every customer on one route.
 * N instances, one 256-thread workgroup each, in ONE launch:
 *   costs      [N, d] fp32   the costs the routes are optimal for
 *   eval_costs [N, d] fp32   or NULL: a second cost tensor the routes are priced under (the regret numerator)
 *   demands    [n-1]  fp32   demand of customer j+1 at [j]
 *   sol        [N, d] fp32   or NULL: 0/1 edge indicator of the optimal routes
 *   obj        [N]    fp64   or NULL: their cost under `costs`
 *   eval       [N]    fp64   or NULL: the fp64 sum, from 0.0, of eval_costs over the routes' edges: route by route in route
 *                            order, each route's edges from the depot out and back (needs eval_costs)
 *   routes     [N, n+K] int32 or NULL: 0, customers of route 1, 0, customers of route 2, 0, ..., 0, then -1; routes in
 *                            order of their lowest customer
 *   status     [N]           or NULL: CAVE_ST_OK; CAVE_ST_BAD_INPUT for a non-finite cost (that instance alone) or a
 *                            negative or non-finite demand (every instance); CAVE_ST_INFEASIBLE where no partition into
 *                            feasible routes exists.  A failed instance gets a zero sol, NaN obj / eval, routes of -1.
 *   workspace                where cave_hip_vrp_dp_slot_bytes(n, K) is 0: unused, may be NULL (the tables lie in LDS).
 *                            Else a device buffer of workspace_bytes bytes, 8-byte aligned, at least one slot; the launch
 *                            uses min(N, workspace_bytes / slot_bytes) workgroups, which stride over the instances.  Its
 *                            contents on entry do not matter and mean nothing afterwards.
 * The dynamic program in fp64 on the exactly converted fp32 inputs (customer j+1 is bit j of a set S):
 *   dp[S, j]  the Held-Karp table above;   load(S) the sum of the demands over j in S, ascending j, from 0.0
 *   r(S)   = min over j in S, ascending, of dp[S, j] + cost(j+1, 0) where S has two or more customers and load(S) <=
 *            capacity (a load equal to the capacity fits), else +inf
 *   g_1 = r;  g_k(S) = min over R containing the lowest customer of S, R a proper subset of S, in ascending numeric order
 *            of R, of r(R) + g_(k-1)(S \ R)
 *   obj    = min over k = 1 .. min(K, (n-1)/2), ascending, of g_k(all customers)
 * every minimum the first one (a candidate replaces the minimum only when strictly smaller), and the routes are walked
 * back through the same argmins: results do not depend on the batch, the launch, the workspace size or the device.
 * With K = 1 and a capacity above the total load this is cave_hip_tsp_hk_solve.  No state between calls.
 * N == 0: nothing to do, CAVE_OK.
 * CAVE_E_INVALID before any launch: n or K out of range; eval without eval_costs; a capacity that is not finite and
 * positive; with N > 0 a NULL costs or demands, or, where a slot is needed, a NULL or misaligned workspace or one
 * smaller than one slot.
 * Tables: the Held-Karp table, (n-1) 2^(n-2) doubles, and (min(K, (n-1)/2) - 1) 2^(n-1) doubles for r and the stored
 * layers.  What fits the 160 KiB of LDS beside the small arrays stays there (both; else the second alone), the rest
 * makes up the slot.  cave_hip_vrp_dp_slot_bytes: the bytes of one slot (0: none needed).
 * cave_hip_vrp_dp_workspace_bytes: slot_bytes * min(N, 512), the default workspace.  Both return CAVE_E_INVALID for
 * an n or K out of range (the second also for N < 0). */
int64_t cave_hip_vrp_dp_slot_bytes(int64_t n, int64_t K);
int64_t cave_hip_vrp_dp_workspace_bytes(int64_t n, int64_t K, int64_t N);
int32_t cave_hip_vrp_dp_solve(const float* costs, const float* eval_costs, const float* demands, double capacity,
                              int64_t K, int64_t N, int64_t n, float* sol, double* obj, double* eval,
                              int32_t* routes, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ Held-Karp TSP, wide tier (additive to v10)
 * The Held-Karp section above for 13 <= n <= 20: the same problem, arguments, outputs, recurrence (bit for bit the same
 * results; at n = 13, 14 the bytes cave_hip_tsp_hk_solve writes) and failure semantics, with a table that always lies in
 * the caller's workspace: one 512-thread workgroup per slot, workgroups striding over the N instances.
 *   workspace   a device buffer of workspace_bytes bytes, 8-byte aligned: a header region of 4 * 2^(n-1) bytes (filled
 *               on every call by a small kernel in front of the sweep, same stream) followed by slots of slot_bytes =
 *               8 (n-1) 2^(n-2) bytes (196608 at n = 13 ... 39845888 at n = 20), at least one.  The launch uses
 *               min(N, (workspace_bytes - header) / slot_bytes) workgroups.  Its contents on entry do not matter and
 *               mean nothing afterwards; two calls that may run at the same time need a workspace each.
 * No state between calls.  N == 0: nothing to do, CAVE_OK (no workspace needed).
 * CAVE_E_INVALID before any launch, nothing written: n < 13 or n > 20; eval without eval_costs; with N > 0 a NULL or
 * misaligned workspace or one smaller than the header region plus one slot.
 * cave_hip_tsp_hk_wide_slot_bytes: the bytes of one slot.
 * cave_hip_tsp_hk_wide_workspace_bytes: header + slot_bytes * min(N, slots(n)), the default workspace, with
 * slots(n) = min(512, floor(8 GiB / slot_bytes)): 512 up to n = 18, 455 at n = 19, 215 at n = 20 -- a default, not a limit.
 * Both return CAVE_E_INVALID for an n out of range (the second also for N < 0). */
int64_t cave_hip_tsp_hk_wide_slot_bytes(int64_t n);
int64_t cave_hip_tsp_hk_wide_workspace_bytes(int64_t n, int64_t N);
int32_t cave_hip_tsp_hk_wide_solve(const float* costs, const float* eval_costs, int64_t N, int64_t n, float* sol, double* obj,
                                   double* eval, int32_t* tour, int32_t* status, void* workspace, int64_t workspace_bytes,
                                   void* stream);

/* ------------------------------------------------------------------ CVRP dynamic program, wide tier (additive to v10)
 * The CVRP section above for 13 <= n <= 20 and 1 <= K <= 8: the same problem, arguments (in the same order), outputs,
 * recurrences (bit for bit the same results; at n = 13, 14 the bytes cave_hip_vrp_dp_solve writes) and failure
 * semantics, with tables that always lie in the caller's workspace: one 512-thread workgroup per slot, workgroups
 * striding over the N instances.
 *   workspace   a device buffer of workspace_bytes bytes, 8-byte aligned: a header region of 4 * 2^(n-1) bytes (filled
 *               on every call by a small kernel in front of the dynamic program, same stream) followed by slots of
 *               slot_bytes = 8 (n-1) 2^(n-2) + 8 (min(K, (n-1)/2) - 1) 2^(n-1) bytes (the Held-Karp table, then r and
 *               the stored layers: 39845888 + 4194304 (min(K, 9) - 1) at n = 20), at least one.  The launch uses
 *               min(N, (workspace_bytes - header) / slot_bytes) workgroups.  Its contents on entry do not matter and
 *               mean nothing afterwards; two calls that may run at the same time need a workspace each.
 * No state between calls.  N == 0: nothing to do, CAVE_OK (no workspace needed).
 * CAVE_E_INVALID before any launch, nothing written: n < 13 or n > 20, K < 1 or K > 8; eval without eval_costs; a
 * capacity that is not finite and positive; with N > 0 a NULL or misaligned workspace or one smaller than the header
 * region plus one slot, or a NULL costs or demands.
 * cave_hip_vrp_dp_wide_slot_bytes: the bytes of one slot.
 * cave_hip_vrp_dp_wide_workspace_bytes: header + slot_bytes * min(N, 512, floor(8 GiB / slot_bytes)), the default
 * workspace -- a default, not a limit.  Both return CAVE_E_INVALID for an n or K out of range (the second also for
 * N < 0). */
int64_t cave_hip_vrp_dp_wide_slot_bytes(int64_t n, int64_t K);
int64_t cave_hip_vrp_dp_wide_workspace_bytes(int64_t n, int64_t K, int64_t N);
int32_t cave_hip_vrp_dp_wide_solve(const float* costs, const float* eval_costs, const float* demands, double capacity,
                                   int64_t K, int64_t N, int64_t n, float* sol, double* obj, double* eval,
                                   int32_t* routes, int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ tight cones of any binary LP (additive to v10)
 * The reference's extraction rule (`_extract_tight_normals`, src/dataset.py:147-215) for N vertices of one constraint
 * system, written directly on the sparse wire format (cave_sparse_cones): what cave_hip_sp_grid_solve's key / val do for
 * the grid's node-arc matrix, for any matrix.  A system is R rows over d columns in CSR form; every array a device
 * pointer, caller-owned, read-only:
 *   row_off [R+1] int64   0 <= row_off[r] <= row_off[r+1] <= Z
 *   col     [Z]   int32   0 <= col < d, strictly increasing within a row
 *   coef    [Z]   fp32    non-zero and finite
 *   sense   [R]   int8    0 `<=`, 1 `>=`, 2 `==`
 *   rhs     [R]   fp64    finite
 * `sys` is shared by the batch.  `lazy` (or NULL) is a second system over the same d whose rows lazy_off[b] ..
 * lazy_off[b+1] (lazy_off [N+1] int64, 0 <= lazy_off[b] <= lazy_off[b+1] <= lazy->R) belong to instance b alone.
 * sol [N, d] fp32 holds the vertices; tol (fp64, finite, >= 0) is the reference's `tol`.
 * A row is tight when |rhs - sum_j (double)coef_j (double)sol_j| < tol, products and sum in fp64 (the order of the
 * additions is not fixed).  Per instance the rows are numbered from 0 in this order, and the entries come out in strictly
 * increasing key = (row << 16) | col:
 *   1 the tight `<=` rows of sys, in row order, as they are     2 the tight `>=` rows, negated
 *   3 the tight `==` rows, as they are                          4 the same `==` rows, negated
 *   5 the instance's tight lazy rows in list order, each oriented: `>=` negated, `==` the row and then its negation
 *   6 -e_k for every k with (double)sol_k <= tol, ascending     7 +e_k for every k with (double)sol_k >= 1 - tol, not in 6
 * A tight row without entries takes a row number and writes nothing (the zero row the reference would emit).
 * Two passes, because the entry count differs per instance:
 *   cave_hip_tight_cones_count  writes n_rows [N] int32 (a cave_sparse_cones' m_max is their maximum), n_ent [N] int64
 *                               and status [N] (or NULL)
 *   cave_hip_tight_cones_fill   takes ent_off [N+1] int64, the caller's exclusive scan of n_ent, and writes key / val
 *                               [ent_cap] (ent_cap >= ent_off[N]); status [N] or NULL
 * Per-instance status: CAVE_ST_BAD_INPUT for a non-finite sol value, a lazy_off window or a lazy row of that instance
 * that breaks the contract above (the other instances are unaffected), and -- for every instance alike -- a sys that
 * breaks it; CAVE_ST_TOO_LARGE for more than 65535 rows.  A failed instance counts 0 rows and 0 entries, and the fill
 * pass writes nothing for it; the fill pass also writes nothing, and reports CAVE_ST_BAD_INPUT, for an instance whose
 * window ent_off[b] .. ent_off[b+1] is not the size the count pass reports or does not lie in [0, ent_cap].  Every index
 * read from an input is checked before it is used: nothing is read or written out of range.  One wave per instance, no
 * workspace, no state between calls; results do not depend on the batch or the launch.  N == 0: nothing to do, CAVE_OK.
 * CAVE_E_INVALID before any launch: sys NULL; d outside 1..65535; lazy->d != sys->d; a negative R, Z, N or ent_cap; tol
 * not finite or < 0; lazy rows (lazy->R > 0) without lazy_off; with N > 0 a null or misaligned array (those of a system
 * with R > 0 -- col / coef with Z > 0 --, sol, n_rows, n_ent, ent_off, key / val with ent_cap > 0; a given lazy_off). */
typedef struct cave_lin_system {
  int64_t R;       /* rows */
  int64_t Z;       /* entries: row_off[R] */
  int32_t d;       /* columns, 1..65535 */
  int32_t reserved;
  const int64_t* row_off;
  const int32_t* col;
  const float* coef;
  const int8_t* sense;
  const double* rhs;
} cave_lin_system;

int32_t cave_hip_tight_cones_count(const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off,
                                   const float* sol, int64_t N, double tol, int32_t* n_rows, int64_t* n_ent, int32_t* status,
                                   void* stream);
int32_t cave_hip_tight_cones_fill(const cave_lin_system* sys, const cave_lin_system* lazy, const int64_t* lazy_off,
                                  const float* sol, int64_t N, double tol, const int64_t* ent_off, int64_t ent_cap,
                                  uint32_t* key, float* val, int32_t* status, void* stream);

/* ------------------------------------------------------------------ APGD projector (additive to v10)
 * The reference's accelerated projected-gradient projector (`project_apgd`, src/qpsolver.py:11-110) restated on the
 * device, on the wire formats themselves: it iterates in the multiplier space of the ORIGINAL rows, so +a/-a pairs, unit
 * rows, repeated rows and zero padding stay as they are (the stores hold the reduced cone and cannot serve).  Per
 * instance, with A the m_max x d block as given and y = sign * pred, all arithmetic in fp64:
 *   step size   v = 1/sqrt(m_max) in every row; power_iter times  u = A^T v, v = A u, v /= max(||v||, 1e-8);
 *               s = 1 / max(||A^T v||^2, 1e-8)                                        (m_max is the batch's)
 *   iterations  from x_curr = x_prev = 0, for k = k_start .. k_start + n_iter - 1 with beta_k = (k-2)/(k+1), beta_0 = 0:
 *               y_k = x_curr + beta_k (x_curr - x_prev);  g = A (A^T y_k - y);  x_prev = x_curr;  x_curr = max(y_k - s g, 0)
 * Arguments:
 *   ctrs, pred, B, m_max, d   as cave_hip_cone_dense (1 <= m_max, d <= 65535), or `cones` on the sparse wire format
 *   mode        CAVE_MODE_PROJECT (writes proj, rnorm) or CAVE_MODE_EXACT (also target = proj / max(||proj||, 1e-8),
 *               loss = 1 - cos(y, target) and grad, the epilogue that mode has everywhere; src/cave.py:129,213-214)
 *   sign        +1 or -1
 *   k_start     0: the launch computes the step size and starts from zero; > 0: it continues from the state
 *   n_iter      iterations of this launch, 0 .. 100000;   power_iter  0 .. 64
 *   nnz_cap     entries per instance the LDS arena holds, 1 .. m_max * d, with cave_hip_apgd_lds_bytes(m_max, d, nnz_cap) > 0
 *   x_curr, x_prev [B, m_max] fp64, step [B] fp64   caller-owned state, all three or none: read when k_start > 0 (then
 *               required), written back by every launch that is given them
 *   proj, rnorm (un-squared), target, loss, grad, status, iters   as cave_hip_cone_dense, any may be NULL; iters = n_iter
 *   pgrad [B] fp64 or NULL   the reference's check quantity (src/qpsolver.py:52-57):
 *               max_i (x_i > 0 ? |g_i| : max(-g_i, 0)) with g = A (A^T x_curr - y)
 * Per-instance status: CAVE_ST_BAD_INPUT for a non-finite prediction or dense entry, or a sparse entry that breaks the
 * contract of cave_sparse_cones; CAVE_ST_TOO_LARGE for more than nnz_cap entries.  A failed instance gets NaN in every
 * float output and in pgrad, iters 0, and its state is left alone; the other instances are unaffected.
 * One workgroup per instance, of one wave, or of four when m_max, d or nnz_cap exceeds 512.  Every row sum and column sum
 * is accumulated by one lane in index order, without atomics: results are bit-reproducible, do not depend on the batch,
 * on the position in it, on the wire format or on the workgroup size, and a chain of launches through the state equals
 * the single launch bit for bit.  No loop bound depends on the values.  B == 0: nothing to do, CAVE_OK.
 * CAVE_E_INVALID before any launch: a shape, mode, sign, k_start (> 2^30), n_iter, power_iter or nnz_cap out of range; an
 * arena beyond 160 KiB; a null or misaligned pred / ctrs / ent_off / key / val; a partial state, a continuation without
 * state, a misaligned state or pgrad; B >= 2^31.
 * cave_hip_apgd_lds_bytes: the LDS arena of one workgroup, 28 m_max + 20 d + 14 nnz_cap bytes and change (TSP-20, m_max
 * 235, d 190, 1617 entries: 33168, four workgroups per compute unit; SP 5x5, 90 x 40, 256 entries: 6992), or -1
 * where a shape or capacity is out of range or the arena exceeds 160 KiB (at TSP-20's shape: beyond about 10 900 entries). */
int32_t cave_hip_apgd_lds_bytes(int64_t m_max, int64_t d, int64_t nnz_cap);
int32_t cave_hip_cone_apgd(const float* ctrs, const float* pred, int64_t B, int64_t m_max, int64_t d, int32_t mode, float sign,
                           int32_t k_start, int32_t n_iter, int32_t power_iter, int32_t nnz_cap, double* x_curr, double* x_prev,
                           double* step, float* proj, float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                           int32_t* iters, double* pgrad, void* stream);
int32_t cave_hip_cone_apgd_sparse(const cave_sparse_cones* cones, const float* pred, int32_t mode, float sign, int32_t k_start,
                                  int32_t n_iter, int32_t power_iter, int32_t nnz_cap, double* x_curr, double* x_prev, double* step,
                                  float* proj, float* rnorm, float* target, float* loss, float* grad, int32_t* status,
                                  int32_t* iters, double* pgrad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CAVE_HIP_H */
