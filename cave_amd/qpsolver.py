"""Batched cone projection on MI355X — the `solver='hip'` arm.

Host-side mirror of the reference's plug point: a lazily imported function
``f(tight_ctrs, signed_cost, **solver_kwargs) -> (proj (B,d), rnorm (B,))``
living next to ``project_apgd`` (/root/reference src/qpsolver.py:11-63, called
from ``_batch_project`` src/cave.py:242-244), but with **nnls semantics**
(src/cave.py:298-309): exact Euclidean projection onto
``cone{lam @ ctrs_b : lam >= 0}``, zero-padded rows ignored, empty cone returns
the input, ``rnorm`` is the un-squared residual norm.

One call is one HIP kernel launch (cave_amd/csrc/kernels.h), or two for small cones on the dense wire
format (the "split" form below: a 4-wave streaming pack kernel, then a 1-wave solve kernel);
this module only marshals pointers, picks launch limits and turns per-instance
status codes into the reference's error behaviour.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import (MODE_AVG, MODE_EXACT, MODE_HEURISTIC, MODE_INNER, MODE_PROJECT, ST_BAD_INPUT,
                   ST_NOT_CONVERGED, ST_OK, ST_TOO_LARGE)
from .sparse import SparseCones

__all__ = ["project_hip", "average_ctrs_hip", "cone_op_dense", "HipSolverError", "PreparedCones", "prepare_dense",
           "prepare_sparse", "prepare_cones", "cone_op_prepared", "step_lds_bytes", "cone_op_sparse", "project_hip_sparse",
           "cone_op_apgd", "cone_op_apgd_sparse", "project_apgd_hip"]


class HipSolverError(RuntimeError):
    """Per-instance solver failure (SciPy's nnls raises RuntimeError on its iteration cap, src/cave.py:307)."""


def _as_device(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _grow_limits(m: int, d: int) -> tuple[int, int]:
    """Largest arena a workgroup can have (160 KiB) and a non-zero capacity that leaves room for the
    rest: the scan output (8 B per non-zero) is a build-phase temporary, so it may take about half."""
    cap = int(_lib.MAX_LDS * 0.55) // 8 - 256
    return int(min(cap, max(m * d, 64))), _lib.MAX_LDS


# shapes (m_max, d) whose cones did not fit the default (structured-cone) arena: go straight to the
# tier that worked next time instead of paying failed launches per call
#   tier 1: full 160 KiB LDS arena (one workgroup per CU, four waves with the wide register budget: waves=8);
#   tier 2: large-cone path (global workspace)
_tier: dict[tuple[int, int], int] = {}
# shapes (m_max, d) whose cones were seen (by a status-checked launch) to fit / not to fit the 4-wave
# workgroup shape (reduced systems up to 32 rows), the fastest one while the GPU has idle SIMDs
_wide_ok: dict[tuple[int, int], bool] = {}


def _auto_waves(B: int, m: int, d: int, check: bool) -> int:
    """Waves per instance of the FUSED dense kernel when the caller leaves it open (cones with d <= 256 normally
    take the split form instead, see launch_split).  Four waves shorten the streaming scan while the GPU has idle
    SIMDs (TSP-20, B = 1024, rotating batches, r02: 219 us with 4 waves, 193 with 2, 196 with 1); one wave per
    instance wins beyond ~1300 instances (more instances in flight).  Four waves hold reduced systems up to 32
    rows and are only used once a status-checked launch has shown the shape fits."""
    if B > 1280:
        return 1  # reduced systems up to 64 rows, like the 2-wave shape
    ok = _wide_ok.get((m, d))
    if ok is True or (ok is None and check):
        return 4
    return 2

_large_hint: dict[tuple[int, int], tuple[int, int]] = {}  # (m, d) -> (nnz_cap, band_entries) that fitted
# shapes that have completed a clean status-checked call (any wave count, any tier): only these may be
# launched unchecked / lazily with what was learnt; `forget_shape` takes a shape out again
_settled: set[tuple[int, int]] = set()


def forget_shape(m: int, d: int) -> None:
    """Drop everything remembered about (m_max, d).  Called when an unchecked or lazily checked launch
    reported CAVE_ST_TOO_LARGE: the caches are keyed by shape only, and a later batch of the same shape
    may hold bigger cones (more reduced rows / non-zeros) than the one that settled it.  The next call
    for the shape then runs status-checked and walks the tiers again."""
    key = (int(m), int(d))
    _tier.pop(key, None)
    _wide_ok.pop(key, None)
    _large_hint.pop(key, None)
    _split_ok.pop(key, None)
    _sparse_split_ok.pop(key, None)
    _step_ok.pop(key, None)
    _apgd_cap.pop(key, None)
    _settled.discard(key)


def _large_guess(m: int, d: int) -> tuple[int, int]:
    """Initial (nnz_cap, band_entries) of the large-cone path: structured cones carry <= d unit entries
    plus a few sparse rows; the reduced systems of the CaVE benchmarks are ~sqrt(2d) dense rows (TSP
    degree rows) or ~d/2 rows of bandwidth ~sqrt(d/2) (grid flow rows): both well under 32*d entries."""
    cap = int(min(max(m * d, 64), 4 * (m + d) + 256))
    return cap, 32 * d + 4096


def fast_path_cannot_fit(d: int) -> bool:
    """The per-coordinate arrays of the LDS-resident solver (sign byte, column pointers, y, avg,
    residual, clipped residual, direction, flags: ~38 bytes per cost coordinate) alone exceed 160 KiB."""
    return 38 * d + 4096 > _lib.MAX_LDS


# ---- "split" form of the dense operator for small cones (d <= 256):
#   kernel 1  cave_hip_pack_fill in slot mode: four waves per instance stream the dense block and leave the
#             reduced cone in a fixed-capacity slot of a transient device store (one pass over the dense bytes);
#   kernel 2  cave_hip_cone_packed with ONE wave per instance, whose small-cone ("lite") solver wants ~200
#             registers -- more than the 4-wave streaming shape can give without losing residency.
# The two kernels each get the launch shape they need; the transient store costs ~10 KB of extra HBM traffic per
# instance against 178 KB of dense input (TSP-20).  Instances beyond the slot capacity (more than 32 reduced
# rows / 1536 non-zeros, or entries other than +-1) report TOO_LARGE and the batch falls back to the fused kernel.
SPLIT_MAX_D, SPLIT_ROWS, SPLIT_NNZ = 256, 32, 1536
_slot_stores: dict = {}
_split_ok: dict[tuple[int, int], bool] = {}  # (m, d) -> the split form fitted every instance of a checked batch
_sparse_split_ok: dict[tuple[int, int], bool] = {}  # the same for batches on the sparse wire format (cone_op_sparse)


class _SlotStore:
    def __init__(self, dev, B: int, d: int):
        self.B, self.d = B, d
        ar = torch.arange(B + 1, dtype=torch.int64, device=dev)
        self.t, self.c = _lib.alloc_store(dev, d, ar * SPLIT_ROWS, ar * SPLIT_NNZ, B * SPLIT_ROWS, B * SPLIT_NNZ, slot_mode=True)
        self.ref = C.byref(self.c)
        self.pack_status = torch.empty(B, dtype=torch.int32, device=dev)
        self.lds_bytes = int(_lib.load_library().cave_hip_packed_lds_bytes(d, SPLIT_ROWS, SPLIT_NNZ, 1))
        self.gen = 0  # bumped every time prepare_dense hands this store out (PreparedCones.stale)


def _slot_store(dev, B: int, d: int) -> _SlotStore:
    key = (dev, B, d)
    st = _slot_stores.get(key)
    if st is None:
        if len(_slot_stores) >= 4:
            _slot_stores.pop(next(iter(_slot_stores)))
        st = _slot_stores[key] = _SlotStore(dev, B, d)
    if st.lds_bytes <= 0:
        raise HipSolverError("split form: no LDS configuration")
    return st


# ---- prepared form: the two stages of a step on the dense format, decoupled and then FUSED ACROSS STEPS.
# The pack stage (stream the dense block, build the reduced cone) depends on the cones only, not on the prediction,
# and a training loop knows the cones of the NEXT batch before it has the next prediction (the DataLoader has
# already collated it: src/dataset.py:133-144).  `prepare_dense(ctrs)` runs the pack stage of a batch into a transient
# "lite store"; `prep.then(next_ctrs)` attaches the following batch, and `cone_op_prepared(prep, pred, ...)` then
# launches ONE grid (cave_hip_cone_step): the one-wave solve blocks of this batch first, the four-wave pack blocks of
# the next batch behind them, filling what the solve waves leave of each compute unit.  Steady state per step =
# max(pack, solve) instead of their sum, on one stream: no side stream, no event, no spacer kernel (rounds 2-3 ran the
# pack on a side stream behind a tuned `torch.cuda._sleep`, which decided a dispatch race and depended on how the
# runtime maps streams to hardware queues).  `cave_amd.dataset.prefetch(loader)` does the wiring for a DataLoader.
STEP_MAX_B = 2048   # the one-wave solver is a latency design: beyond ~2 instances per SIMD the general path wins
STEP_POOL = 3       # lite stores cycled per (device, stream, B, d); two are in use by a running chain
_step_pool: dict = {}
_step_lds: dict = {}
_step_ok: dict[tuple[int, int], bool] = {}  # (m, d) -> a checked batch of this shape had a cone the lite form does not take
_tickets: dict = {}


class _LiteSlots:
    """B slots of a cave_lite_store (include/cave_hip.h) + the pack status of the batch it holds (or, for a
    device-resident ConeStore, of all its instances)."""

    def __init__(self, dev, B: int, d: int):
        self.B, self.d = B, d
        t = {
            "hdr": torch.zeros(B * 8, dtype=torch.int32, device=dev),
            "usign": torch.zeros(B * d, dtype=torch.uint8, device=dev),
            "avg": torch.zeros(B * d, dtype=torch.float32, device=dev),
            "rowptr": torch.zeros(B * 33, dtype=torch.int32, device=dev),
            "ell": torch.zeros(B * 4 * d, dtype=torch.int32, device=dev),
            "csr16": torch.zeros(B * 768, dtype=torch.int32, device=dev),
            "rl": torch.zeros(B * 32, dtype=torch.uint8, device=dev),
        }
        self.t = t
        self.c = _lib.LiteStore(n=B, d=d, reserved=0, **{k: v.data_ptr() for k, v in t.items()})
        self.ref = C.byref(self.c)
        self.pack_status = torch.empty(B, dtype=torch.int32, device=dev)
        self.gen = 0  # bumped every time the store is handed out (PreparedCones.stale)


def _tickets_for(dev) -> torch.Tensor:
    t = _tickets.get(dev)
    if t is None:
        t = _tickets[dev] = torch.zeros(4096, dtype=torch.int32, device=dev)
    return t


def step_lds_bytes(m: int, d: int) -> int:
    """LDS per workgroup of the fused step kernel for dense batches of shape (m_max, d); <= 0: does not qualify."""
    key = (int(m), int(d))
    v = _step_lds.get(key)
    if v is None:
        v = _step_lds[key] = int(_lib.load_library().cave_hip_step_lds_bytes(key[0], key[1]))
    return v


def _take_store(dev, B: int, d: int, avoid=None) -> _LiteSlots:
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, B, d)
    pool = _step_pool.get(key)
    if pool is None:
        if len(_step_pool) >= 8:
            _step_pool.pop(next(iter(_step_pool)))
        pool = _step_pool[key] = []
    if len(pool) < STEP_POOL:
        ss = _LiteSlots(dev, B, d)
    else:
        ss = pool.pop(0)  # round robin: the store handed out STEP_POOL calls ago (its holder is stale from now on)
        if ss is avoid:
            pool.append(ss)
            ss = pool.pop(0)
    pool.append(ss)
    ss.gen += 1
    return ss


class PreparedCones:
    """A batch -- a dense (B, m_max, d) tensor or a SparseCones -- whose reduced cones sit in a transient lite store
    (packed by an earlier launch on the same stream).  Usable in place of `tight_ctrs` in a loss call.
    `then(next_cones)` attaches the batch that follows, a tensor or a SparseCones (its kind chooses the kernel; the
    solve half does not care which route packed its store, so a chain may alternate): the loss call then packs it in
    the same launch and leaves its PreparedCones in `.next`.  Keeps the batch itself (`ctrs`) alive for the fallback of
    a batch the lite form does not take -- or whose store has been handed out again in the meantime (`gen` no longer
    matches: more prepared batches held than the pool has stores)."""

    def __init__(self, ctrs, store: _LiteSlots, gen: int):
        self.ctrs, self.store, self.gen = ctrs, store, gen
        self.sparse = not isinstance(ctrs, torch.Tensor)
        self.shape = _shape(ctrs)
        self.follow = None   # the batch after this one (consumed by the first solve)
        self.next = None     # what to pass for that batch: a PreparedCones, or the batch itself

    def stale(self) -> bool:
        return self.gen != self.store.gen

    def then(self, next_cones) -> "PreparedCones":
        self.follow, self.next = next_cones, None
        return self

    # a training loop moves every field of a batch to the device (code_sample.py:50): nothing to move here
    def cuda(self, *a, **k) -> "PreparedCones":
        return self

    def to(self, *a, **k) -> "PreparedCones":
        return self

    @property
    def device(self):
        return self.ctrs.device


def _shape(x) -> tuple[int, int, int]:
    """(B, m_max, d) of a batch of cones on either wire format."""
    return tuple(x.shape) if isinstance(x, torch.Tensor) else (len(x), x.m_max, x.d)


def _step_qualifies(x) -> bool:
    """The fused step takes this batch: a dense (B, m_max, d) tensor or a SparseCones, on the device.  The rules on
    (B, m_max, d) and the verdicts are the same for both (`_step_ok` is shared: from the same non-zeros the two pack halves
    refuse the same cones); the sparse pack half keeps row indices in 15 bits."""
    if isinstance(x, torch.Tensor):
        if not (x.is_cuda and x.dim() == 3):
            return False
    elif not (isinstance(x, SparseCones) and x.is_cuda and x.m_max <= 32767):
        return False
    B, m, d = _shape(x)
    return 0 < m and d <= SPLIT_MAX_D and 0 < B <= STEP_MAX_B and _step_ok.get((m, d)) is not False and step_lds_bytes(m, d) > 0


_step_qualifies_sparse = _step_qualifies


def _alloc_out(outputs, B: int, d: int, dev):
    """-> (out, status, iters): the outputs asked for ([B] for rnorm / loss, else [B, d]) plus out["status"] / out["iters"]."""
    out = {name: torch.empty((B,) if name in ("rnorm", "loss") else (B, d), dtype=torch.float32, device=dev) for name in outputs}
    status = out["status"] = torch.empty(B, dtype=torch.int32, device=dev)
    iters = out["iters"] = torch.empty(B, dtype=torch.int32, device=dev)
    return out, status, iters


def _out_ptrs(out, status, iters) -> tuple:
    """The seven trailing output pointers of every operator entry point (NULL: not asked for)."""
    ptr, get = _lib.ptr, out.get
    return (ptr(get("proj")), ptr(get("rnorm")), ptr(get("target")), ptr(get("loss")), ptr(get("grad")), ptr(status), ptr(iters))


def _launch_step(solve, pred, B, mode, sign, inner_ratio, max_iter, out, status, iters, nxt, nxt_store, ids=None,
                 zero_failed=False, warm=None, keys=None):
    """One launch of the step kernel: the solve half for `solve` (None / B = 0: pack only) and the pack half for `nxt`
    into `nxt_store` -- None (solve only), a dense tensor (cave_hip_cone_step) or a SparseCones (cave_hip_cone_step_sparse).
    `warm` (a cave_amd.warm.WarmCache): the warm variant, which starts each solve from the cache's multipliers for its
    key -- `keys` [B] int64, or None: the content of the cone -- and writes the final ones back; out["warm_hit"] [B] uint8
    then tells which instances hit.  Mode INNER_IPM goes to the kernels of its own (cave_hip_cone_step_ipm /
    _sparse_ipm), which have no cache: `warm` is ignored, the mode runs cold."""
    lib = _lib.load()
    ptr = _lib.ptr
    sparse = nxt is not None and not isinstance(nxt, torch.Tensor)
    dev = status.device if status is not None else nxt.device
    name, cache = "cave_hip_cone_step_sparse" if sparse else "cave_hip_cone_step", ()
    flag = 1 if zero_failed else 0
    if mode == _lib.MODE_INNER_IPM and B > 0:
        name += "_ipm"
        scalars = (float(sign), int(max_iter), flag)
    else:
        scalars = (int(mode), float(sign), float(inner_ratio), int(max_iter), flag)
        if sparse:  # one entry point, cold when its cache is NULL (a pack-only launch has nothing to warm-start)
            hit = None
            if warm is not None and B > 0:
                hit = out["warm_hit"] = torch.empty(B, dtype=torch.uint8, device=dev)
            cache = (warm.ref if hit is not None else None, ptr(keys), ptr(hit))
        elif warm is not None:
            name += "_warm"
            hit = out["warm_hit"] = torch.empty(B, dtype=torch.uint8, device=dev)
            cache = (warm.ref, ptr(keys), ptr(hit))
    if sparse:
        pack = (nxt.c_ref(), nxt_store.ref, ptr(nxt_store.pack_status))
    elif nxt is not None:
        pack = (ptr(nxt), *nxt.shape, nxt_store.ref, ptr(nxt_store.pack_status))
    else:
        pack = (None, 0, 0, solve.d, None, None)
    rc = getattr(lib, name)(solve.ref if solve is not None else None, ptr(ids), ptr(pred), B, *scalars,
                            *_out_ptrs(out, status, iters), *pack, *cache, ptr(_tickets_for(dev)), _lib.current_stream())
    _lib.check(rc, name)


_launch_step_sparse = _launch_step


def _on_device(x, dev):
    """A batch of cones as the kernels read it (float32, contiguous) on `dev`."""
    return _as_device(x, dev) if isinstance(x, torch.Tensor) else x.to(dev)


def prepare_cones(x):
    """Run the pack stage of a batch -- a dense tensor or a SparseCones -- now, on the current stream: a pack-only launch
    of the step kernel into a pooled lite store.  Returns the batch itself (a SparseCones: on the device) when the shape
    does not qualify; the loss call then takes the ordinary path."""
    _lib.load()
    if not isinstance(x, torch.Tensor) and not x.is_cuda:
        x = x.cuda()
    if not _step_qualifies(x):
        return x
    dev = x.device
    x = _on_device(x, dev)
    B, _, d = _shape(x)
    with torch.cuda.device(dev):
        ss = _take_store(dev, B, d)
        _launch_step(None, None, 0, MODE_PROJECT, 1.0, 0.0, 0, {}, None, None, x, ss)
    return PreparedCones(x, ss, ss.gen)


prepare_dense = prepare_sparse = prepare_cones


def cone_op_prepared(prep: PreparedCones, pred_cost: torch.Tensor, mode: int, sign: float = 1.0, inner_ratio: float = 0.2, *,
                     max_iter: int = 0, check: bool = True, zero_failed: bool = False,
                     outputs: tuple[str, ...] = ("proj", "rnorm"), warm=None, keys=None) -> dict[str, torch.Tensor]:
    """The solve stage for a prepared batch (same outputs as cone_op_dense) and, in the same launch, the pack stage of
    the batch attached with `prep.then(...)` -- a dense tensor (cave_hip_cone_step) or a SparseCones
    (cave_hip_cone_step_sparse) -- whose PreparedCones is left in `prep.next`.  A batch with a cone the lite
    form does not take falls back to the general operator of its own wire format, cone_op_dense or cone_op_sparse
    (checked calls only; unchecked calls report CAVE_ST_TOO_LARGE in `status`); an instance the sparse loader rejected
    reports CAVE_ST_BAD_INPUT.  `warm` (cave_amd.warm.WarmCache on this device) / `keys` ([B] int64 or None:
    keyed by cone content): warm start from the cache, out["warm_hit"] says where it hit (the fallbacks run cold).
    Mode INNER_IPM runs the interior-point step kernels (cave_hip_cone_step_ipm / _sparse_ipm), always cold."""
    _lib.load()
    B, m, d = prep.shape
    dev = prep.ctrs.device

    def general(chk):  # the batch itself through the general operator of its wire format
        op = cone_op_sparse if prep.sparse else cone_op_dense
        return op(prep.ctrs, pred_cost, mode, sign, inner_ratio, max_iter=max_iter, check=chk, outputs=outputs)

    follow, prep.follow = prep.follow, None
    if prep.stale():
        # its store now holds a later batch: solve from the batch itself
        if follow is not None:
            prep.next = prepare_cones(follow)
        return general(check)
    pred = _as_device(pred_cost, dev)
    if pred.shape != (B, d):
        raise ValueError(f"pred_cost must have shape ({B}, {d}), got {tuple(pred.shape)}")
    with torch.cuda.device(dev):
        out, status, iters = _alloc_out(outputs, B, d, dev)
        nxt = nstore = None
        if follow is not None:
            # (a dense batch is moved to this device; a sparse one on another device goes the ordinary way)
            if _step_qualifies(follow) and (isinstance(follow, torch.Tensor) or follow.device == dev):
                nxt = _on_device(follow, dev)
                Bn, _, dn = _shape(nxt)
                nstore = _take_store(dev, Bn, dn, avoid=prep.store)
                prep.next = PreparedCones(nxt, nstore, nstore.gen)
            else:
                prep.next = follow
        if keys is not None and (keys.device != dev or keys.dtype != torch.int64 or not keys.is_contiguous()):
            keys = keys.to(device=dev, dtype=torch.int64).contiguous()
        # the pack status of THIS batch (its store may be packed again by a later launch: keep the verdict now, in stream order)
        bad = (prep.store.pack_status == ST_BAD_INPUT) if prep.sparse else None
        _launch_step(prep.store, pred, B, mode, sign, inner_ratio, max_iter, out, status, iters, nxt, nstore,
                     zero_failed=zero_failed, warm=warm, keys=keys)
        if bad is not None:
            # an instance the sparse loader rejected left slot state -1, which the solve reports as TOO_LARGE: its own
            # verdict is the loader's (as cone_op_sparse)
            status = out["status"] = torch.where(bad, torch.full_like(status, ST_BAD_INPUT), status)
        if zero_failed:
            out["zero_failed"] = True  # (the kernel wrote loss 0 / gradient 0 for instances whose status is not OK)
        if check:
            if bool((status == ST_TOO_LARGE).any()):
                _step_ok[(m, d)] = False
                return general(True)
            _raise_for_status(status, "solver='hip' (prepared)", sparse=prep.sparse)
    return out


def _raise_for_status(status: torch.Tensor, what: str, sparse: bool = False, offset: int = 0) -> None:
    """`sparse`: the cones came in on the sparse wire format, whose loader reports a broken entry as ST_BAD_INPUT.
    `offset`: batch index of status[0] (a chunk of a larger batch)."""
    st = status.cpu()
    if bool((st == ST_OK).all()):
        return
    bad = int((st != ST_OK).sum())
    first = int((st != ST_OK).nonzero()[0])
    code = int(st[first])
    first += int(offset)
    if code == ST_NOT_CONVERGED:
        raise HipSolverError(f"{what}: Maximum number of iterations reached ({bad} instance(s), first index {first}).")
    if code == ST_TOO_LARGE:
        raise HipSolverError(
            f"{what}: {bad} cone(s) (first index {first}) did not fit the workspace of the large-cone path "
            "after four 4x size increases (non-zeros / band of the reduced system).")
    if code == ST_BAD_INPUT and sparse:
        raise ValueError(f"{what}: malformed sparse cone: unsorted / out-of-range / zero or non-finite entry (or "
                         f"non-finite input) in {bad} instance(s), first index {first}.")
    if code == ST_BAD_INPUT:
        raise ValueError(f"{what}: non-finite input in {bad} instance(s), first index {first}.")
    raise HipSolverError(f"{what}: unknown status {code}")


def _device_and_pred(cones, pred_cost, B: int, d: int, mode: int):
    """What a general operator call starts with: the device it runs on (the cones', else the prediction's, else the
    current one) and the validated prediction there (None: MODE_AVG only)."""
    dev = cones.device if cones.is_cuda else (
        pred_cost.device if pred_cost is not None and pred_cost.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    if pred_cost is not None:
        if pred_cost.shape != (B, d):
            raise ValueError(f"pred_cost must have shape ({B}, {d}), got {tuple(pred_cost.shape)}")
        return dev, _as_device(pred_cost, dev)
    if mode != MODE_AVG:
        raise ValueError("pred_cost is required")
    return dev, None


def _launch_packed(store_ref, ids, pred, B, mode, sign, inner_ratio, max_iter, lds, waves, out, status, iters,
                   what="cave_hip_cone_packed"):
    """cave_hip_cone_packed on a store: slots `ids`, or slots [0, B) of a slot store (ids None)."""
    rc = _lib.load_library().cave_hip_cone_packed(
        store_ref, _lib.ptr(ids), _lib.ptr(pred), B, int(mode), float(sign), float(inner_ratio), int(max_iter), lds, waves,
        *_out_ptrs(out, status, iters), _lib.current_stream())
    _lib.check(rc, what)


def cone_op_dense(tight_ctrs: torch.Tensor, pred_cost: torch.Tensor | None, mode: int, sign: float = 1.0,
                  inner_ratio: float = 0.2, *, max_iter: int = 0, nnz_cap: int = 0, lds_bytes: int = 0,
                  waves: int = 0, check: bool = True, outputs: tuple[str, ...] = ("proj", "rnorm")) -> dict[str, torch.Tensor]:
    """Run the fused per-instance kernel on the reference's dense wire format.

    tight_ctrs (B, m_max, d) float32 zero-padded (src/dataset.py:143); pred_cost (B, d).
    ``outputs`` selects which of proj / rnorm / target / loss / grad are materialised.
    ``waves``: wavefronts cooperating per instance (0 = chosen from the batch size and what is known
    about the shape, see ``_auto_waves``; 1 or 2: reduced systems up to 64 rows; 4: up to 32 rows).
    With ``check=True`` (default) the per-instance status is read back (one host sync):
    a batch with a cone that does not fit is retried with one wave per instance and the largest
    LDS arena, then on the large-cone path (global workspace, band Newton systems: TSP-100,
    30x30 grids); the tier that worked is remembered per (m_max, d).  Anything else raises.
    """
    lib = _lib.load()
    if tight_ctrs.dim() != 3:
        raise ValueError("tight_ctrs must have shape (B, m_max, d)")
    B, m, d = tight_ctrs.shape
    dev, pred = _device_and_pred(tight_ctrs, pred_cost, B, d, mode)
    ctrs = _as_device(tight_ctrs, dev)
    with torch.cuda.device(dev):
        out, status, iters = _alloc_out(outputs, B, d, dev)
        if B == 0:
            return out

        def launch(cap: int, lds: int, nw: int) -> None:
            rc = lib.cave_hip_cone_dense(
                _lib.ptr(ctrs), _lib.ptr(pred), B, m, d, int(mode), float(sign), float(inner_ratio),
                int(max_iter), int(cap), int(lds), int(nw),
                *_out_ptrs(out, status, iters), _lib.current_stream())
            _lib.check(rc, "cave_hip_cone_dense")

        # LDS of the large path's hot arrays (band window + staging).  The band is only known inside the
        # kernel: wide cost vectors go with dense reduced systems (TSP: ~sqrt(2d) rows, window ~16 d bytes)
        large_lds = _lib.MAX_LDS if d >= 4096 else 64 * 1024

        def launch_large(cap: int, band: int) -> None:
            slice_bytes = int(lib.cave_hip_large_slice_bytes(m, d, cap, band))
            if slice_bytes <= 0 or slice_bytes >= 1 << 32:
                raise HipSolverError(f"solver='hip': a cone of this size needs a {slice_bytes}-byte workspace slice "
                                     "(limit 4 GiB)")
            slots = _lib.large_slots(dev, B, slice_bytes)
            ws = _lib.workspace(dev, slots * slice_bytes)
            rc = lib.cave_hip_cone_dense_large(
                _lib.ptr(ctrs), _lib.ptr(pred), B, m, d, int(mode), float(sign), float(inner_ratio),
                int(max_iter), int(cap), large_lds, _lib.ptr(ws), slice_bytes, slots,
                *_out_ptrs(out, status, iters), _lib.current_stream())
            _lib.check(rc, "cave_hip_cone_dense_large")

        def run_large() -> None:
            cap, band = _large_hint.get((m, d), _large_guess(m, d))
            cap = max(cap, nnz_cap)
            for attempt in range(5):
                launch_large(cap, band)
                if not check or not bool((status == ST_TOO_LARGE).any()):
                    break
                cap, band = min(4 * cap, max(m * d, 64)), 4 * band  # dense cones: m*d non-zeros, p*p band entries
            _large_hint[(m, d)] = (cap, band)

        auto = lds_bytes == 0

        def launch_split() -> None:
            ss = _slot_store(dev, B, d)
            rc = lib.cave_hip_pack_fill(_lib.ptr(ctrs), B, m, d, int(nnz_cap), 0, 4, ss.ref, 0, _lib.ptr(ss.pack_status),
                                        _lib.current_stream())
            _lib.check(rc, "cave_hip_pack_fill (slot mode)")
            _launch_packed(ss.ref, None, pred, B, mode, sign, inner_ratio, max_iter, ss.lds_bytes, 1, out, status, iters,
                           "cave_hip_cone_packed (slot mode)")

        # small cones: the split form, once a checked batch of this shape has fitted it (or when this call is checked)
        if auto and waves == 0 and 0 < m and d <= SPLIT_MAX_D and B <= 2048 and (m, d) not in _tier:
            ok = _split_ok.get((m, d))
            if ok is True or (ok is None and check):
                launch_split()
                if not check:
                    return out
                fits = not bool((status == ST_TOO_LARGE).any())
                _split_ok[(m, d)] = fits
                if fits:
                    _raise_for_status(status, "solver='hip'")
                    _settled.add((m, d))
                    return out
        if auto and (m, d) not in _tier and fast_path_cannot_fit(d):
            _tier[(m, d)] = 2
        tier = _tier.get((m, d), 0) if auto else 0
        if m > 65535:
            raise HipSolverError("solver='hip': more than 65535 rows per instance are not supported")
        if tier == 2:
            run_large()
        elif tier == 1:
            cap, lds = _grow_limits(m, d)
            launch(max(cap, nnz_cap), lds, 8)  # full arena = one workgroup per CU: four waves with the wide register budget
        else:
            nw = waves if (waves != 0 or not auto) else _auto_waves(B, m, d, check)
            launch(nnz_cap, lds_bytes, nw)
            if check and auto and waves == 0 and nw == 4:
                fits = not bool((status == ST_TOO_LARGE).any())
                _wide_ok[(m, d)] = fits
                if not fits:
                    launch(nnz_cap, lds_bytes, 2)  # more than 32 reduced rows: two waves hold up to 64
        if check:
            if auto and tier == 0 and bool((status == ST_TOO_LARGE).any()):
                tier = _tier[(m, d)] = 1
                cap, lds = _grow_limits(m, d)
                launch(max(cap, nnz_cap), lds, 8)  # full arena = one workgroup per CU: four waves with the wide register budget
            if auto and tier == 1 and bool((status == ST_TOO_LARGE).any()):
                tier = _tier[(m, d)] = 2
                run_large()
            _raise_for_status(status, "solver='hip'")
            if auto:
                _settled.add((m, d))
    return out


def project_hip(tight_ctrs: torch.Tensor, signed_cost: torch.Tensor, max_iter: int = 0, nnz_cap: int = 0,
                lds_bytes: int = 0, waves: int = 0, check: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """(proj, rnorm) on signed_cost's device and dtype — `_batch_project(..., 'nnls')` (src/cave.py:231-264).

    ``max_iter`` caps the Newton iterations of the GPU solver (0 = default 100); unlike
    Clarabel's ``max_iter`` it does not produce an interior iterate (src/cave.py:302).
    """
    o = cone_op_dense(tight_ctrs, signed_cost, MODE_PROJECT, 1.0, 0.0, max_iter=max_iter, nnz_cap=nnz_cap,
                      lds_bytes=lds_bytes, waves=waves, check=check, outputs=("proj", "rnorm"))
    device, dtype = signed_cost.device, signed_cost.dtype
    return o["proj"].to(device=device, dtype=dtype), o["rnorm"].to(device=device, dtype=dtype)


def cone_op_sparse(cones, pred_cost: torch.Tensor | None, mode: int, sign: float = 1.0, inner_ratio: float = 0.2, *,
                   max_iter: int = 0, check: bool = True, outputs: tuple[str, ...] = ("proj", "rnorm")) -> dict[str, torch.Tensor]:
    """cone_op_dense for a batch on the sparse wire format (cave_amd.sparse.SparseCones): no dense tensor anywhere.

    Shapes the split form takes (d <= SPLIT_MAX_D, B <= 2048): cave_hip_pack_fill_sparse in slot mode, four waves per
    instance, in place of the dense pack launch -- it copies 8 bytes per non-zero instead of streaming the zeros --
    followed by the same one-wave cave_hip_cone_packed as the dense split form, so the outputs are the dense call's
    bit for bit.  Anything else, and a split batch that reports CAVE_ST_TOO_LARGE under ``check=True``, builds a
    transient ConeStore.from_sparse and runs its cone_op on every slot.

    A malformed instance (unsorted or repeated key, row / column out of range, zero or non-finite value) is rejected
    on the device: ``check=True`` raises ValueError naming the first one; ``check=False`` leaves status
    CAVE_ST_BAD_INPUT and NaN outputs at its index and the other instances correct."""
    lib = _lib.load()
    if not isinstance(cones, SparseCones):
        raise TypeError("cone_op_sparse: cones must be a SparseCones")
    B, m, d = _shape(cones)
    dev, pred = _device_and_pred(cones, pred_cost, B, d, mode)
    x = cones.to(dev)
    what = "solver='hip' (sparse cones)"
    with torch.cuda.device(dev):
        if B == 0:
            return _alloc_out(outputs, 0, d, dev)[0]
        if 0 < m and d <= SPLIT_MAX_D and B <= 2048 and _sparse_split_ok.get((m, d)) is not False:
            out, status, iters = _alloc_out(outputs, B, d, dev)
            ss = _slot_store(dev, B, d)
            rc = lib.cave_hip_pack_fill_sparse(x.c_ref(), 0, 0, 4, ss.ref, 0, _lib.ptr(ss.pack_status), _lib.current_stream())
            _lib.check(rc, "cave_hip_pack_fill_sparse (slot mode)")
            _launch_packed(ss.ref, None, pred, B, mode, sign, inner_ratio, max_iter, ss.lds_bytes, 1, out, status, iters,
                           "cave_hip_cone_packed (slot mode)")
            # an instance the loader rejected left an empty slot, which the solve reports as TOO_LARGE (NaN outputs):
            # its own verdict is the loader's
            status = out["status"] = torch.where(ss.pack_status == ST_BAD_INPUT, ss.pack_status, status)
            if not check:
                return out
            st = status.cpu()
            if not bool((st == ST_TOO_LARGE).any()):
                _sparse_split_ok[(m, d)] = True
                _raise_for_status(st, what, sparse=True)
                return out
            _sparse_split_ok[(m, d)] = False
        from .dataset import ConeStore

        store = ConeStore.from_sparse(x, strict=check)
        out = store.cone_op(torch.arange(B, dtype=torch.int64, device=dev), pred, mode, sign, inner_ratio, max_iter=max_iter,
                            check=check, outputs=outputs)
        bad = store.bad_input
        if bad is not None:  # (check=False only: the store holds an empty cone in a rejected instance's slot)
            out["status"] = torch.where(bad, torch.full_like(out["status"], ST_BAD_INPUT), out["status"])
            for name in outputs:
                o = out[name]
                o.masked_fill_(bad if o.dim() == 1 else bad.unsqueeze(1), float("nan"))
    return out


def project_hip_sparse(cones, signed_cost: torch.Tensor, max_iter: int = 0, check: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """project_hip for a SparseCones batch: (proj, rnorm) on signed_cost's device and dtype."""
    o = cone_op_sparse(cones, signed_cost, MODE_PROJECT, 1.0, 0.0, max_iter=max_iter, check=check, outputs=("proj", "rnorm"))
    device, dtype = signed_cost.device, signed_cost.dtype
    return o["proj"].to(device=device, dtype=dtype), o["rnorm"].to(device=device, dtype=dtype)


# ---- the APGD projector (cave_hip_cone_apgd / cave_hip_cone_apgd_sparse, cave_amd/csrc/apgd.h): the reference's
# `project_apgd` (src/qpsolver.py:11-110) restated on the device.  It iterates on the rows of the wire format as they are
# (pairs, unit rows, repeated rows, padding), so it reads the two wire formats themselves and never a store.
APGD_MAX_ITERS = 10_000  # the reference's cap when max_iters is None (src/qpsolver.py:23)
_apgd_cap: dict[tuple[int, int], int] = {}  # (m_max, d) -> the entry capacity a checked dense call settled


_apgd_full: dict[tuple[int, int], int] = {}


def apgd_full_cap(m: int, d: int) -> int:
    """The largest entry capacity whose arena fits the 160 KiB of LDS at this shape (0: none does); found once per shape."""
    key = (int(m), int(d))
    if key not in _apgd_full:
        _apgd_full[key] = _apgd_full_cap_search(*key)
    return _apgd_full[key]


def _apgd_full_cap_search(m: int, d: int) -> int:
    lib = _lib.load_library()
    hi = min(m * d, _lib.MAX_LDS // 14)
    if hi < 1 or lib.cave_hip_apgd_lds_bytes(m, d, 1) < 0:
        return 0
    lo = 1  # (fits)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lib.cave_hip_apgd_lds_bytes(m, d, mid) > 0:
            lo = mid
        else:
            hi = mid - 1
    return lo


def _apgd_limit_error(m: int, d: int, cap: int) -> "HipSolverError":
    return HipSolverError(f"solver='hip' (apgd): an instance with more than {cap} non-zeros does not fit the 160 KiB LDS arena "
                          f"of the APGD kernel at m_max = {m}, d = {d} (28 m_max + 20 d + 14 nnz bytes).")


def _apgd_launch(cones, pred, B, m, d, mode, sign, k_start, n_iter, power_iter, cap, state, want_pgrad, outputs, dev):
    lib = _lib.load()
    out, status, iters = _alloc_out(outputs, B, d, dev)
    if state is None and k_start == 0:
        state = (torch.empty(B, m, dtype=torch.float64, device=dev), torch.empty(B, m, dtype=torch.float64, device=dev),
                 torch.empty(B, dtype=torch.float64, device=dev))
    out["state"] = state
    pgrad = out["pgrad"] = torch.empty(B, dtype=torch.float64, device=dev) if want_pgrad else None
    ptr = _lib.ptr
    tail = (int(mode), float(sign), int(k_start), int(n_iter), int(power_iter), int(cap), *(ptr(t) for t in (state or (None,) * 3)),
            *_out_ptrs(out, status, iters), ptr(pgrad), _lib.current_stream())
    if isinstance(cones, SparseCones):
        rc, what = lib.cave_hip_cone_apgd_sparse(cones.c_ref(), ptr(pred), *tail), "cave_hip_cone_apgd_sparse"
    else:
        rc, what = lib.cave_hip_cone_apgd(ptr(cones), ptr(pred), B, m, d, *tail), "cave_hip_cone_apgd"
    _lib.check(rc, what)
    return out


def _apgd_empty(outputs, m: int, d: int, dev, want_pgrad: bool) -> dict:
    """What a launch returns for an empty batch (the C ABI answers B == 0 with CAVE_OK and touches nothing)."""
    out = _alloc_out(outputs, 0, d, dev)[0]
    out["state"] = (torch.empty(0, m, dtype=torch.float64, device=dev), torch.empty(0, m, dtype=torch.float64, device=dev),
                    torch.empty(0, dtype=torch.float64, device=dev))
    out["pgrad"] = torch.empty(0, dtype=torch.float64, device=dev) if want_pgrad else None
    return out


def _apgd_state_ok(state, B: int, m: int, dev) -> None:
    if state is None:
        return
    xc, xp, st = state
    for t, shape in ((xc, (B, m)), (xp, (B, m)), (st, (B,))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"state: need contiguous float64 tensors x_curr ({B}, {m}), x_prev ({B}, {m}), step ({B},) on {dev}")


def cone_op_apgd(tight_ctrs: torch.Tensor, pred_cost: torch.Tensor, mode: int = MODE_PROJECT, sign: float = 1.0, *,
                 n_iter: int = 200, k_start: int = 0, power_iter: int = 8, nnz_cap: int = 0, state=None, pgrad: bool = False,
                 check: bool = True, outputs: tuple[str, ...] = ("proj", "rnorm")) -> dict:
    """`n_iter` APGD iterations per instance on the dense wire format (cave_hip_cone_apgd), numbered from `k_start`.

    -> the outputs asked for (proj / rnorm un-squared / target / loss / grad; mode MODE_PROJECT or MODE_EXACT) plus
    "status", "iters", "state" = (x_curr [B, m_max], x_prev, step [B]) in float64 and, with ``pgrad=True``, "pgrad" [B],
    the reference's convergence quantity.  ``k_start > 0`` continues from ``state`` (the tensors of the launch before,
    updated in place).  ``nnz_cap`` = 0: the capacity settled for this (m_max, d) -- a guess at first; under
    ``check=True`` a batch with an instance beyond it is retried once with the largest capacity the LDS holds, and what
    worked is remembered.  ``check=True`` reads the status back (one host sync) and raises like cone_op_dense;
    ``check=False`` leaves CAVE_ST_TOO_LARGE / CAVE_ST_BAD_INPUT in "status" and NaN in that instance's outputs."""
    _lib.load()
    if not isinstance(tight_ctrs, torch.Tensor) or tight_ctrs.dim() != 3:
        raise ValueError("tight_ctrs must have shape (B, m_max, d)")
    B, m, d = tight_ctrs.shape
    dev, pred = _device_and_pred(tight_ctrs, pred_cost, B, d, mode)
    ctrs = _as_device(tight_ctrs, dev)
    with torch.cuda.device(dev):
        if B == 0:
            return _apgd_empty(outputs, m, d, dev, pgrad)
        _apgd_state_ok(state, B, m, dev)
        full = apgd_full_cap(m, d)
        if full < 1:
            raise _apgd_limit_error(m, d, 0)
        auto = nnz_cap <= 0
        cap = min(full, _apgd_cap.get((m, d), min(m * d, 3 * (m + d) + 64))) if auto else int(nnz_cap)
        args = (ctrs, pred, B, m, d, mode, sign, k_start, n_iter, power_iter)
        out = _apgd_launch(*args, cap, state, pgrad, outputs, dev)
        if check:
            if auto and cap < full and k_start == 0 and bool((out["status"] == ST_TOO_LARGE).any()):
                cap = full
                out = _apgd_launch(*args, cap, state, pgrad, outputs, dev)
            if bool((out["status"] == ST_TOO_LARGE).any()):
                raise _apgd_limit_error(m, d, cap)
            _raise_for_status(out["status"], "solver='hip' (apgd)")
            if auto:
                _apgd_cap[(m, d)] = cap
    return out


def cone_op_apgd_sparse(cones, pred_cost: torch.Tensor, mode: int = MODE_PROJECT, sign: float = 1.0, *, n_iter: int = 200,
                        k_start: int = 0, power_iter: int = 8, nnz_cap: int = 0, state=None, pgrad: bool = False,
                        check: bool = True, outputs: tuple[str, ...] = ("proj", "rnorm")) -> dict:
    """cone_op_apgd for a batch on the sparse wire format (cave_hip_cone_apgd_sparse): the same bits as the dense call on
    the densified batch.  ``nnz_cap`` = 0: the entries of the largest instance (read from the offsets once per batch
    object), at most what the LDS holds.  A malformed instance is rejected on the device (CAVE_ST_BAD_INPUT)."""
    _lib.load()
    if not isinstance(cones, SparseCones):
        raise TypeError("cone_op_apgd_sparse: cones must be a SparseCones")
    B, m, d = _shape(cones)
    dev, pred = _device_and_pred(cones, pred_cost, B, d, mode)
    x = cones.to(dev)
    with torch.cuda.device(dev):
        if B == 0:
            return _apgd_empty(outputs, m, d, dev, pgrad)
        _apgd_state_ok(state, B, m, dev)
        full = apgd_full_cap(m, d) if m > 0 else 0
        if full < 1:
            raise _apgd_limit_error(m, d, 0)
        if nnz_cap <= 0:
            big = getattr(cones, "_max_nnz", None)
            if big is None:
                big = cones._max_nnz = int(cones.nnz_per_instance.max()) if B else 0
            nnz_cap = min(full, max(big, 1))
        out = _apgd_launch(x, pred, B, m, d, mode, sign, k_start, n_iter, power_iter, int(nnz_cap), state, pgrad, outputs, dev)
        if check:
            if bool((out["status"] == ST_TOO_LARGE).any()):
                raise _apgd_limit_error(m, d, int(nnz_cap))
            _raise_for_status(out["status"], "solver='hip' (apgd, sparse cones)", sparse=True)
    return out


def _apgd_chunks(cones, pred, mode, sign, max_iters, tol_grad, check_frequency, power_iter, check, outputs):
    """The reference's outer loop (src/qpsolver.py:39-58): chunks of `check_frequency` iterations through the
    continuation state; with `tol_grad` the check quantity is read on the host once per chunk and the loop stops at the
    first chunk whose batch maximum is <= tol_grad.  -> (outputs of the last launch, chunks run, the maxima read).
    `check` applies to the first chunk, whose status is every chunk's (the cones and the prediction do not change); an
    empty batch runs no chunk."""
    op = cone_op_apgd_sparse if isinstance(cones, SparseCones) else cone_op_apgd
    if _shape(cones)[0] == 0:
        return op(cones, pred, mode, sign, n_iter=0, pgrad=tol_grad is not None, check=check, outputs=outputs), 0, []
    cap = APGD_MAX_ITERS if max_iters is None else int(max_iters)
    K = int(check_frequency)
    if K < 1:
        raise ValueError("check_frequency must be positive")
    out, state, seen, chunks = None, None, [], 0
    starts = list(range(0, cap, K)) or [0]
    for k_start in starts:
        n = max(0, min(K, cap - k_start))
        last = k_start == starts[-1]
        # only the last launch needs the outputs; with tol_grad any launch may be the last
        o = op(cones, pred, mode, sign, n_iter=n, k_start=k_start, power_iter=power_iter, state=state, pgrad=tol_grad is not None,
               check=check if k_start == 0 else False, outputs=outputs if (last or tol_grad is not None) else ())
        out, state, chunks = o, o["state"], chunks + 1
        if tol_grad is not None:
            pg = o["pgrad"]
            worst = float(pg[~torch.isnan(pg)].max()) if bool((~torch.isnan(pg)).any()) else 0.0
            seen.append(worst)
            if worst <= tol_grad:
                break
    return out, chunks, seen


def project_apgd_hip(tight_ctrs, signed_cost: torch.Tensor, tol_grad: float | None = 1e-4, max_iters: int | None = None,
                     check_frequency: int = 200, power_iter: int = 8, *, check: bool = True,
                     info: dict | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """The reference's `project_apgd` (src/qpsolver.py:11-63), signature and return values: (proj (B, d), rnorm (B,)) with
    rnorm the SQUARED residual, on signed_cost's device and dtype.  `tight_ctrs`: a dense tensor or a SparseCones.  The
    stopping rule is the reference's, batch-global.  With ``tol_grad=None`` there is one launch per chunk and no host read
    between the chunks; ``check=True`` (the default, beyond the reference's signature) still reads the status of the FIRST
    chunk back -- on the dense route that is also where the entry capacity of a new shape settles, possibly with one
    relaunch -- and raises for an instance that failed.  ``check=False`` makes no host read at all: a failed instance
    then holds NaN, and a dense shape runs with the capacity it has settled or the first guess.  `info` (a dict) receives
    "chunks", the chunks run, and "pgrad", the check quantity read after each."""
    out, chunks, seen = _apgd_chunks(tight_ctrs, signed_cost, MODE_PROJECT, 1.0, max_iters, tol_grad, check_frequency, power_iter,
                                     check, ("proj", "rnorm"))
    if info is not None:
        info["chunks"], info["pgrad"] = chunks, seen
    device, dtype = signed_cost.device, signed_cost.dtype
    rn = out["rnorm"].to(torch.float64)
    return out["proj"].to(device=device, dtype=dtype), (rn * rn).to(device=device, dtype=dtype)


def average_ctrs_hip(tight_ctrs: torch.Tensor) -> torch.Tensor:
    """`_average_ctrs` (src/cave.py:222-228) in one streaming pass."""
    o = cone_op_dense(tight_ctrs, None, MODE_AVG, outputs=("target",))
    return o["target"].to(device=tight_ctrs.device, dtype=tight_ctrs.dtype)
