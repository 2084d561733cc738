"""CPU tier, no compute: what the twenty cone entry points of include/cave_hip.h refuse, in which order, with which
return code and which full cave_hip_last_error() text -- every check runs before any launch, so none of this needs a
GPU.  Per entry: CHECKS lists its checks in the order the entry makes them, each with a call (the entry's good arguments
plus the overrides shown) in which exactly that check is the first to fail; every adjacent pair is called once more
with both violated and must report the earlier one.  EXTRA holds further calls per check and the early returns
(B == 0, B == 0 and B_next == 0, src->n == 0, a sparse step without a next batch taking the dense path).  An entry
that sets no message (the size queries) and every call that succeeds must leave the last error as it was."""

import ctypes as C

import numpy as np
import pytest

from cave_amd import _lib

KEEP = []   # the host arrays behind every struct of the tables
SENTINEL = "default_limits: bad shape"


def _addr(n, dtype=np.uint8, off=0):
    """address of a 16-byte aligned host array of n elements (+ off bytes): nothing below is ever read or launched on"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 32, np.uint8)
    KEEP.append(raw)
    return raw.ctypes.data + (-raw.ctypes.data) % 16 + off


def store(n=4, d=10, **kw):
    return _lib.Store(n=n, d=d, reserved=0, **kw)


def lite(n=4, d=10, **kw):
    f = {"hdr": _addr(n * 8, np.int32), "usign": _addr(n * d), "avg": _addr(n * d, np.float32), "rowptr": _addr(n * 33, np.int32),
         "ell": _addr(n * 4 * d, np.int32), "csr16": _addr(n * 768, np.int32), "rl": _addr(n * 32)}
    f.update(kw)
    return _lib.LiteStore(n=n, d=d, reserved=0, **f)


def cones(B=4, m=15, d=10, **kw):
    f = {"ent_off": _addr(8, np.int64), "key": _addr(8, np.uint32), "val": _addr(8, np.float32)}
    f.update(kw)
    return _lib.SparseConesC(B=B, m_max=m, d=d, **f)


def warm(n=8, **kw):
    f = {"key": _addr(8, np.uint64), "theta": _addr(8 * 32, np.float32)}
    f.update(kw)
    return _lib.WarmCacheC(n_entries=n, **f)


CTRS, PRED, WS, TICKETS, NROWS, NNNZ = _addr(64, np.float32), _addr(64, np.float32), _addr(4096), _addr(4096, np.uint32), _addr(4, np.int32), _addr(4, np.int32)
SOLVE, NEXT, STORE = lite(), lite(), store()
HALF = store(n_rows=NROWS)                      # n_rows without n_nnz
NULLS = dict(ent_off=0, key=0, val=0)
BIG_LDS = 160 * 1024 + 1
OUT7 = ["proj", "rnorm", "target", "loss", "grad", "status", "iters"]
NO_OUT = {k: None for k in OUT7}
WSMSG = "bad workspace (16-byte aligned, 1 KiB <= slice_bytes < 4 GiB, multiple of 8, n_slots > 0)"
STOREMSG = "(size, d, null or unaligned array)"

# entry -> (parameter names in the header's order, good arguments)
ENTRIES = {
    "default_limits": (["m_max", "d", "nnz_cap", "lds_bytes"], dict(m_max=15, d=10, nnz_cap=None, lds_bytes=None)),
    "cone_dense": (["ctrs", "pred", "B", "m_max", "d", "mode", "sign", "inner_ratio", "max_iter", "nnz_cap", "lds_bytes", "waves", *OUT7, "stream"],
                   dict(ctrs=CTRS, pred=PRED, B=4, m_max=15, d=10, mode=0, sign=1.0, inner_ratio=0.2, max_iter=0, nnz_cap=0, lds_bytes=0, waves=0, **NO_OUT, stream=None)),
    "pack_count": (["ctrs", "B", "m_max", "d", "nnz_cap", "lds_bytes", "waves", "n_rows", "n_nnz", "status", "stream"],
                   dict(ctrs=CTRS, B=4, m_max=15, d=10, nnz_cap=0, lds_bytes=0, waves=0, n_rows=NROWS, n_nnz=NNNZ, status=None, stream=None)),
    "pack_fill": (["ctrs", "B", "m_max", "d", "nnz_cap", "lds_bytes", "waves", "store", "slot0", "status", "stream"],
                  dict(ctrs=CTRS, B=4, m_max=15, d=10, nnz_cap=0, lds_bytes=0, waves=0, store=STORE, slot0=0, status=None, stream=None)),
    "packed_lds_bytes": (["d", "max_rows", "max_nnz", "all_pm1"], dict(d=190, max_rows=26, max_nnz=700, all_pm1=1)),
    "cone_packed": (["store", "ids", "pred", "B", "mode", "sign", "inner_ratio", "max_iter", "lds_bytes", "waves", *OUT7, "stream"],
                    dict(store=STORE, ids=None, pred=PRED, B=4, mode=0, sign=1.0, inner_ratio=0.2, max_iter=0, lds_bytes=4096, waves=0, **NO_OUT, stream=None)),
    "large_slice_bytes": (["m_max", "d", "nnz_cap", "band_entries"], dict(m_max=15, d=10, nnz_cap=64, band_entries=16)),
    "packed_large_slice_bytes": (["d", "max_rows", "band_entries"], dict(d=10, max_rows=15, band_entries=16)),
    "packed_large_lds_bytes": (["max_rows", "max_bw"], dict(max_rows=15, max_bw=4)),
    "packed_large_rb_bytes": (["max_rows"], dict(max_rows=15)),
    "cone_dense_large": (["ctrs", "pred", "B", "m_max", "d", "mode", "sign", "inner_ratio", "max_iter", "nnz_cap", "lds_bytes", "workspace", "slice_bytes", "n_slots", *OUT7, "stream"],
                         dict(ctrs=CTRS, pred=PRED, B=4, m_max=15, d=10, mode=0, sign=1.0, inner_ratio=0.2, max_iter=0, nnz_cap=64, lds_bytes=0, workspace=WS, slice_bytes=1024, n_slots=1, **NO_OUT, stream=None)),
    "pack_large": (["ctrs", "B", "m_max", "d", "nnz_cap", "workspace", "slice_bytes", "n_slots", "n_rows", "n_nnz", "store", "slot0", "status", "stream"],
                   dict(ctrs=CTRS, B=4, m_max=15, d=10, nnz_cap=64, workspace=WS, slice_bytes=1024, n_slots=1, n_rows=NROWS, n_nnz=NNNZ, store=None, slot0=0, status=None, stream=None)),
    "cone_packed_large": (["store", "ids", "pred", "B", "mode", "sign", "inner_ratio", "max_iter", "lds_bytes", "waves", "workspace", "slice_bytes", "n_slots", *OUT7, "stream"],
                          dict(store=STORE, ids=None, pred=PRED, B=4, mode=0, sign=1.0, inner_ratio=0.2, max_iter=0, lds_bytes=0, waves=0, workspace=WS, slice_bytes=1024, n_slots=1, **NO_OUT, stream=None)),
    "pack_count_sparse": (["cones", "nnz_cap", "lds_bytes", "waves", "n_rows", "n_nnz", "status", "stream"],
                          dict(cones=cones(), nnz_cap=0, lds_bytes=0, waves=0, n_rows=NROWS, n_nnz=NNNZ, status=None, stream=None)),
    "pack_fill_sparse": (["cones", "nnz_cap", "lds_bytes", "waves", "store", "slot0", "status", "stream"],
                         dict(cones=cones(), nnz_cap=0, lds_bytes=0, waves=0, store=STORE, slot0=0, status=None, stream=None)),
    "pack_large_sparse": (["cones", "nnz_cap", "workspace", "slice_bytes", "n_slots", "n_rows", "n_nnz", "store", "slot0", "status", "stream"],
                          dict(cones=cones(), nnz_cap=64, workspace=WS, slice_bytes=1024, n_slots=1, n_rows=NROWS, n_nnz=NNNZ, store=None, slot0=0, status=None, stream=None)),
    "step_lds_bytes": (["m_max", "d"], dict(m_max=15, d=10)),
    "lite_from_packed": (["src", "dst", "status", "stream"], dict(src=STORE, dst=SOLVE, status=None, stream=None)),
}
_SOLVE = ["solve", "ids", "pred", "B", "mode", "sign", "inner_ratio", "max_iter", "flags", *OUT7]
_SOLVE_IPM = [n for n in _SOLVE if n not in ("mode", "inner_ratio")]
_DENSE_NEXT = ["next_ctrs", "B_next", "m_max", "d", "next", "pack_status"]
_SPARSE_NEXT = ["next_cones", "next", "pack_status"]
_WARM = ["warm", "keys", "warm_hit"]
_STEP = dict(solve=SOLVE, ids=None, pred=PRED, B=4, mode=0, sign=1.0, inner_ratio=0.2, max_iter=0, flags=0, **NO_OUT, next_ctrs=CTRS, B_next=4,
             m_max=15, d=10, next_cones=cones(), next=NEXT, pack_status=None, warm=None, keys=None, warm_hit=None, cu_tickets=TICKETS, stream=None)
ENTRIES["cone_step"] = (_SOLVE + _DENSE_NEXT + ["cu_tickets", "stream"], _STEP)
ENTRIES["cone_step_warm"] = (_SOLVE + _DENSE_NEXT + _WARM + ["cu_tickets", "stream"], dict(_STEP, warm=warm()))
ENTRIES["cone_step_sparse"] = (_SOLVE + _SPARSE_NEXT + _WARM + ["cu_tickets", "stream"], _STEP)
ENTRIES["cone_step_ipm"] = (_SOLVE_IPM + _DENSE_NEXT + ["cu_tickets", "stream"], _STEP)
ENTRIES["cone_step_sparse_ipm"] = (_SOLVE_IPM + _SPARSE_NEXT + ["cu_tickets", "stream"], _STEP)


def _named(who, rows):
    return [(over, f"{who}: {what}") for over, what in rows]


def _warm_checks(who):
    return _named(who, [(dict(warm=warm(6)), "n_entries must be a power of two"),
                        (dict(warm=warm(key=0)), "null key / theta array"),
                        (dict(warm=warm(theta=_addr(8 * 32, np.float32, off=4))), "theta must be 16-byte aligned")])


def _dense_step_checks(mode=True):
    rows = [(dict(B=-1), "bad batch sizes"), (dict(d=0), "need 0 < d <= 256"), (dict(cu_tickets=None), "cu_tickets is null"),
            (dict(mode=5), "bad mode (PROJECT .. AVG)"), (dict(pred=None), "pred is null"), (dict(solve=None), "bad solve store " + STOREMSG),
            (dict(m_max=40000), "shape does not qualify (cave_hip_step_lds_bytes)"), (dict(m_max=0), "bad m_max"),
            (dict(next_ctrs=None), "next_ctrs is null"), (dict(next=None), "bad next store " + STOREMSG),
            (dict(next=SOLVE), "solve and next must be different stores")]
    return _named("cone_step", [r for r in rows if mode or "mode" not in r[0]])


def _sparse_step_checks(mode=True, warm_too=True):
    who = "cone_step_sparse"
    rows = [(dict(next_cones=cones(m=-1)), "bad batch (need 0 <= m_max <= 65535, 0 < d <= 65535)"),
            (dict(next_cones=cones(**NULLS)), "null or misaligned ent_off / key / val"), (dict(B=-1), "bad batch sizes"),
            (dict(cu_tickets=None), "cu_tickets is null"), (dict(next_cones=cones(m=40000)), "shape does not qualify (cave_hip_step_lds_bytes)"),
            (dict(next=None), "next store is null"), (dict(next=lite(d=11)), "d of the batch differs from the store's d"),
            (dict(next=lite(n=3)), "bad next store " + STOREMSG), (dict(mode=5), "bad mode (PROJECT .. AVG)"), (dict(pred=None), "pred is null"),
            (dict(solve=None), "bad solve store " + STOREMSG), (dict(next=SOLVE), "solve and next must be different stores")]
    return (_warm_checks(who) if warm_too else []) + _named(who, [r for r in rows if mode or "mode" not in r[0]])


def _sparse_batch_checks(who):
    return _named(who, [(dict(cones=None), "bad batch (need 0 <= m_max <= 65535, 0 < d <= 65535)"),
                        (dict(cones=cones(**NULLS)), "null or misaligned ent_off / key / val")])


# entry -> [(overrides, full message)] in the order the entry checks
CHECKS = {
    "default_limits": _named("default_limits", [(dict(m_max=-1), "bad shape")]),
    "cone_dense": _named("cone_dense", [
        (dict(B=-1), "bad shape (need 0 < d <= 65535)"), (dict(m_max=1 << 17, d=1 << 15), "m_max*d must be < 2^32"), (dict(mode=6), "bad mode"),
        (dict(ctrs=None), "ctrs is null"), (dict(pred=None), "pred is null"), (dict(waves=3), "waves must be 0, 1, 2, 4 or 8"),
        (dict(lds_bytes=BIG_LDS), "bad nnz_cap / lds_bytes")]),
    "pack_count": _named("pack_count", [
        (dict(B=-1), "bad shape"), (dict(ctrs=None), "null pointer"), (dict(lds_bytes=BIG_LDS), "bad limits"), (dict(waves=3), "waves must be 0, 1, 2, 4 or 8")]),
    "pack_fill": _named("pack_fill", [
        (dict(B=-1), "bad shape"), (dict(ctrs=None), "null pointer"), (dict(slot0=-1), "store mismatch"), (dict(lds_bytes=BIG_LDS), "bad limits"),
        (dict(waves=3), "waves must be 0, 1, 2, 4 or 8"), (dict(store=HALF), "n_rows and n_nnz go together")]),
    "cone_packed": _named("cone_packed", [
        (dict(store=None), "null store / bad B"), (dict(mode=6), "bad mode"), (dict(pred=None), "pred is null"), (dict(lds_bytes=0), "bad lds_bytes"),
        (dict(waves=3), "waves must be 0, 1, 2, 4 or 8")]),
    "cone_dense_large": _named("cone_dense_large", [
        (dict(B=-1), "bad shape (need m_max, d <= 65535, m_max*d < 2^32)"), (dict(mode=6), "bad mode"), (dict(ctrs=None), "ctrs is null"),
        (dict(pred=None), "pred is null"), (dict(nnz_cap=0), "bad nnz_cap"), (dict(workspace=None), WSMSG), (dict(lds_bytes=512), "bad lds_bytes")]),
    "pack_large": _named("pack_large", [
        (dict(B=-1), "bad shape"), (dict(ctrs=None), "ctrs is null"), (dict(store=None, n_rows=None), "count pass needs n_rows and n_nnz"),
        (dict(store=STORE, slot0=-1), "store mismatch"), (dict(nnz_cap=0), "bad nnz_cap"), (dict(workspace=None), WSMSG)]),
    "cone_packed_large": _named("cone_packed_large", [
        (dict(store=None), "null store / bad B"), (dict(mode=6), "bad mode"), (dict(pred=None), "pred is null"), (dict(workspace=None), WSMSG),
        (dict(lds_bytes=512), "bad lds_bytes"), (dict(waves=3), "waves must be 0, 1, 2 or 4")]),
    "pack_count_sparse": _sparse_batch_checks("pack_count_sparse") + _named("pack_count_sparse", [
        (dict(n_rows=None), "null pointer"), (dict(lds_bytes=BIG_LDS), "bad limits"), (dict(waves=1), "waves must be 0, 2, 4 or 8")]),
    "pack_fill_sparse": _sparse_batch_checks("pack_fill_sparse") + _named("pack_fill_sparse", [
        (dict(store=None), "null pointer"), (dict(slot0=-1), "store mismatch"), (dict(lds_bytes=BIG_LDS), "bad limits"),
        (dict(waves=1), "waves must be 0, 2, 4 or 8"), (dict(store=HALF), "n_rows and n_nnz go together")]),
    "pack_large_sparse": _sparse_batch_checks("pack_large_sparse") + _named("pack_large_sparse", [
        (dict(store=None, n_rows=None), "count pass needs n_rows and n_nnz"), (dict(store=STORE, slot0=-1), "store mismatch"), (dict(nnz_cap=0), "bad nnz_cap"),
        (dict(workspace=None), WSMSG)]),
    "cone_step": _dense_step_checks(),
    "cone_step_warm": _warm_checks("cone_step_warm") + _dense_step_checks(),
    "cone_step_ipm": _dense_step_checks(mode=False),
    "cone_step_sparse": _sparse_step_checks(),
    "cone_step_sparse_ipm": _sparse_step_checks(mode=False, warm_too=False),
    "lite_from_packed": _named("lite_from_packed", [
        (dict(src=None), "null store"), (dict(src=store(n=-1)), "need 0 < d <= 256, n < 2^31"), (dict(dst=lite(n=3)), "bad lite store " + STOREMSG)]),
}

E = -1   # CAVE_E_INVALID
NOTHING = dict(solve=None, pred=None, B=0, next_ctrs=None, B_next=0, m_max=0, next=None, cu_tickets=None)   # a step with nothing to do
NO_NEXT = dict(next_cones=None, next=None)


def _bad_solve_stores(who):
    bad = [lite(n=3), lite(d=11), lite(ell=_addr(160, np.int32, off=8)), lite(csr16=_addr(4 * 768, np.int32, off=4))]
    bad += [lite(**{k: 0}) for k in ("hdr", "usign", "avg", "rowptr", "ell", "csr16", "rl")]
    return [(dict(solve=s), E, f"{who}: bad solve store {STOREMSG}") for s in bad]


def _bad_workspaces(who):
    return [(over, E, f"{who}: {WSMSG}") for over in (dict(slice_bytes=1016), dict(slice_bytes=1 << 32), dict(slice_bytes=1028), dict(n_slots=0),
                                                      dict(workspace=WS + 8))]


def _bad_batches(who, arg):
    bad = [cones(B=-1), cones(m=65536), cones(d=0), cones(d=65536)]
    mis = [cones(key=_addr(8, np.uint32, off=2)), cones(val=_addr(8, np.float32, off=2)), cones(ent_off=_addr(8, np.int64, off=4)), cones(key=0)]
    return [({arg: c}, E, f"{who}: bad batch (need 0 <= m_max <= 65535, 0 < d <= 65535)") for c in bad] + \
           [({arg: c}, E, f"{who}: null or misaligned ent_off / key / val") for c in mis]


# entry -> [(overrides, return code, full message or None: the last error stays as it was)]
EXTRA = {
    "default_limits": [({}, 0, None), (dict(d=0), E, "default_limits: bad shape"), (dict(m_max=0), 0, None)],
    "cone_dense": [(dict(m_max=-1), E, "cone_dense: bad shape (need 0 < d <= 65535)"), (dict(d=0), E, "cone_dense: bad shape (need 0 < d <= 65535)"),
                   (dict(d=65536), E, "cone_dense: bad shape (need 0 < d <= 65535)"), (dict(mode=-1), E, "cone_dense: bad mode"),
                   (dict(B=0, ctrs=None, pred=None, waves=3), 0, None), (dict(B=0, mode=6), E, "cone_dense: bad mode"),
                   (dict(mode=4, pred=None, waves=3), E, "cone_dense: waves must be 0, 1, 2, 4 or 8"),     # AVG needs no prediction
                   (dict(m_max=0, ctrs=None, waves=3), E, "cone_dense: waves must be 0, 1, 2, 4 or 8"),     # no rows: no block
                   (dict(nnz_cap=-5, lds_bytes=BIG_LDS), E, "cone_dense: bad nnz_cap / lds_bytes")],
    "pack_count": [(dict(m_max=-1), E, "pack_count: bad shape"), (dict(d=0), E, "pack_count: bad shape"), (dict(d=65536), E, "pack_count: bad shape"),
                   (dict(m_max=1 << 17, d=1 << 15), E, "pack_count: bad shape"), (dict(n_rows=None), E, "pack_count: null pointer"),
                   (dict(n_nnz=None), E, "pack_count: null pointer"), (dict(B=0, ctrs=None), 0, None)],
    "pack_fill": [(dict(d=0), E, "pack_fill: bad shape"), (dict(store=None), E, "pack_fill: null pointer"),
                  (dict(store=store(d=11)), E, "pack_fill: store mismatch"), (dict(slot0=1), E, "pack_fill: store mismatch"),
                  (dict(store=store(n_nnz=NNNZ)), E, "pack_fill: n_rows and n_nnz go together"), (dict(B=0, ctrs=None, store=None), 0, None)],
    "packed_lds_bytes": [(dict(d=0), E, None), (dict(max_rows=-1), E, None), (dict(max_nnz=-1), E, None), (dict(max_rows=5000), E, None)],
    "cone_packed": [(dict(B=-1), E, "cone_packed: null store / bad B"), (dict(mode=-1), E, "cone_packed: bad mode"),
                    (dict(lds_bytes=BIG_LDS), E, "cone_packed: bad lds_bytes"), (dict(B=0, pred=None, lds_bytes=0), 0, None),
                    (dict(B=0, mode=6), E, "cone_packed: bad mode"), (dict(mode=4, pred=None, lds_bytes=0), E, "cone_packed: bad lds_bytes")],
    "large_slice_bytes": [(dict(m_max=-1), E, None), (dict(d=0), E, None), (dict(nnz_cap=0), E, None), (dict(band_entries=-1), E, None)],
    "packed_large_slice_bytes": [(dict(d=0), E, None), (dict(max_rows=-1), E, None), (dict(band_entries=-1), E, None)],
    "packed_large_lds_bytes": [(dict(max_rows=-1), E, None), (dict(max_bw=-1), E, None)],
    "packed_large_rb_bytes": [],
    "cone_dense_large": [(dict(m_max=65536), E, "cone_dense_large: bad shape (need m_max, d <= 65535, m_max*d < 2^32)"),
                         (dict(d=65536), E, "cone_dense_large: bad shape (need m_max, d <= 65535, m_max*d < 2^32)"),
                         (dict(nnz_cap=1 << 31), E, "cone_dense_large: bad nnz_cap"), (dict(lds_bytes=BIG_LDS), E, "cone_dense_large: bad lds_bytes"),
                         (dict(B=0, ctrs=None, workspace=None), 0, None), (dict(B=0, mode=6), E, "cone_dense_large: bad mode"),
                         *_bad_workspaces("cone_dense_large")],
    "pack_large": [(dict(m_max=65536), E, "pack_large: bad shape"), (dict(n_nnz=None), E, "pack_large: count pass needs n_rows and n_nnz"),
                   (dict(store=store(d=11)), E, "pack_large: store mismatch"), (dict(store=STORE, slot0=1), E, "pack_large: store mismatch"),
                   (dict(nnz_cap=1 << 31), E, "pack_large: bad nnz_cap"), (dict(B=0, ctrs=None, workspace=None), 0, None),
                   (dict(store=STORE, n_rows=None, n_nnz=None, workspace=None), E, "pack_large: " + WSMSG), *_bad_workspaces("pack_large")],
    "cone_packed_large": [(dict(B=-1), E, "cone_packed_large: null store / bad B"), (dict(waves=8), E, "cone_packed_large: waves must be 0, 1, 2 or 4"),
                          (dict(lds_bytes=BIG_LDS), E, "cone_packed_large: bad lds_bytes"), (dict(B=0, pred=None, workspace=None), 0, None),
                          *_bad_workspaces("cone_packed_large")],
    "pack_count_sparse": [*_bad_batches("pack_count_sparse", "cones"), (dict(n_nnz=None), E, "pack_count_sparse: null pointer"),
                          (dict(waves=3), E, "pack_count_sparse: waves must be 0, 2, 4 or 8"), (dict(cones=cones(B=0, **NULLS), n_rows=None), 0, None)],
    "pack_fill_sparse": [*_bad_batches("pack_fill_sparse", "cones"), (dict(store=store(d=11)), E, "pack_fill_sparse: store mismatch"),
                         (dict(slot0=1), E, "pack_fill_sparse: store mismatch"), (dict(cones=cones(B=0, **NULLS), store=None), 0, None)],
    "pack_large_sparse": [*_bad_batches("pack_large_sparse", "cones"), (dict(n_nnz=None), E, "pack_large_sparse: count pass needs n_rows and n_nnz"),
                          (dict(store=store(d=11)), E, "pack_large_sparse: store mismatch"), (dict(nnz_cap=1 << 31), E, "pack_large_sparse: bad nnz_cap"),
                          (dict(cones=cones(B=0, **NULLS), workspace=None), 0, None), *_bad_workspaces("pack_large_sparse")],
    "step_lds_bytes": [(dict(m_max=-1), E, None), (dict(d=0), E, None), (dict(d=257), E, None), (dict(m_max=32768), E, None), (dict(m_max=235, d=229), E, None)],
    "lite_from_packed": [(dict(dst=None), E, "lite_from_packed: null store"), (dict(src=store(n=0), dst=lite(n=0, ell=0)), 0, None),
                         (dict(src=store(n=1 << 31)), E, "lite_from_packed: need 0 < d <= 256, n < 2^31"),
                         (dict(src=store(d=0)), E, "lite_from_packed: need 0 < d <= 256, n < 2^31"),
                         (dict(src=store(d=257)), E, "lite_from_packed: need 0 < d <= 256, n < 2^31"),
                         (dict(dst=lite(d=11)), E, "lite_from_packed: bad lite store " + STOREMSG),
                         (dict(dst=lite(ell=_addr(160, np.int32, off=8))), E, "lite_from_packed: bad lite store " + STOREMSG)],
}
_DENSE_EXTRA = [(dict(B_next=-1), E, "cone_step: bad batch sizes"), (dict(B_next=(1 << 31) - 4), E, "cone_step: bad batch sizes"),
                (dict(d=257), E, "cone_step: need 0 < d <= 256"), (NOTHING, 0, None), (dict(NOTHING, d=0), 0, None),
                (dict(B_next=0, m_max=40000, next_ctrs=None, next=None, cu_tickets=None), E, "cone_step: cu_tickets is null"),   # solve only: m_max unused
                (dict(B=0, solve=None, pred=None, next=None), E, "cone_step: bad next store " + STOREMSG),                    # pack only
                (dict(B=0, next=SOLVE, next_ctrs=None), E, "cone_step: next_ctrs is null"),
                (dict(next=lite(n=3)), E, "cone_step: bad next store " + STOREMSG), (dict(ids=PRED, solve=lite(n=1), next=None), E, "cone_step: bad next store " + STOREMSG),
                (dict(m_max=235, d=229, solve=lite(d=229)), E, "cone_step: shape does not qualify (cave_hip_step_lds_bytes)"),
                *_bad_solve_stores("cone_step")]
_MODE_EXTRA = [(dict(mode=-1), E, "{}: bad mode (PROJECT .. AVG)"), (dict(mode=4, pred=None, solve=None), E, "{}: bad solve store " + STOREMSG)]
EXTRA["cone_step"] = _DENSE_EXTRA + [(o, rc, m.format("cone_step")) for o, rc, m in _MODE_EXTRA]
EXTRA["cone_step_warm"] = EXTRA["cone_step"] + [
    (dict(warm=warm(0)), E, "cone_step_warm: n_entries must be a power of two"), (dict(warm=warm(1 << 40)), E, "cone_step_warm: n_entries must be a power of two"),
    (dict(warm=warm(theta=0)), E, "cone_step_warm: null key / theta array"), (dict(NOTHING, warm=warm(6)), E, "cone_step_warm: n_entries must be a power of two"),
    (dict(warm=None, cu_tickets=None), E, "cone_step: cu_tickets is null")]
EXTRA["cone_step_ipm"] = _DENSE_EXTRA + [(dict(pred=None, solve=None), E, "cone_step: pred is null")]
_SPARSE_EXTRA = [*_bad_batches("cone_step_sparse", "next_cones"), (dict(next_cones=cones(B=(1 << 31) - 4)), E, "cone_step_sparse: bad batch sizes"),
                 (dict(next_cones=cones(m=0)), E, "cone_step_sparse: shape does not qualify (cave_hip_step_lds_bytes)"),
                 (dict(next_cones=cones(d=257)), E, "cone_step_sparse: shape does not qualify (cave_hip_step_lds_bytes)"),
                 (dict(solve=lite(d=11)), E, "cone_step_sparse: d of the batch differs from the store's d"),
                 (dict(B=0, solve=lite(d=11), pred=None, cu_tickets=None), E, "cone_step_sparse: cu_tickets is null"),
                 (dict(B=0, solve=None, pred=None, next=lite(n=3)), E, "cone_step_sparse: bad next store " + STOREMSG),
                 (dict(solve=lite(n=3)), E, "cone_step_sparse: bad solve store " + STOREMSG),
                 # no next batch (null or empty): the dense entry's checks under the dense entry's name, d from the solve store
                 (dict(NO_NEXT, solve=None), E, "cone_step_sparse: solve store is null"), (dict(NO_NEXT, solve=None, cu_tickets=None, B=-1), E, "cone_step: bad batch sizes"),
                 (dict(NO_NEXT, B=0, solve=None, pred=None, cu_tickets=None), 0, None), (dict(next_cones=cones(B=0, **NULLS), B=0, solve=None, next=None), 0, None),
                 (dict(NO_NEXT, cu_tickets=None), E, "cone_step: cu_tickets is null"), (dict(next_cones=cones(B=0, m=-1), next=None, pred=None), E, "cone_step: pred is null"),
                 (dict(NO_NEXT, solve=lite(d=257)), E, "cone_step: need 0 < d <= 256"), (dict(NO_NEXT, solve=lite(n=3)), E, "cone_step: bad solve store " + STOREMSG)]
EXTRA["cone_step_sparse"] = _SPARSE_EXTRA + [(o, rc, m.format("cone_step_sparse")) for o, rc, m in _MODE_EXTRA] + [
    (dict(warm=warm(0)), E, "cone_step_sparse: n_entries must be a power of two"), (dict(warm=warm(theta=0)), E, "cone_step_sparse: null key / theta array"),
    (dict(NO_NEXT, warm=warm(6)), E, "cone_step_warm: n_entries must be a power of two"), (dict(NO_NEXT, solve=None, warm=warm(6)), E, "cone_step_sparse: solve store is null"),
    (dict(NO_NEXT, mode=5), E, "cone_step: bad mode (PROJECT .. AVG)")]
EXTRA["cone_step_sparse_ipm"] = _SPARSE_EXTRA + [(dict(pred=None, solve=None), E, "cone_step_sparse: pred is null")]


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load_library()


def run(lib, entry, over):
    names, good = ENTRIES[entry]
    assert set(over) <= set(good), (entry, over)
    args = dict(good, **over)
    argv = [C.byref(v) if isinstance(v, C.Structure) else v for v in (args[n] for n in names)]
    assert lib.cave_hip_default_limits(-1, 1, None, None) == E   # the last error before the call: SENTINEL
    rc = getattr(lib, "cave_hip_" + entry)(*argv)
    return rc, lib.cave_hip_last_error().decode()


def test_the_tables_cover_the_twenty_cone_entries():
    assert len(ENTRIES) == 23 and set(ENTRIES) == set(EXTRA)    # "the twenty": the four large size queries and the five steps one by one
    assert set(CHECKS) <= set(ENTRIES)
    assert all("cave_hip_" + e in _lib.ABI_SYMBOLS for e in ENTRIES)


@pytest.mark.parametrize("entry", sorted(CHECKS))
def test_each_check_alone_is_the_first_to_fail(lib, entry):
    for over, msg in CHECKS[entry]:
        assert run(lib, entry, over) == (E, msg), (entry, over)


def _bad_theta():
    return _addr(8 * 32, np.float32, off=4)


# Adjacent checks that read the same argument: the merge of their two rows would only repeat the earlier row, so the call
# that violates both is written out.  (argument, what it holds) -> the earlier check's message, without the entry's name
SAME_ARGUMENT = {
    "warm": [(lambda: warm(6, key=0), "n_entries must be a power of two"), (lambda: warm(key=0, theta=_bad_theta()), "null key / theta array")],
    "batch": [(lambda: cones(m=-1, **NULLS), "bad batch (need 0 <= m_max <= 65535, 0 < d <= 65535)")],
    "next": [(lambda: lite(n=3, d=11), "d of the batch differs from the store's d")],
}
SAME_ARGUMENT_CALLS = [(e, "warm", "warm", e) for e in ("cone_step_warm", "cone_step_sparse")] + \
    [(e, "cones", "batch", e) for e in ("pack_count_sparse", "pack_fill_sparse", "pack_large_sparse")] + \
    [(e, "next_cones", "batch", "cone_step_sparse") for e in ("cone_step_sparse", "cone_step_sparse_ipm")] + \
    [(e, "next", "next", "cone_step_sparse") for e in ("cone_step_sparse", "cone_step_sparse_ipm")]


@pytest.mark.parametrize("entry", sorted(CHECKS))
def test_of_two_adjacent_checks_the_earlier_one_reports(lib, entry):
    rows = CHECKS[entry]
    for (first, msg), (second, _) in zip(rows, rows[1:]):
        both = dict(second, **first)
        assert run(lib, entry, both) == (E, msg), (entry, both)
    for e, arg, kind, who in SAME_ARGUMENT_CALLS:
        if e == entry:
            for make, what in SAME_ARGUMENT[kind]:
                assert run(lib, entry, {arg: make()}) == (E, f"{who}: {what}"), (entry, arg, what)


@pytest.mark.parametrize("entry", sorted(EXTRA))
def test_further_rejections_and_early_returns(lib, entry):
    for over, rc, msg in EXTRA[entry]:
        assert run(lib, entry, over) == (rc, SENTINEL if msg is None else msg), (entry, over)


def test_a_size_query_that_succeeds_leaves_the_last_error(lib):
    for entry in ("default_limits", "packed_lds_bytes", "large_slice_bytes", "packed_large_slice_bytes", "packed_large_lds_bytes",
                  "packed_large_rb_bytes", "step_lds_bytes"):
        rc, msg = run(lib, entry, {})
        assert rc >= 0 and msg == SENTINEL, (entry, rc, msg)
