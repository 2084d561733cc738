"""CPU tier, no compute: cave_hip_cone_step_ipm and cave_hip_cone_step_sparse_ipm (the fused step in the interior-point
mode) are declared, exported and bound with the header's 22 / 19 parameters -- those of their siblings without `mode`,
`inner_ratio` and the cache arguments --, every argument error of include/cave_hip.h is refused before any launch, and
the existing entry points keep refusing mode 5 (works without a GPU)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from cave_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSE, SPARSE = "cave_hip_cone_step_ipm", "cave_hip_cone_step_sparse_ipm"
NONE7 = [None] * 7


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load_library()


def _buf(n, dtype=np.uint8):
    """a 16-byte aligned host array: the calls below fail before anything is read or launched"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * np.dtype(dtype).itemsize].view(dtype)


def _lite(n, d):
    arrs = {"hdr": _buf(n * 8, np.int32), "usign": _buf(n * d), "avg": _buf(n * d, np.float32), "rowptr": _buf(n * 33, np.int32),
            "ell": _buf(n * 4 * d, np.int32), "csr16": _buf(n * 768, np.int32), "rl": _buf(n * 32)}
    return _lib.LiteStore(n=n, d=d, reserved=0, **{k: v.ctypes.data for k, v in arrs.items()}), arrs


def _cones(B, m, d, null=False):
    arrs = (_buf(B + 1, np.int64), _buf(8, np.uint32), _buf(8, np.float32))
    p = [0, 0, 0] if null else [a.ctypes.data for a in arrs]
    return _lib.SparseConesC(B=B, m_max=m, d=d, ent_off=p[0], key=p[1], val=p[2]), arrs


def _ref(x):
    return None if x is None else C.byref(x)


def call_dense(lib, solve, B, ctrs, B_next, m, d, nxt, tickets=True, pred=True):
    tk = _buf(4096, np.uint32)
    pr = _buf(max(B, 1) * 256, np.float32)
    rc = lib.cave_hip_cone_step_ipm(
        _ref(solve), None, pr.ctypes.data if pred else None, B, 1.0, 0, 0, *NONE7,
        None if ctrs is None else ctrs.ctypes.data, B_next, m, d, _ref(nxt), None, tk.ctypes.data if tickets else None, None)
    return rc, lib.cave_hip_last_error().decode()


def call_sparse(lib, solve, B, cones, nxt, tickets=True, pred=True):
    tk = _buf(4096, np.uint32)
    pr = _buf(max(B, 1) * 256, np.float32)
    rc = lib.cave_hip_cone_step_sparse_ipm(
        _ref(solve), None, pr.ctypes.data if pred else None, B, 1.0, 0, 0, *NONE7,
        _ref(cones), _ref(nxt), None, tk.ctypes.data if tickets else None, None)
    return rc, lib.cave_hip_last_error().decode()


def _params(name):
    hdr = open(os.path.join(ROOT, "include", "cave_hip.h")).read()
    decl = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    return [" ".join(p.split()) for p in decl.split(",")]


def test_symbols_are_declared_exported_and_bound(lib):
    for name in (DENSE, SPARSE):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
    # the siblings' parameters in the siblings' order, without mode, inner_ratio and the cache arguments
    drop = {"int32_t mode", "float inner_ratio", "const cave_warm_cache* warm", "const int64_t* keys", "uint8_t* warm_hit"}
    for name, sibling, n in ((DENSE, "cave_hip_cone_step", 22), (SPARSE, "cave_hip_cone_step_sparse", 19)):
        params = _params(name)
        assert params == [p for p in _params(sibling) if p not in drop]
        assert len(params) == n and len(getattr(lib, name).argtypes) == n and params[-1] == "void* stream"
    assert lib.cave_hip_version() == 10   # additive: the ABI version stays


def test_nothing_to_do_returns_ok(lib):
    assert call_dense(lib, None, 0, None, 0, 0, 190, None, tickets=False)[0] == 0
    assert call_sparse(lib, None, 0, None, None, tickets=False)[0] == 0
    empty, keep = _cones(0, 235, 190, null=True)
    assert call_sparse(lib, None, 0, empty, None, tickets=False)[0] == 0


def test_dense_entry_refuses_invalid_arguments_before_any_launch(lib):
    d, m = 190, 235
    solve, k1 = _lite(4, d)
    nxt, k2 = _lite(4, d)
    ctrs = _buf(8, np.float32)
    # null solve store, too small a store, a store of another d, a null array
    rc, msg = call_dense(lib, None, 4, None, 0, 0, d, None)
    assert rc == -1 and "bad solve store" in msg
    rc, msg = call_dense(lib, solve, 5, None, 0, 0, d, None)
    assert rc == -1 and "bad solve store" in msg
    rc, msg = call_dense(lib, solve, 4, None, 0, 0, 64, None)
    assert rc == -1 and "bad solve store" in msg
    broken, k3 = _lite(4, d)
    broken.ell = 0
    rc, msg = call_dense(lib, broken, 4, None, 0, 0, d, None)
    assert rc == -1 and "bad solve store" in msg
    # batch sizes, d
    rc, msg = call_dense(lib, solve, -1, None, 0, 0, d, None)
    assert rc == -1 and "bad batch sizes" in msg
    rc, msg = call_dense(lib, solve, 4, ctrs, 1 << 31, m, d, nxt)
    assert rc == -1 and "bad batch sizes" in msg
    for dd in (0, 257):
        rc, msg = call_dense(lib, solve, 4, None, 0, 0, dd, None)
        assert rc == -1 and "0 < d <= 256" in msg
    # cu_tickets missing: with a pack half, and on the solve-only and pack-only forms
    for B, Bn in ((4, 4), (4, 0), (0, 4)):
        rc, msg = call_dense(lib, solve, B, ctrs if Bn else None, Bn, m if Bn else 0, d, nxt if Bn else None, tickets=False)
        assert rc == -1 and "cu_tickets" in msg
    # a null prediction
    rc, msg = call_dense(lib, solve, 4, None, 0, 0, d, None, pred=False)
    assert rc == -1 and "pred is null" in msg
    # the pack half: shapes step_limits refuses, null next_ctrs, null / same next store
    for mm, dd in ((m, 229), (40000, d)):
        s2, k4 = _lite(4, dd)
        n2, k5 = _lite(4, dd)
        rc, msg = call_dense(lib, s2, 4, ctrs, 4, mm, dd, n2)
        assert rc == -1 and "does not qualify" in msg, (mm, dd, msg)
    rc, msg = call_dense(lib, solve, 4, ctrs, 4, 0, d, nxt)
    assert rc == -1 and "bad m_max" in msg
    rc, msg = call_dense(lib, solve, 4, None, 4, m, d, nxt)
    assert rc == -1 and "next_ctrs is null" in msg
    rc, msg = call_dense(lib, solve, 4, ctrs, 4, m, d, None)
    assert rc == -1 and "bad next store" in msg
    rc, msg = call_dense(lib, solve, 4, ctrs, 4, m, d, solve)
    assert rc == -1 and "different stores" in msg


def test_sparse_entry_refuses_invalid_arguments_before_any_launch(lib):
    d, m = 190, 235
    solve, k1 = _lite(4, d)
    nxt, k2 = _lite(4, d)
    good, k3 = _cones(4, m, d)
    bad, k4 = _cones(4, m, d, null=True)
    rc, msg = call_sparse(lib, solve, 4, bad, nxt)
    assert rc == -1 and "ent_off / key / val" in msg
    other, k5 = _lite(4, 64)
    rc, msg = call_sparse(lib, solve, 4, good, other)
    assert rc == -1 and "differs from the store's d" in msg
    rc, msg = call_sparse(lib, other, 4, good, nxt)
    assert rc == -1 and "differs from the store's d" in msg
    rc, msg = call_sparse(lib, solve, 4, good, solve)
    assert rc == -1 and "different stores" in msg
    rc, msg = call_sparse(lib, solve, 4, good, nxt, tickets=False)
    assert rc == -1 and "cu_tickets" in msg
    rc, msg = call_sparse(lib, solve, 4, None, None, tickets=False)   # the solve-only form delegates: the same rules
    assert rc == -1 and "cu_tickets" in msg
    rc, msg = call_sparse(lib, None, 4, None, None)
    assert rc == -1 and "solve store is null" in msg
    for mm, dd in ((m, 229), (m, 300), (40000, d), (0, d)):
        s2, k6 = _lite(4, dd)
        n2, k7 = _lite(4, dd)
        c2, k8 = _cones(4, mm, dd)
        rc, msg = call_sparse(lib, s2, 4, c2, n2)
        assert rc == -1 and "does not qualify" in msg, (mm, dd, msg)
    rc, msg = call_sparse(lib, solve, 4, good, None)
    assert rc == -1 and "next store" in msg
    rc, msg = call_sparse(lib, solve, 4, good, nxt, pred=False)
    assert rc == -1 and "pred is null" in msg
    rc, msg = call_sparse(lib, solve, 4, None, None, pred=False)
    assert rc == -1 and "pred is null" in msg


def test_the_existing_entry_points_still_refuse_mode_5(lib):
    d, m = 190, 235
    solve, k1 = _lite(4, d)
    nxt, k2 = _lite(4, d)
    good, k3 = _cones(4, m, d)
    tk, pr = _buf(4096, np.uint32), _buf(4 * 256, np.float32)
    key, theta = _buf(8, np.uint64), _buf(8 * 32, np.float32)
    wc = _lib.WarmCacheC(n_entries=8, key=key.ctypes.data, theta=theta.ctypes.data)
    head = (C.byref(solve), None, pr.ctypes.data, 4, 5, 1.0, 0.2, 0, 0, *NONE7)
    rc = lib.cave_hip_cone_step(*head, None, 0, 0, d, None, None, tk.ctypes.data, None)
    assert rc == -1 and "bad mode" in lib.cave_hip_last_error().decode()
    rc = lib.cave_hip_cone_step_warm(*head, None, 0, 0, d, None, None, C.byref(wc), None, None, tk.ctypes.data, None)
    assert rc == -1 and "bad mode" in lib.cave_hip_last_error().decode()
    for cones, nx in ((good, nxt), (None, None)):
        rc = lib.cave_hip_cone_step_sparse(*head, _ref(cones), _ref(nx), None, None, None, None, tk.ctypes.data, None)
        assert rc == -1 and "bad mode" in lib.cave_hip_last_error().decode()


def test_the_integration_stub_binds_and_calls_the_entry_point(lib):
    """the prototypes are the header's, the ctypes stub is executed as printed (a call with
    nothing to do returns without touching a device; a bad call raises with the library's text)"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 10. The fused step in the interior-point mode"):]
    norm = lambda t: re.sub(r"\s+", " ", t).replace("( ", "(").strip()
    hdr = norm(open(os.path.join(ROOT, "include", "cave_hip.h")).read())
    protos = re.findall(r"int32_t cave_hip_\w+\([^;]*\);", re.search(r"^```c\n(.*?)^```", sec, flags=re.S | re.M).group(1))
    assert len(protos) == 2
    for proto in protos:
        assert norm(proto) in hdr, proto
    ns = {}
    exec(re.search(r"^```py\n(.*?)^```", sec, flags=re.S | re.M).group(1), ns)
    fresh = C.CDLL(_lib.LIB_PATH)
    fresh.cave_hip_last_error.restype = C.c_char_p
    ns["bind_cone_step_ipm"](fresh, _lib.LiteStore, _lib.SparseConesC)
    assert len(fresh.cave_hip_cone_step_ipm.argtypes) == 22 and len(fresh.cave_hip_cone_step_sparse_ipm.argtypes) == 19
    ns["cone_step_ipm"](fresh, None, None, 0, -1.0, None, None, None, None, None, None)
    solve, keep = _lite(4, 190)
    with pytest.raises(RuntimeError, match="cu_tickets"):
        ns["cone_step_ipm"](fresh, solve, _buf(4 * 190, np.float32).ctypes.data, 4, -1.0, None, None, None, None, None, None, d=190)
