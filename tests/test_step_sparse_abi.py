"""CPU tier, no compute: cave_hip_cone_step_sparse is declared, exported and bound with the header's 24 parameters, and
every argument error of include/cave_hip.h is refused before any launch (works without a GPU)."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from cave_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cave_hip_cone_step_sparse"
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


def call(lib, solve, B, cones, nxt, warm=None, tickets=True, pred=True, mode=2):
    tk = _buf(4096, np.uint32)
    pr = _buf(max(B, 1) * 256, np.float32)
    rc = lib.cave_hip_cone_step_sparse(
        None if solve is None else C.byref(solve), None, pr.ctypes.data if pred else None, B, mode, 1.0, 0.2, 0, 0, *NONE7,
        None if cones is None else C.byref(cones), None if nxt is None else C.byref(nxt), None,
        None if warm is None else C.byref(warm), None, None, tk.ctypes.data if tickets else None, None)
    return rc, lib.cave_hip_last_error().decode()


def test_symbol_is_declared_exported_and_bound_with_24_parameters(lib):
    assert NAME in _lib.ABI_SYMBOLS and hasattr(lib, NAME)
    hdr = open(os.path.join(ROOT, "include", "cave_hip.h")).read()
    decl = re.search(r"int32_t\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == 24 and params[16].startswith("const cave_sparse_cones*") and params[-1] == "void* stream"
    assert len(getattr(lib, NAME).argtypes) == 24
    assert lib.cave_hip_version() == 10   # additive: the ABI version stays


def test_nothing_to_do_returns_ok(lib):
    assert call(lib, None, 0, None, None, tickets=False)[0] == 0
    empty, keep = _cones(0, 235, 190, null=True)
    assert call(lib, None, 0, empty, None, tickets=False)[0] == 0


def test_invalid_arguments_are_refused_before_any_launch(lib):
    d, m = 190, 235
    solve, k1 = _lite(4, d)
    nxt, k2 = _lite(4, d)
    good, k3 = _cones(4, m, d)
    # null ent_off / key / val with B > 0
    bad, k4 = _cones(4, m, d, null=True)
    rc, msg = call(lib, solve, 4, bad, nxt)
    assert rc == -1 and "ent_off / key / val" in msg
    # d different from a store's d
    other, k5 = _lite(4, 64)
    rc, msg = call(lib, solve, 4, good, other)
    assert rc == -1 and "differs from the store's d" in msg
    rc, msg = call(lib, other, 4, good, nxt)
    assert rc == -1 and "differs from the store's d" in msg
    # next the same store as solve
    rc, msg = call(lib, solve, 4, good, solve)
    assert rc == -1 and "different stores" in msg
    # cu_tickets missing: with a pack half, and on the solve-only form
    rc, msg = call(lib, solve, 4, good, nxt, tickets=False)
    assert rc == -1 and "cu_tickets" in msg
    rc, msg = call(lib, solve, 4, None, None, tickets=False)
    assert rc == -1 and "cu_tickets" in msg
    # shapes step_limits refuses: d beyond the fused form, too many rows, no rows
    for mm, dd in ((m, 229), (m, 300), (40000, d), (0, d)):
        s2, k6 = _lite(4, dd)
        n2, k7 = _lite(4, dd)
        c2, k8 = _cones(4, mm, dd)
        rc, msg = call(lib, s2, 4, c2, n2)
        assert rc == -1 and "does not qualify" in msg, (mm, dd, msg)
        assert (lib.cave_hip_step_lds_bytes(mm, dd) < 0) or mm == 0
    # a bad warm cache: same rules as cave_hip_cone_step_warm
    key, theta = _buf(8, np.uint64), _buf(8 * 32 + 1, np.float32)
    for wc, text in ((_lib.WarmCacheC(n_entries=6, key=key.ctypes.data, theta=theta.ctypes.data), "power of two"),
                     (_lib.WarmCacheC(n_entries=8, key=0, theta=theta.ctypes.data), "null key / theta"),
                     (_lib.WarmCacheC(n_entries=8, key=key.ctypes.data, theta=theta.ctypes.data + 4), "16-byte aligned")):
        rc, msg = call(lib, solve, 4, good, nxt, warm=wc)
        assert rc == -1 and text in msg, msg
        rc, msg = call(lib, solve, 4, None, None, warm=wc)   # the solve-only form delegates: the same rules
        assert rc == -1 and text in msg, msg
    # a null next store, a null prediction, a bad mode
    rc, msg = call(lib, solve, 4, good, None)
    assert rc == -1 and "next store" in msg
    rc, msg = call(lib, solve, 4, good, nxt, pred=False)
    assert rc == -1 and "pred is null" in msg
    rc, msg = call(lib, solve, 4, good, nxt, mode=5)
    assert rc == -1 and "bad mode" in msg
