"""ctypes loader for the serial gcc build of the sparse pack pass, tests/emul/emul_sparse.cpp (TEST INFRASTRUCTURE ONLY).

Beside tests/emul_lib.py, whose `Emul.pack` / `Emul.pack_large` write a store from the dense form; `EmulSparse` writes
one from the sparse wire format (host arrays ent_off / key / val) with the same launch limits, so the two can be
compared array by array.  Unlike the dense helpers these do not assert on the per-instance status: malformed input is
part of what the tests feed them.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from emul_lib import _DEPS, Store, _p

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "emul_sparse.cpp")


class SparseC(C.Structure):
    """struct cave_sparse_cones (include/cave_hip.h) over host arrays."""
    _fields_ = [("B", C.c_int64), ("m_max", C.c_int32), ("d", C.c_int32),
                ("ent_off", C.c_void_p), ("key", C.c_void_p), ("val", C.c_void_p)]


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_emul_sparse_asan.so" if asan else "_emul_sparse.so")
    newest = max(os.path.getmtime(p) for p in _DEPS[1:] + [_SRC])
    if os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-w", *flags, _SRC, "-o", out], check=True)
    return out


def empty_store(n_rows, n_nnz, d):
    """Exact-fit host store for the given per-instance counts: (Store, arrays)."""
    B = len(n_rows)
    row_off = np.concatenate([[0], np.cumsum(n_rows, dtype=np.int64)]).astype(np.int64)
    nnz_off = np.concatenate([[0], np.cumsum(n_nnz, dtype=np.int64)]).astype(np.int64)
    R, Z = int(row_off[-1]), int(nnz_off[-1])
    arrs = {
        "row_off": row_off, "nnz_off": nnz_off, "n_valid": np.zeros(B, np.int32), "flags": np.zeros(B, np.uint8),
        "usign": np.zeros(B * d, np.uint8), "avg": np.zeros(B * d, np.float32),
        "vkind": np.zeros(max(R, 1), np.uint8), "rlo": np.zeros(max(R, 1), np.uint32),
        "rhi": np.zeros(max(R, 1), np.uint32), "ccol": np.zeros(max(Z, 1), np.uint16),
        "cval": np.zeros(max(Z, 1), np.float32), "cptr": np.zeros(B * (d + 1), np.uint32),
        "cvar": np.zeros(max(Z, 1), np.uint16), "cvalc": np.zeros(max(Z, 1), np.float32),
    }
    return Store(n=B, d=d, reserved=0, **{k: v.ctypes.data for k, v in arrs.items()}), arrs


class EmulSparse:
    def __init__(self, asan: bool = False):
        self.lib = C.CDLL(build(asan))

    @staticmethod
    def _batch(ent_off, key, val, m_max, d):
        ent_off = np.ascontiguousarray(ent_off, dtype=np.int64)
        key = np.ascontiguousarray(key, dtype=np.uint32)
        val = np.ascontiguousarray(val, dtype=np.float32)
        s = SparseC(B=len(ent_off) - 1, m_max=m_max, d=d, ent_off=ent_off.ctypes.data, key=key.ctypes.data, val=val.ctypes.data)
        return s, (ent_off, key, val)  # (the arrays must outlive the call)

    def pack(self, ent_off, key, val, m_max, d, nnz_cap=0, lds_bytes=0):
        """Count + fill on the LDS path: (arrays, n_rows, n_nnz, status of the count pass, status of the fill pass)."""
        s, keep = self._batch(ent_off, key, val, m_max, d)
        B = s.B
        n_rows = np.zeros(B, np.int32); n_nnz = np.zeros(B, np.int32); st1 = np.zeros(B, np.int32); st2 = np.zeros(B, np.int32)
        rc = self.lib.cave_emul_pack_count_sparse(C.byref(s), C.c_int32(nnz_cap), C.c_int32(lds_bytes), _p(n_rows), _p(n_nnz), _p(st1))
        assert rc == 0, rc
        store, arrs = empty_store(n_rows, n_nnz, d)
        rc = self.lib.cave_emul_pack_fill_sparse(C.byref(s), C.c_int32(nnz_cap), C.c_int32(lds_bytes), C.byref(store),
                                                 C.c_int64(0), _p(st2))
        assert rc == 0, rc
        return arrs, n_rows, n_nnz, st1, st2

    def pack_large(self, ent_off, key, val, m_max, d, nnz_cap, slice_bytes):
        s, keep = self._batch(ent_off, key, val, m_max, d)
        B = s.B
        n_rows = np.zeros(B, np.int32); n_nnz = np.zeros(B, np.int32); st1 = np.zeros(B, np.int32); st2 = np.zeros(B, np.int32)
        rc = self.lib.cave_emul_pack_large_sparse(C.byref(s), C.c_int64(nnz_cap), C.c_int64(slice_bytes), _p(n_rows), _p(n_nnz),
                                                  None, C.c_int64(0), _p(st1))
        assert rc == 0, rc
        store, arrs = empty_store(n_rows, n_nnz, d)
        rc = self.lib.cave_emul_pack_large_sparse(C.byref(s), C.c_int64(nnz_cap), C.c_int64(slice_bytes), None, None,
                                                  C.byref(store), C.c_int64(0), _p(st2))
        assert rc == 0, rc
        return arrs, n_rows, n_nnz, st1, st2
