"""ctypes loader for the serial gcc build of the sparse pack pass, tests/emul/emul_sparse.cpp (TEST INFRASTRUCTURE ONLY).

Beside tests/emul_lib.py, whose `Emul.pack` / `Emul.pack_large` write a store from the dense form; `EmulSparse` writes
one from the sparse wire format (host arrays ent_off / key / val) with the same launch limits, so the two can be
compared array by array.  Unlike the dense helpers these do not assert on the per-instance status: malformed input is
part of what the tests feed them.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from cave_amd import _build
from cave_amd._lib import SparseConesC as SparseC  # struct cave_sparse_cones (include/cave_hip.h), here over host arrays
from emul_lib import _p, host_store as empty_store

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "emul_sparse.cpp")


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_emul_sparse_asan.so" if asan else "_emul_sparse.so")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    return _build.make(["g++", "-std=c++17", "-fPIC", "-shared", "-w", *flags, _SRC, "-o", out], _SRC, out)


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
