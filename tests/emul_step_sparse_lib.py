"""ctypes loader for tests/emul/simt_step_sparse.cpp: the SIMT emulation with the step kernel's sparse pack half
(TEST INFRASTRUCTURE ONLY).

A small unit of its own (one code path: it builds in a fraction of the time tests/emul/simt_abi.cpp takes), loaded
beside that library: `SimtStepSparse` is an emul_lib.Simt (dense pack half, solve half, ...) with one more entry,
`step_pack_sparse`, which fills a host lite store from host arrays of the sparse wire format with the product's own
launch limits.  Unlike `Simt.step_pack` callers choose the array objects themselves (the alignment tests pass slices
at chosen element offsets), so nothing here copies `key` / `val`.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from cave_amd import _build
from emul_lib import Simt, _p, lite_store
from emul_sparse_lib import SparseC

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "simt_step_sparse.cpp")


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_simt_step_sparse_asan.so" if asan else "_simt_step_sparse.so")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    return _build.make(["g++", "-std=c++17", "-fPIC", "-shared", "-w", *flags, "-I" + os.path.join(_HERE, "emul", "simt"), _SRC,
                        "-o", out], _SRC, out)


def sparse_of(ctrs):
    """(ent_off int64, key uint32, val float32) of a dense (B, m, d) array: row-major entries, as SparseCones.from_dense"""
    ctrs = np.asarray(ctrs, dtype=np.float32)
    B, m, d = ctrs.shape
    off, keys, vals = np.zeros(B + 1, np.int64), [], []
    for b in range(B):
        r, c = np.nonzero(ctrs[b])
        keys.append(((r.astype(np.int64) << 16) | c).astype(np.uint32))
        vals.append(ctrs[b][r, c].astype(np.float32))
        off[b + 1] = off[b] + len(r)
    return off, np.concatenate(keys) if keys else np.zeros(0, np.uint32), np.concatenate(vals) if vals else np.zeros(0, np.float32)


def shifted(a, o):
    """a copy of `a` whose first element sits at 16-byte residue 4 * o: a slice of a 16-byte aligned buffer"""
    raw = np.zeros(a.nbytes + 32, np.uint8)
    base = (-raw.ctypes.data) % 16 + 4 * o
    out = raw[base:base + a.nbytes].view(a.dtype)
    out[...] = a
    assert out.ctypes.data % 16 == 4 * o
    return out


class SimtStepSparse(Simt):
    def __init__(self, asan: bool = False):
        super().__init__(asan)            # tests/emul/simt_abi.cpp: the dense pack half, the solve half
        self.slib = C.CDLL(build(asan))   # tests/emul/simt_step_sparse.cpp: the sparse pack half

    def step_nnz_cap(self, m_max, d):
        return int(self.slib.cave_simt_step_nnz_cap(C.c_int64(m_max), C.c_int64(d)))

    def step_pack_sparse(self, ent_off, key, val, m_max, d, seed=0, fill=0):
        """run_pack_sparse_lite_instance over the batch (two waves per instance): -> (store, arrays, pack status [B]).
        ent_off int64, key uint32, val float32 are used where they lie."""
        assert ent_off.dtype == np.int64 and key.dtype == np.uint32 and val.dtype == np.float32
        assert ent_off.flags.c_contiguous and key.flags.c_contiguous and val.flags.c_contiguous
        B = len(ent_off) - 1
        s = SparseC(B=B, m_max=m_max, d=d, ent_off=ent_off.ctypes.data, key=key.ctypes.data, val=val.ctypes.data)
        st, arrs = lite_store(B, d, fill)
        status = np.full(B, -7, np.int32)
        rc = self.slib.cave_simt_step_pack_sparse(C.byref(s), C.c_uint64(seed), C.byref(st), _p(status))
        assert rc == 0, rc
        return st, arrs, status
