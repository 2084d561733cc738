"""Loader for tests/emul/simt_apgd.cpp: the APGD projector (cave_amd/csrc/apgd.h) under the SIMT emulation (TEST
INFRASTRUCTURE ONLY).

Two builds of the one unit (emul_solver_common): a shared library for ctypes (`SimtApgd`), and a stand-alone program
under AddressSanitizer + UBSan (`run_asan`: cases go in through a file, results come back through a file; every buffer
is a heap block of its exact size).  `SimtApgd.run` and `apgd_cases.gpu_run` take the same arguments and return the same
dict, so the two tiers share their checks.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

import emul_solver_common as common
from cave_amd._lib import SparseConesC
from emul_solver_common import _p

_SRC = "simt_apgd.cpp"

# (name, dtype, flag bit, shape of (B, m, d))
TABLE = (("proj", np.float32, 1, lambda B, m, d: (B, d)), ("rnorm", np.float32, 1, lambda B, m, d: (B,)),
         ("target", np.float32, 1, lambda B, m, d: (B, d)), ("loss", np.float32, 1, lambda B, m, d: (B,)),
         ("grad", np.float32, 1, lambda B, m, d: (B, d)), ("status", np.int32, 1, lambda B, m, d: (B,)),
         ("iters", np.int32, 1, lambda B, m, d: (B,)), ("x_curr", np.float64, 1, lambda B, m, d: (B, m)),
         ("x_prev", np.float64, 1, lambda B, m, d: (B, m)), ("step", np.float64, 1, lambda B, m, d: (B,)),
         ("pgrad", np.float64, 1, lambda B, m, d: (B,)))
FLOAT_OUT = ("proj", "rnorm", "target", "loss", "grad")


def build(asan: bool = False) -> str:
    return common.build(_SRC, "APGD_MAIN", asan)


class SimtApgd:
    def __init__(self):
        self.lib = C.CDLL(build())
        tail = [C.c_int32, C.c_float] + [C.c_int32] * 4 + [C.c_void_p] * 11 + [C.c_uint64, C.c_int32]
        self.lib.cave_simt_cone_apgd.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + tail
        self.lib.cave_simt_cone_apgd_sparse.argtypes = [C.POINTER(SparseConesC), C.c_void_p] + tail
        self.lib.cave_simt_apgd_lds_bytes.argtypes = self.lib.cave_simt_apgd_waves.argtypes = [C.c_int64] * 3
        self.lib.cave_simt_apgd_last_error.restype = C.c_char_p

    def lds_bytes(self, m, d, cap):
        return int(self.lib.cave_simt_apgd_lds_bytes(m, d, cap))

    def waves(self, m, d, cap):
        return int(self.lib.cave_simt_apgd_waves(m, d, cap))

    def last_error(self):
        return self.lib.cave_simt_apgd_last_error().decode()

    def raw(self, cones, pred, dims, mode, sign, k_start, n_iter, power_iter, cap, ptrs, seed=0, waves=0):
        """the raw entry: `cones` a dense array / None, or a SparseConesC; `ptrs` the eleven trailing pointers as numpy
        arrays or None (x_curr, x_prev, step, proj, rnorm, target, loss, grad, status, iters, pgrad)"""
        tail = (mode, sign, k_start, n_iter, power_iter, cap, *[_p(a) for a in ptrs], seed, waves)
        if isinstance(cones, SparseConesC) or dims is None:
            return int(self.lib.cave_simt_cone_apgd_sparse(None if cones is None else C.byref(cones), _p(pred), *tail))
        return int(self.lib.cave_simt_cone_apgd(_p(cones), _p(pred), *dims, *tail))

    def run(self, cones, pred, mode=1, sign=1.0, n_iter=20, power_iter=8, cap=None, k_start=0, state=None, seed=0, waves=0,
            want_state=True):
        """One launch on sentinel-filled outputs -> (rc, dict of TABLE's outputs).  `cones`: a dense (B, m, d) float32 array
        or a sparse triple (m, d, ent_off, key, val); `state`: (x_curr, x_prev, step) of the launch before, copied."""
        sparse = not isinstance(cones, np.ndarray)
        if sparse:
            m, d, ent_off, key, val = cones
            B = len(ent_off) - 1
            ent_off, key, val = (np.ascontiguousarray(ent_off, np.int64), np.ascontiguousarray(key, np.uint32),
                                 np.ascontiguousarray(val, np.float32))
            keep = (ent_off, key, val)
            c = SparseConesC(B=B, m_max=m, d=d, ent_off=ent_off.ctypes.data, key=key.ctypes.data if key.size else 8,
                             val=val.ctypes.data if val.size else 8)
            dims = None
        else:
            cones = np.ascontiguousarray(cones, np.float32)
            B, m, d = cones.shape
            c, dims = cones, (B, m, d)
        pred = np.ascontiguousarray(pred, np.float32)
        if cap is None:
            cap = m * d
        o = common.outputs(TABLE, 1, (B, m, d))
        if state is not None:
            for name, a in zip(("x_curr", "x_prev", "step"), state):
                o[name][:a.size] = np.asarray(a, np.float64).ravel()
        elif not want_state:
            o["x_curr"] = o["x_prev"] = o["step"] = None
        ptrs = [o[n] for n in ("x_curr", "x_prev", "step", "proj", "rnorm", "target", "loss", "grad", "status", "iters", "pgrad")]
        rc = self.raw(c, pred, dims, mode, sign, k_start, n_iter, power_iter, cap, ptrs, seed, waves)
        if rc != 0:
            return rc, o
        table = [t for t in TABLE if o[t[0]] is not None]
        return rc, common.strip_guards(table, o, (B, m, d))


def run_asan(cases, workdir: str, seed: int = 11):
    """`cases`: dicts with cones (dense array or sparse triple), pred, mode, sign, n_iter, power_iter, cap, waves.  Runs
    them in ONE process of the sanitizer build and returns a list of (rc, outputs dict)."""
    records = []
    for k in cases:
        cones = k["cones"]
        sparse = not isinstance(cones, np.ndarray)
        if sparse:
            m, d, ent_off, key, val = cones
            B = len(ent_off) - 1
            blobs = [np.ascontiguousarray(ent_off, np.int64), np.ascontiguousarray(key, np.uint32), np.ascontiguousarray(val, np.float32)]
            Z = len(key)
        else:
            B, m, d = cones.shape
            blobs, Z = [np.ascontiguousarray(cones, np.float32)], 0
        blobs.append(np.ascontiguousarray(k["pred"], np.float32))
        hdr = [int(sparse), B, m, d, Z, k.get("mode", 1), int(k.get("sign", 1)), k.get("n_iter", 20), k.get("power_iter", 8),
               k.get("cap") or m * d, seed, k.get("waves", 0)]
        records.append((hdr, blobs, 1, (B, m, d)))
    return common.run_asan(build(asan=True), "apgd", "apgd-ok", TABLE, records, workdir)
