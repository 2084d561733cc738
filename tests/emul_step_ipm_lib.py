"""ctypes loader for tests/emul/simt_step_ipm.cpp: the SIMT emulation with the step kernel's interior-point solve half
(TEST INFRASTRUCTURE ONLY).

A small unit of its own (one code path: run_lite_instance<SoloCtx<32, 4>, false, IPM>), loaded beside the library of
tests/emul/simt_abi.cpp: `SimtStepIpm` is an emul_lib.Simt (pack half, lite_from_packed, the general kernels at one to
eight waves) with one more entry, `step_solve_ipm`, which reads the host lite stores those fill.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from cave_amd import _build
from emul_lib import Simt, _p, outs

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "simt_step_ipm.cpp")


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_simt_step_ipm_asan.so" if asan else "_simt_step_ipm.so")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    return _build.make(["g++", "-std=c++17", "-fPIC", "-shared", "-w", *flags, "-I" + os.path.join(_HERE, "emul", "simt"), _SRC,
                        "-o", out], _SRC, out)


class SimtStepIpm(Simt):
    def __init__(self, asan: bool = False):
        super().__init__(asan)            # tests/emul/simt_abi.cpp: the pack half, lite_from_packed, the general kernels
        self.ilib = C.CDLL(build(asan))   # tests/emul/simt_step_ipm.cpp: the interior-point solve half

    def step_solve_ipm(self, store, pred, sign=-1.0, max_iter=0, ids=None, B=None, flags=0, lds_bytes=0, m_max=0, seed=0):
        """The solve half of cave_hip_cone_step_ipm (one 64-lane wave per instance).  LDS: `lds_bytes`, or the product's
        figure for a launch with a pack half of m_max rows (0: solve-only, step_solve_lds_bytes(d) exactly)."""
        d = store.d
        pred = np.ascontiguousarray(pred, dtype=np.float32)
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        if B is None:
            B = len(ids) if ids is not None else len(pred)
        lds = lds_bytes or self.step_lds_bytes(m_max, d)
        assert lds > 0, (m_max, d, lds)
        out = outs(B, d)
        for k in ("proj", "target", "grad", "rnorm", "loss"):   # sentinels: what an instance does not write stays visible
            out[k][...] = 77.0
        out["status"][...] = -7
        out["iters"][...] = -7
        rc = self.ilib.cave_simt_step_solve_ipm(
            C.byref(store), _p(ids), _p(pred), C.c_int64(B), C.c_float(sign), C.c_int32(max_iter), C.c_int32(flags),
            C.c_int32(lds), C.c_uint64(seed),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out

    def general_ipm(self, ctrs, pred, max_iter, waves, sign=-1.0, nnz_cap=0, lds_bytes=0):
        """The EXISTING general kernel (cone_dense.h on WaveCtx / BlockCtx<waves>) in the interior-point mode, with a
        non-zero budget and an LDS figure of the caller's choosing (0: the product's defaults)."""
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        pred = np.ascontiguousarray(pred, dtype=np.float32)
        B, m, d = ctrs.shape
        out = outs(B, d)
        rc = self.lib.cave_simt_cone_dense(
            _p(ctrs), _p(pred), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int32(5), C.c_float(sign), C.c_float(0.0),
            C.c_int32(max_iter), C.c_int32(nnz_cap), C.c_int32(lds_bytes), C.c_int32(waves), C.c_uint64(0),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out
