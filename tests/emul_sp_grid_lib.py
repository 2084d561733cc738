"""Loader for tests/emul/simt_sp_grid.cpp: the grid shortest-path kernel (cave_amd/csrc/sp_grid.h) under the SIMT
emulation (TEST INFRASTRUCTURE ONLY).

Two builds of the one unit (emul_solver_common): a shared library for ctypes (`SimtSpGrid`), and a stand-alone program
under AddressSanitizer + UBSan (`run_asan`: cases go in through a file, results come back through a file; every buffer
is a heap block of its exact size, the LDS block too).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

import emul_solver_common as common
from emul_solver_common import F_EVAL_COSTS, _p  # noqa: F401

_SRC = "simt_sp_grid.cpp"

F_SOL, F_OBJ, F_EVAL, F_STATUS, F_CONES = 2, 4, 8, 16, 32
F_ALL = 63


def n_arcs(h: int, w: int) -> int:
    return h * (w - 1) + (h - 1) * w


TABLE = (("sol", np.float32, F_SOL, lambda N, h, w: (N, n_arcs(h, w))), ("obj", np.float64, F_OBJ, lambda N, h, w: (N,)),
         ("eval", np.float64, F_EVAL, lambda N, h, w: (N,)), ("status", np.int32, F_STATUS, lambda N, h, w: (N,)),
         ("key", np.int32, F_CONES, lambda N, h, w: (N * 5 * n_arcs(h, w),)), ("val", np.float32, F_CONES, lambda N, h, w: (N * 5 * n_arcs(h, w),)))


def build(asan: bool = False) -> str:
    return common.build(_SRC, "SP_GRID_MAIN", asan)


class SimtSpGrid:
    def __init__(self):
        self.lib = C.CDLL(build())
        self.lib.cave_simt_sp_grid_lds_bytes.argtypes = [C.c_int64, C.c_int64]
        self.lib.cave_simt_sp_grid_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 6 + \
            [C.c_uint64, C.c_void_p]

    def lds_bytes(self, h: int, w: int) -> int:
        return int(self.lib.cave_simt_sp_grid_lds_bytes(h, w))

    def solve(self, costs, h, w, eval_costs=None, flags=F_ALL, seed=0):
        """-> (rc, outputs dict, waves per workgroup).  `flags`: which outputs get a buffer (F_EVAL_COSTS is implied by
        `eval_costs`)."""
        costs, ev = common.f32(costs), common.f32(eval_costs)
        N = costs.shape[0]
        o = common.outputs(TABLE, flags, (N, h, w), guard=0)  # sentinel-filled, in their shapes
        waves = C.c_int32(0)
        rc = self.lib.cave_simt_sp_grid_solve(_p(costs), _p(ev), N, h, w, _p(o["sol"]), _p(o["obj"]), _p(o["eval"]),
                                              _p(o["status"]), _p(o["key"]), _p(o["val"]), seed, C.byref(waves))
        return int(rc), o, int(waves.value)


def run_asan(cases, workdir: str):
    """`cases`: (costs, h, w, eval_costs or None, flags, seed) tuples.  Runs them in ONE process of the sanitizer build and
    returns a list of (rc, outputs dict)."""
    records = []
    for costs, h, w, ev, flags, seed in cases:
        costs, ev = common.f32(costs), common.f32(ev)
        records.append(([costs.shape[0], h, w, common.eval_flag(flags, ev), seed], [costs] + ([] if ev is None else [ev]), flags,
                        (costs.shape[0], h, w)))
    return common.run_asan(build(asan=True), "sp_grid", "sp-grid-ok", TABLE, records, workdir)
