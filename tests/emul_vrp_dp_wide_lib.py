"""Loader for tests/emul/simt_vrp_dp_wide.cpp: the wide CVRP tier (cave_amd/csrc/vrp_dp_wide.h, 13 <= n <= 20) under the
SIMT emulation (TEST INFRASTRUCTURE ONLY).  The flags, the output table and the case file are emul_vrp_dp_lib's.

Two builds of the one unit (emul_solver_common): a shared library for ctypes (`SimtVrpDpWide`), and a stand-alone program
under AddressSanitizer + UBSan (`run_asan`: cases go in through a file, results come back through a file; every buffer
is a heap block of its exact size, the LDS block and the workspace too).
"""

from __future__ import annotations

import ctypes as C

import numpy as np

import emul_solver_common as common
from emul_solver_common import F_EVAL_COSTS, GUARD, _p, n_edges, untouched  # noqa: F401
from emul_vrp_dp_lib import F_ALL, F_EVAL, F_NULL_DEMANDS, F_OBJ, F_ROUTES, F_SOL, F_STATUS, NAMES, TABLE, outputs, strip_guards  # noqa: F401

_SRC = "simt_vrp_dp_wide.cpp"


def build(asan: bool = False) -> str:
    return common.build(_SRC, "VRP_DP_WIDE_MAIN", asan)


class SimtVrpDpWide:
    def __init__(self):
        self.lib = C.CDLL(build())
        for name in ("slot_bytes", "lds_bytes", "header_bytes"):
            f = getattr(self.lib, "cave_simt_vrp_dp_wide_" + name)
            f.argtypes, f.restype = [C.c_int64, C.c_int64], C.c_int64
            setattr(self, name, lambda n, K, f=f: int(f(n, K)))
        self.lib.cave_simt_vrp_dp_wide_workspace_bytes.argtypes = [C.c_int64] * 3
        self.lib.cave_simt_vrp_dp_wide_workspace_bytes.restype = C.c_int64
        self.lib.cave_simt_vrp_dp_wide_solve.argtypes = [C.c_void_p] * 3 + [C.c_double, C.c_int64, C.c_int64, C.c_int64] + \
            [C.c_void_p] * 6 + [C.c_int64, C.c_uint64, C.c_void_p]

    def workspace_bytes(self, n: int, K: int, N: int) -> int:
        return int(self.lib.cave_simt_vrp_dp_wide_workspace_bytes(n, K, N))

    def solve(self, costs, n, demands, capacity, K, eval_costs=None, flags=F_ALL, seed=0, workspace_bytes=None, into=None,
              null_costs=False):
        """-> (rc, outputs dict, workgroups launched).  `flags`: which outputs get a buffer.  `workspace_bytes`: None = the
        size query's default; the workspace is a 0xFF-filled array of exactly that size (none for 0).  `into`: a dict of
        prepared output arrays to use in place of fresh sentinel-filled ones (returned as they are, guards included).
        `demands` None: a null pointer."""
        costs, ev, q = common.f32(costs), common.f32(eval_costs), common.f32(demands)
        N = costs.shape[0]
        o = outputs(N, n, K, flags) if into is None else into
        if workspace_bytes is None:
            workspace_bytes = max(self.workspace_bytes(n, K, N), 0)
        ws, ws_bytes = common.workspace(workspace_bytes)
        grid = C.c_int32(0)
        rc = self.lib.cave_simt_vrp_dp_wide_solve(None if null_costs else _p(costs), _p(ev), _p(q), float(capacity), K, N, n, _p(o["sol"]),
                                             _p(o["obj"]), _p(o["eval"]), _p(o["routes"]), _p(o["status"]), _p(ws), ws_bytes, seed,
                                             C.byref(grid))
        if into is not None:
            return int(rc), o, int(grid.value)
        return int(rc), (strip_guards(o, N, n, K) if rc == 0 and N else o), int(grid.value)


def run_asan(cases, workdir: str):
    """`cases`: (costs, n, demands, capacity, K, eval_costs or None, flags, seed, workspace_bytes) tuples.  Runs them in
    ONE process of the sanitizer build and returns a list of (rc, outputs dict)."""
    records = []
    for costs, n, q, cap, K, ev, flags, seed, wsb in cases:
        costs, ev = common.f32(costs), common.f32(ev)
        flags = common.eval_flag(flags, ev)
        records.append(([costs.shape[0], n, K, flags, seed, wsb], [np.float64(cap), common.f32(q), costs] + ([] if ev is None else [ev]),
                        flags, (costs.shape[0], n, K)))
    return common.run_asan(build(asan=True), "vrp_dp_wide", "vrp-dp-wide-ok", TABLE, records, workdir, timeout=900)
