"""Loader for tests/emul/simt_tsp_hk_wide.cpp: the wide Held-Karp tier (cave_amd/csrc/tsp_hk_wide.h) under the SIMT
emulation (TEST INFRASTRUCTURE ONLY).

Two builds of the one unit (emul_solver_common, whose Held-Karp flags, sentinel-filled outputs and guard check serve
both tiers): a shared library for ctypes (`SimtTspHkWide`), and a stand-alone program under AddressSanitizer + UBSan
(`run_asan`: cases go in through a file, results come back through a file; every buffer is a heap block of its exact
size, the LDS blocks and the workspace too).
"""

from __future__ import annotations

import emul_solver_common as common
from emul_solver_common import F_ALL, F_EVAL, F_EVAL_COSTS, F_OBJ, F_SOL, F_STATUS, F_TOUR, GUARD, n_edges  # noqa: F401
from emul_solver_common import tsp_outputs as outputs, tsp_strip_guards as strip_guards  # noqa: F401

_SRC = "simt_tsp_hk_wide.cpp"


def build(asan: bool = False) -> str:
    return common.build(_SRC, "TSP_HK_WIDE_MAIN", asan)


class SimtTspHkWide(common.SimtTsp):
    """slot_bytes(n), header_bytes(n), lds_bytes(n), workspace_bytes(n, N), solve(...)"""

    def __init__(self):
        super().__init__(build(), "tsp_hk_wide", ("slot_bytes", "header_bytes", "lds_bytes"))


def run_asan(cases, workdir: str):
    """`cases`: (costs, n, eval_costs or None, flags, seed, workspace_bytes) tuples.  Runs them in ONE process of the
    sanitizer build and returns a list of (rc, outputs dict)."""
    return common.tsp_run_asan(build(asan=True), "tsp_hk_wide", "tsp-hk-wide-ok", cases, workdir)
