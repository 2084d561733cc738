"""Loader for tests/emul/simt_tsp_hk_wide.cpp: the wide Held-Karp tier (cave_amd/csrc/tsp_hk_wide.h) under the SIMT
emulation (TEST INFRASTRUCTURE ONLY).

Two builds of the one unit, as tests/emul_tsp_hk_lib.py (whose flags, sentinel-filled outputs and guard check are used
here): a shared library for ctypes (`SimtTspHkWide`), and a stand-alone program under AddressSanitizer + UBSan
(`run_asan`: cases go in through a file, results come back through a file; every buffer is a heap block of its exact
size, the LDS blocks and the workspace too).
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from emul_tsp_hk_lib import F_ALL, F_EVAL, F_EVAL_COSTS, F_OBJ, F_SOL, F_STATUS, F_TOUR, n_edges, outputs, strip_guards  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "simt_tsp_hk_wide.cpp")
_DEPS = [_SRC, os.path.join(_HERE, "emul", "simt", "hip", "hip_runtime.h"), os.path.join(_HERE, "..", "include", "cave_hip.h")] + [
    os.path.join(_HERE, "..", "cave_amd", "csrc", n) for n in ("tsp_hk_wide.h", "cone_common.h")]


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_simt_tsp_hk_wide_asan.exe" if asan else "_simt_tsp_hk_wide.so")
    newest = max(os.path.getmtime(p) for p in _DEPS)
    if os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    if asan:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                 "-static-libasan", "-static-libubsan", "-DTSP_HK_WIDE_MAIN"]  # runtimes linked in: the program runs as it is
    else:
        flags = ["-O2", "-fPIC", "-shared"]
    subprocess.run(["g++", "-std=c++17", "-w", *flags, "-I" + os.path.join(_HERE, "emul", "simt"), _SRC, "-o", out], check=True)
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class SimtTspHkWide:
    def __init__(self):
        self.lib = C.CDLL(build())
        for name in ("slot_bytes", "header_bytes", "lds_bytes"):
            f = getattr(self.lib, "cave_simt_tsp_hk_wide_" + name)
            f.argtypes, f.restype = [C.c_int64], C.c_int64
        self.lib.cave_simt_tsp_hk_wide_workspace_bytes.argtypes = [C.c_int64, C.c_int64]
        self.lib.cave_simt_tsp_hk_wide_workspace_bytes.restype = C.c_int64
        self.lib.cave_simt_tsp_hk_wide_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 6 + \
            [C.c_int64, C.c_uint64, C.c_void_p]

    def slot_bytes(self, n: int) -> int:
        return int(self.lib.cave_simt_tsp_hk_wide_slot_bytes(n))

    def header_bytes(self, n: int) -> int:
        return int(self.lib.cave_simt_tsp_hk_wide_header_bytes(n))

    def workspace_bytes(self, n: int, N: int) -> int:
        return int(self.lib.cave_simt_tsp_hk_wide_workspace_bytes(n, N))

    def lds_bytes(self, n: int) -> int:
        return int(self.lib.cave_simt_tsp_hk_wide_lds_bytes(n))

    def solve(self, costs, n, eval_costs=None, flags=F_ALL, seed=0, workspace_bytes=None, into=None):
        """-> (rc, outputs dict, workgroups launched).  `flags`: which outputs get a buffer.  `workspace_bytes`: None = the
        size query's default; the workspace is a 0xFF-filled array of exactly that size (none for 0).  `into`: a dict of
        prepared output arrays to use in place of fresh sentinel-filled ones (returned as they are, guards included)."""
        costs = np.ascontiguousarray(costs, dtype=np.float32)
        N = costs.shape[0]
        ev = None if eval_costs is None else np.ascontiguousarray(eval_costs, dtype=np.float32)
        o = outputs(N, n, flags) if into is None else into
        if workspace_bytes is None:
            workspace_bytes = max(self.workspace_bytes(n, N), 0)
        ws = np.full(workspace_bytes // 8, -1, np.int64) if workspace_bytes >= 8 else None
        grid = C.c_int32(0)
        rc = self.lib.cave_simt_tsp_hk_wide_solve(_p(costs), _p(ev), N, n, _p(o["sol"]), _p(o["obj"]), _p(o["eval"]), _p(o["tour"]),
                                                  _p(o["status"]), _p(ws), workspace_bytes if ws is not None else 0, seed,
                                                  C.byref(grid))
        if into is not None:
            return int(rc), o, int(grid.value)
        return int(rc), (strip_guards(o, N, n) if rc == 0 and N else o), int(grid.value)


def run_asan(cases, workdir: str):
    """`cases`: (costs, n, eval_costs or None, flags, seed, workspace_bytes) tuples.  Runs them in ONE process of the
    sanitizer build and returns a list of (rc, outputs dict)."""
    exe = build(asan=True)
    fin, fout = os.path.join(workdir, "tsp_hk_wide_in.bin"), os.path.join(workdir, "tsp_hk_wide_out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for costs, n, ev, flags, seed, wsb in cases:
            costs = np.ascontiguousarray(costs, dtype=np.float32)
            flags = (flags & ~F_EVAL_COSTS) | (F_EVAL_COSTS if ev is not None else 0)
            fh.write(np.asarray([costs.shape[0], n, flags, seed, wsb], np.int64).tobytes())
            fh.write(costs.tobytes())
            if ev is not None:
                fh.write(np.ascontiguousarray(ev, dtype=np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "tsp-hk-wide-ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    res, buf, pos = [], open(fout, "rb").read(), 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(buf, dtype=dtype, count=n, offset=pos).copy()
        pos += a.nbytes
        return a

    for costs, n, ev, flags, seed, wsb in cases:
        N, d = np.asarray(costs).shape[0], n_edges(n)
        rc = int(take(np.int32, 1)[0])
        o = {"sol": None, "obj": None, "eval": None, "tour": None, "status": None}
        if rc == 0:
            if flags & F_SOL:
                o["sol"] = take(np.float32, N * d).reshape(N, d)
            if flags & F_OBJ:
                o["obj"] = take(np.float64, N)
            if flags & F_EVAL:
                o["eval"] = take(np.float64, N)
            if flags & F_TOUR:
                o["tour"] = take(np.int32, N * n).reshape(N, n)
            if flags & F_STATUS:
                o["status"] = take(np.int32, N)
        res.append((rc, o))
    assert pos == len(buf)
    return res
