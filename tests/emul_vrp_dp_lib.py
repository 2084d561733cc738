"""Loader for tests/emul/simt_vrp_dp.cpp: the CVRP dynamic-program kernels (cave_amd/csrc/vrp_dp.h) under the SIMT
emulation (TEST INFRASTRUCTURE ONLY).

Two builds of the one unit: a shared library for ctypes (`SimtVrpDp`), and a stand-alone program under AddressSanitizer +
UBSan (`run_asan`: cases go in through a file, results come back through a file; every buffer is a heap block of its
exact size, the LDS block and the workspace too).
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "simt_vrp_dp.cpp")
_DEPS = [_SRC, os.path.join(_HERE, "emul", "simt", "hip", "hip_runtime.h"), os.path.join(_HERE, "..", "include", "cave_hip.h")] + [
    os.path.join(_HERE, "..", "cave_amd", "csrc", n) for n in ("vrp_dp.h", "tsp_hk.h", "cone_common.h")]

F_EVAL_COSTS, F_SOL, F_OBJ, F_EVAL, F_ROUTES, F_STATUS, F_NULL_DEMANDS = 1, 2, 4, 8, 16, 32, 64
F_ALL = 63
GUARD = 8  # sentinel elements behind every output
NAMES = ("sol", "obj", "eval", "routes", "status")


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_simt_vrp_dp_asan.exe" if asan else "_simt_vrp_dp.so")
    newest = max(os.path.getmtime(p) for p in _DEPS)
    if os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    if asan:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                 "-static-libasan", "-static-libubsan", "-DVRP_DP_MAIN"]  # runtimes linked in: the program runs as it is
    else:
        flags = ["-O2", "-fPIC", "-shared"]
    subprocess.run(["g++", "-std=c++17", "-w", *flags, "-I" + os.path.join(_HERE, "emul", "simt"), _SRC, "-o", out], check=True)
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def n_edges(n: int) -> int:
    return n * (n - 1) // 2


def _sizes(N: int, n: int, K: int):
    return {"sol": N * n_edges(n), "obj": N, "eval": N, "routes": N * (n + K), "status": N}


def outputs(N: int, n: int, K: int, flags: int):
    """sentinel-filled output arrays (GUARD extra elements behind each) for the outputs `flags` asks for"""
    size = _sizes(N, n, K)
    dt = {"sol": (np.float32, 77.0, F_SOL), "obj": (np.float64, 77.0, F_OBJ), "eval": (np.float64, 77.0, F_EVAL),
          "routes": (np.int32, -7, F_ROUTES), "status": (np.int32, -7, F_STATUS)}
    return {k: np.full(size[k] + GUARD, dt[k][1], dt[k][0]) if flags & dt[k][2] else None for k in NAMES}


def untouched(o) -> bool:
    return all(a is None or (a == (-7 if a.dtype == np.int32 else 77.0)).all() for a in o.values())


def strip_guards(o, N: int, n: int, K: int):
    """check the sentinels behind every output and return the outputs in their shapes"""
    shape = {"sol": (N, n_edges(n)), "obj": (N,), "eval": (N,), "routes": (N, n + K), "status": (N,)}
    r = {}
    for k, a in o.items():
        if a is None:
            r[k] = None
            continue
        guard = a[len(a) - GUARD:]
        assert (guard == (-7 if a.dtype == np.int32 else 77.0)).all(), (k, "written beyond its end")
        r[k] = a[:len(a) - GUARD].reshape(shape[k]).copy()
    return r


class SimtVrpDp:
    def __init__(self):
        self.lib = C.CDLL(build())
        for name in ("slot_bytes", "lds_bytes", "tier"):
            f = getattr(self.lib, "cave_simt_vrp_dp_" + name)
            f.argtypes, f.restype = [C.c_int64, C.c_int64], (C.c_int32 if name == "tier" else C.c_int64)
        self.lib.cave_simt_vrp_dp_workspace_bytes.argtypes = [C.c_int64] * 3
        self.lib.cave_simt_vrp_dp_workspace_bytes.restype = C.c_int64
        self.lib.cave_simt_vrp_dp_solve.argtypes = [C.c_void_p] * 3 + [C.c_double, C.c_int64, C.c_int64, C.c_int64] + \
            [C.c_void_p] * 6 + [C.c_int64, C.c_uint64, C.c_void_p]

    def slot_bytes(self, n: int, K: int) -> int:
        return int(self.lib.cave_simt_vrp_dp_slot_bytes(n, K))

    def workspace_bytes(self, n: int, K: int, N: int) -> int:
        return int(self.lib.cave_simt_vrp_dp_workspace_bytes(n, K, N))

    def lds_bytes(self, n: int, K: int) -> int:
        return int(self.lib.cave_simt_vrp_dp_lds_bytes(n, K))

    def tier(self, n: int, K: int) -> int:
        return int(self.lib.cave_simt_vrp_dp_tier(n, K))

    def solve(self, costs, n, demands, capacity, K, eval_costs=None, flags=F_ALL, seed=0, workspace_bytes=None, into=None,
              null_costs=False):
        """-> (rc, outputs dict, workgroups launched).  `flags`: which outputs get a buffer.  `workspace_bytes`: None = the
        size query's default; the workspace is a 0xFF-filled array of exactly that size (none for 0).  `into`: a dict of
        prepared output arrays to use in place of fresh sentinel-filled ones (returned as they are, guards included).
        `demands` None: a null pointer."""
        costs = np.ascontiguousarray(costs, dtype=np.float32)
        N = costs.shape[0]
        ev = None if eval_costs is None else np.ascontiguousarray(eval_costs, dtype=np.float32)
        q = None if demands is None else np.ascontiguousarray(demands, dtype=np.float32)
        o = outputs(N, n, K, flags) if into is None else into
        if workspace_bytes is None:
            workspace_bytes = max(self.workspace_bytes(n, K, N), 0)
        ws = np.full(workspace_bytes // 8, -1, np.int64) if workspace_bytes >= 8 else None
        grid = C.c_int32(0)
        rc = self.lib.cave_simt_vrp_dp_solve(None if null_costs else _p(costs), _p(ev), _p(q), float(capacity), K, N, n, _p(o["sol"]),
                                             _p(o["obj"]), _p(o["eval"]), _p(o["routes"]), _p(o["status"]), _p(ws),
                                             workspace_bytes if ws is not None else 0, seed, C.byref(grid))
        if into is not None:
            return int(rc), o, int(grid.value)
        return int(rc), (strip_guards(o, N, n, K) if rc == 0 and N else o), int(grid.value)


def run_asan(cases, workdir: str):
    """`cases`: (costs, n, demands, capacity, K, eval_costs or None, flags, seed, workspace_bytes) tuples.  Runs them in
    ONE process of the sanitizer build and returns a list of (rc, outputs dict)."""
    exe = build(asan=True)
    fin, fout = os.path.join(workdir, "vrp_dp_in.bin"), os.path.join(workdir, "vrp_dp_out.bin")
    norm = []
    with open(fin, "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for costs, n, q, cap, K, ev, flags, seed, wsb in cases:
            costs = np.ascontiguousarray(costs, dtype=np.float32)
            flags = (flags & ~F_EVAL_COSTS) | (F_EVAL_COSTS if ev is not None else 0)
            norm.append((costs, n, K, flags))
            fh.write(np.asarray([costs.shape[0], n, K, flags, seed, wsb], np.int64).tobytes())
            fh.write(np.float64(cap).tobytes())
            fh.write(np.ascontiguousarray(q, dtype=np.float32).tobytes())
            fh.write(costs.tobytes())
            if ev is not None:
                fh.write(np.ascontiguousarray(ev, dtype=np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "vrp-dp-ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    res, buf, pos = [], open(fout, "rb").read(), 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(buf, dtype=dtype, count=n, offset=pos).copy()
        pos += a.nbytes
        return a

    for costs, n, K, flags in norm:
        N, d = costs.shape[0], n_edges(n)
        rc = int(take(np.int32, 1)[0])
        o = dict.fromkeys(NAMES)
        if rc == 0:
            if flags & F_SOL:
                o["sol"] = take(np.float32, N * d).reshape(N, d)
            if flags & F_OBJ:
                o["obj"] = take(np.float64, N)
            if flags & F_EVAL:
                o["eval"] = take(np.float64, N)
            if flags & F_ROUTES:
                o["routes"] = take(np.int32, N * (n + K)).reshape(N, n + K)
            if flags & F_STATUS:
                o["status"] = take(np.int32, N)
        res.append((rc, o))
    assert pos == len(buf)
    return res
