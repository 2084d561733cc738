"""Loader for tests/emul/simt_sp_grid.cpp: the grid shortest-path kernel (cave_amd/csrc/sp_grid.h) under the SIMT
emulation (TEST INFRASTRUCTURE ONLY).

Two builds of the one unit: a shared library for ctypes (`SimtSpGrid`), and a stand-alone program under AddressSanitizer +
UBSan (`run_asan`: cases go in through a file, results come back through a file; every buffer is a heap block of its
exact size, the LDS block too).
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "simt_sp_grid.cpp")
_DEPS = [_SRC, os.path.join(_HERE, "emul", "simt", "hip", "hip_runtime.h"), os.path.join(_HERE, "..", "include", "cave_hip.h")] + [
    os.path.join(_HERE, "..", "cave_amd", "csrc", n) for n in ("sp_grid.h", "wave_prims.h", "cone_common.h")]

F_EVAL_COSTS, F_SOL, F_OBJ, F_EVAL, F_STATUS, F_CONES = 1, 2, 4, 8, 16, 32
F_ALL = 63


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_simt_sp_grid_asan.exe" if asan else "_simt_sp_grid.so")
    newest = max(os.path.getmtime(p) for p in _DEPS)
    if os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    if asan:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                 "-static-libasan", "-static-libubsan", "-DSP_GRID_MAIN"]  # runtimes linked in: the program runs as it is
    else:
        flags = ["-O2", "-fPIC", "-shared"]
    subprocess.run(["g++", "-std=c++17", "-w", *flags, "-I" + os.path.join(_HERE, "emul", "simt"), _SRC, "-o", out], check=True)
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def n_arcs(h: int, w: int) -> int:
    return h * (w - 1) + (h - 1) * w


def _outputs(N: int, d: int, flags: int):
    """sentinel-filled output arrays for the outputs `flags` asks for (None for the others)"""
    o = {"sol": None, "obj": None, "eval": None, "status": None, "key": None, "val": None}
    if flags & F_SOL:
        o["sol"] = np.full((N, d), 77.0, np.float32)
    if flags & F_OBJ:
        o["obj"] = np.full(N, 77.0, np.float64)
    if flags & F_EVAL:
        o["eval"] = np.full(N, 77.0, np.float64)
    if flags & F_STATUS:
        o["status"] = np.full(N, -7, np.int32)
    if flags & F_CONES:
        o["key"] = np.full(N * 5 * d, -7, np.int32)
        o["val"] = np.full(N * 5 * d, 77.0, np.float32)
    return o


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
        costs = np.ascontiguousarray(costs, dtype=np.float32)
        N = costs.shape[0]
        d = n_arcs(h, w)
        ev = None if eval_costs is None else np.ascontiguousarray(eval_costs, dtype=np.float32)
        o = _outputs(N, d, flags)
        waves = C.c_int32(0)
        rc = self.lib.cave_simt_sp_grid_solve(_p(costs), _p(ev), N, h, w, _p(o["sol"]), _p(o["obj"]), _p(o["eval"]),
                                              _p(o["status"]), _p(o["key"]), _p(o["val"]), seed, C.byref(waves))
        return int(rc), o, int(waves.value)


def run_asan(cases, workdir: str):
    """`cases`: (costs, h, w, eval_costs or None, flags, seed) tuples.  Runs them in ONE process of the sanitizer build and
    returns a list of (rc, outputs dict)."""
    exe = build(asan=True)
    fin, fout = os.path.join(workdir, "sp_grid_in.bin"), os.path.join(workdir, "sp_grid_out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.int64(len(cases)).tobytes())
        for costs, h, w, ev, flags, seed in cases:
            costs = np.ascontiguousarray(costs, dtype=np.float32)
            flags = (flags & ~F_EVAL_COSTS) | (F_EVAL_COSTS if ev is not None else 0)
            fh.write(np.asarray([costs.shape[0], h, w, flags, seed], np.int64).tobytes())
            fh.write(costs.tobytes())
            if ev is not None:
                fh.write(np.ascontiguousarray(ev, dtype=np.float32).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sp-grid-ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    res, buf, pos = [], open(fout, "rb").read(), 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(buf, dtype=dtype, count=n, offset=pos).copy()
        pos += a.nbytes
        return a

    for costs, h, w, ev, flags, seed in cases:
        N, d = np.asarray(costs).shape[0], n_arcs(h, w)
        rc = int(take(np.int32, 1)[0])
        o = {"sol": None, "obj": None, "eval": None, "status": None, "key": None, "val": None}
        if rc == 0:
            if flags & F_SOL:
                o["sol"] = take(np.float32, N * d).reshape(N, d)
            if flags & F_OBJ:
                o["obj"] = take(np.float64, N)
            if flags & F_EVAL:
                o["eval"] = take(np.float64, N)
            if flags & F_STATUS:
                o["status"] = take(np.int32, N)
            if flags & F_CONES:
                o["key"] = take(np.int32, N * 5 * d)
                o["val"] = take(np.float32, N * 5 * d)
        res.append((rc, o))
    assert pos == len(buf)
    return res
