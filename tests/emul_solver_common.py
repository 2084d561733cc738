"""What the loaders of the exact-solver emulation drivers share (emul_sp_grid_lib, emul_tsp_hk_lib, emul_tsp_hk_wide_lib,
emul_vrp_dp_lib; TEST INFRASTRUCTURE ONLY): the two builds of a driver, the sentinel-filled outputs with their guards,
and the run of a stand-alone sanitizer program over a file of cases.

A loader describes its outputs in a table, one row per output in the order of the entry point's arguments and of the
flag bits:  (name, dtype, flag bit, shape function of the case's dimensions).
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from cave_amd import _build

_HERE = os.path.dirname(os.path.abspath(__file__))
F_EVAL_COSTS = 1  # flag bit 1 of every driver: eval_costs is given
GUARD = 8  # sentinel elements behind every guarded output


def build(src: str, main_define: str, asan: bool = False) -> str:
    """tests/emul/<src> -> the shared library for ctypes, or (`asan`) the stand-alone program under AddressSanitizer +
    UBSan with `main_define` set; rebuilt when a file it was compiled from is newer (cave_amd._build)"""
    stem = os.path.splitext(src)[0]
    out = os.path.join(_HERE, "emul", f"_{stem}_asan.exe" if asan else f"_{stem}.so")
    if asan:
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                 "-static-libasan", "-static-libubsan", "-D" + main_define]  # runtimes linked in: the program runs as it is
    else:
        flags = ["-O2", "-fPIC", "-shared"]
    path = os.path.join(_HERE, "emul", src)
    return _build.make(["g++", "-std=c++17", "-w", *flags, "-I" + os.path.join(_HERE, "emul", "simt"), path, "-o", out], path, out)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def n_edges(n: int) -> int:
    return n * (n - 1) // 2


def _fill(dtype):
    return -7 if np.dtype(dtype) == np.int32 else 77.0


def outputs(table, flags: int, dims, guard: int = GUARD):
    """sentinel-filled arrays for the outputs `flags` asks for (None for the others): flat with `guard` extra elements
    behind each, or -- guard 0 -- in their shapes"""
    o = {}
    for name, dtype, bit, shape in table:
        s = shape(*dims)
        o[name] = None if not flags & bit else \
            np.full(int(np.prod(s)) + guard, _fill(dtype), dtype) if guard else np.full(s, _fill(dtype), dtype)
    return o


def untouched(o) -> bool:
    return all(a is None or (a == _fill(a.dtype)).all() for a in o.values())


def strip_guards(table, o, dims, guard: int = GUARD):
    """check the sentinels behind every output and return the outputs in their shapes"""
    r = {}
    for name, dtype, bit, shape in table:
        a = o[name]
        if a is None:
            r[name] = None
            continue
        assert (a[len(a) - guard:] == _fill(dtype)).all(), (name, "written beyond its end")
        r[name] = a[:len(a) - guard].reshape(shape(*dims)).copy()
    return r


def workspace(nbytes: int):
    """-> (0xFF-filled array of exactly that size or None, the size to state)"""
    ws = np.full(nbytes // 8, -1, np.int64) if nbytes >= 8 else None
    return ws, nbytes if ws is not None else 0


def run_asan(exe: str, tag: str, word: str, table, records, workdir: str, timeout: int = 600):
    """Run the cases in ONE process of the sanitizer build `exe` -> a list of (rc, outputs dict).  `records`: per case
    (header: the int64s in front, blobs: the input arrays behind them in file order, flags, dims); the program answers
    with an int32 rc and, rc == 0, the outputs of `table` that `flags` asks for, in table order; it prints `word`."""
    fin, fout = os.path.join(workdir, tag + "_in.bin"), os.path.join(workdir, tag + "_out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.int64(len(records)).tobytes())
        for header, blobs, _, _ in records:
            fh.write(np.asarray(header, np.int64).tobytes())
            for b in blobs:
                fh.write(b.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0 and word in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    res, buf, pos = [], open(fout, "rb").read(), 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(buf, dtype=dtype, count=n, offset=pos).copy()
        pos += a.nbytes
        return a

    for _, _, flags, dims in records:
        rc = int(take(np.int32, 1)[0])
        o = {name: None for name, _, _, _ in table}
        if rc == 0:
            for name, dtype, bit, shape in table:
                if flags & bit:
                    s = shape(*dims)
                    o[name] = take(dtype, int(np.prod(s))).reshape(s)
        res.append((rc, o))
    assert pos == len(buf)
    return res


def eval_flag(flags: int, ev) -> int:
    """`flags` with bit 1 as `ev` says"""
    return (flags & ~F_EVAL_COSTS) | (F_EVAL_COSTS if ev is not None else 0)


# ---- the two Held-Karp tiers (emul_tsp_hk_lib, emul_tsp_hk_wide_lib): one argument list, one output table

F_SOL, F_OBJ, F_EVAL, F_TOUR, F_STATUS = 2, 4, 8, 16, 32
F_ALL = 63
TSP_TABLE = (("sol", np.float32, F_SOL, lambda N, n: (N, n_edges(n))), ("obj", np.float64, F_OBJ, lambda N, n: (N,)),
             ("eval", np.float64, F_EVAL, lambda N, n: (N,)), ("tour", np.int32, F_TOUR, lambda N, n: (N, n)),
             ("status", np.int32, F_STATUS, lambda N, n: (N,)))


def tsp_outputs(N: int, n: int, flags: int):
    """sentinel-filled output arrays (GUARD extra elements behind each) for the outputs `flags` asks for"""
    return outputs(TSP_TABLE, flags, (N, n))


def tsp_strip_guards(o, N: int, n: int):
    """check the sentinels behind every output and return the outputs in their shapes"""
    return strip_guards(TSP_TABLE, o, (N, n))


class SimtTsp:
    """the ctypes face of cave_simt_<entry>_<query>, cave_simt_<entry>_workspace_bytes and cave_simt_<entry>_solve"""

    def __init__(self, lib_path: str, entry: str, queries):
        self.lib = C.CDLL(lib_path)
        self._fn = lambda name: getattr(self.lib, f"cave_simt_{entry}_{name}")
        for name in queries:  # int64 f(int64 n), as methods of their names
            f = self._fn(name)
            f.argtypes, f.restype = [C.c_int64], C.c_int64
            setattr(self, name, lambda n, f=f: int(f(n)))
        self._fn("workspace_bytes").argtypes, self._fn("workspace_bytes").restype = [C.c_int64, C.c_int64], C.c_int64
        self._fn("solve").argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 6 + \
            [C.c_int64, C.c_uint64, C.c_void_p]

    def workspace_bytes(self, n: int, N: int) -> int:
        return int(self._fn("workspace_bytes")(n, N))

    def solve(self, costs, n, eval_costs=None, flags=F_ALL, seed=0, workspace_bytes=None, into=None):
        """-> (rc, outputs dict, workgroups launched).  `flags`: which outputs get a buffer.  `workspace_bytes`: None = the
        size query's default; the workspace is a 0xFF-filled array of exactly that size (none for 0).  `into`: a dict of
        prepared output arrays to use in place of fresh sentinel-filled ones (returned as they are, guards included)."""
        costs, ev = f32(costs), f32(eval_costs)
        N = costs.shape[0]
        o = tsp_outputs(N, n, flags) if into is None else into
        if workspace_bytes is None:
            workspace_bytes = max(self.workspace_bytes(n, N), 0)
        ws, ws_bytes = workspace(workspace_bytes)
        grid = C.c_int32(0)
        rc = self._fn("solve")(_p(costs), _p(ev), N, n, _p(o["sol"]), _p(o["obj"]), _p(o["eval"]), _p(o["tour"]), _p(o["status"]),
                               _p(ws), ws_bytes, seed, C.byref(grid))
        if into is not None:
            return int(rc), o, int(grid.value)
        return int(rc), (tsp_strip_guards(o, N, n) if rc == 0 and N else o), int(grid.value)


def tsp_run_asan(exe: str, tag: str, word: str, cases, workdir: str):
    """`cases`: (costs, n, eval_costs or None, flags, seed, workspace_bytes) tuples -> a list of (rc, outputs dict)"""
    records = []
    for costs, n, ev, flags, seed, wsb in cases:
        costs, ev = f32(costs), f32(ev)
        records.append(([costs.shape[0], n, eval_flag(flags, ev), seed, wsb], [costs] + ([] if ev is None else [ev]), flags,
                        (costs.shape[0], n)))
    return run_asan(exe, tag, word, TSP_TABLE, records, workdir)
