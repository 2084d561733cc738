"""Loader for tests/emul/simt_tight_cones.cpp: the tight-cone kernels (cave_amd/csrc/tight_cones.h) under the SIMT
emulation (TEST INFRASTRUCTURE ONLY).

Two builds of the one unit (emul_solver_common): a shared library for ctypes (`SimtTightCones`), and a stand-alone
program under AddressSanitizer + UBSan (`run_asan`: cases go in through a file, results come back through a file; every
buffer is a heap block of its exact size).  A system is a `tight_cones_cases.RawSys` of numpy arrays.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

import emul_solver_common as common
from cave_amd._lib import LinSystemC
from emul_solver_common import _p

_SRC = "simt_tight_cones.cpp"

TABLE = (("n_rows", np.int32, 1, lambda N, cap: (N,)), ("n_ent", np.int64, 1, lambda N, cap: (N,)),
         ("status", np.int32, 1, lambda N, cap: (N,)), ("fill_status", np.int32, 1, lambda N, cap: (N,)),
         ("key", np.int32, 1, lambda N, cap: (cap,)), ("val", np.float32, 1, lambda N, cap: (cap,)))


def build(asan: bool = False) -> str:
    return common.build(_SRC, "TIGHT_CONES_MAIN", asan)


def c_system(s):
    """struct cave_lin_system over the arrays of a RawSys (which must outlive the call), or None"""
    if s is None:
        return None
    return LinSystemC(R=s.R, Z=s.Z, d=s.d, reserved=0, **{k: (getattr(s, k).ctypes.data if getattr(s, k) is not None else None)
                                                            for k in ("row_off", "col", "coef", "sense", "rhs")})


def _ref(c):
    return None if c is None else C.byref(c)


class SimtTightCones:
    def __init__(self):
        self.lib = C.CDLL(build())
        S = C.POINTER(LinSystemC)
        self.lib.cave_simt_tight_cones_count.argtypes = [S, S, C.c_void_p, C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 3 + [C.c_uint64]
        self.lib.cave_simt_tight_cones_fill.argtypes = [S, S, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_int64] + \
            [C.c_void_p] * 3 + [C.c_uint64]

    def count(self, sys, lazy, lazy_off, sol, N, tol, n_rows, n_ent, status, seed=0):
        """the raw entry: numpy arrays (or None) as they are"""
        return int(self.lib.cave_simt_tight_cones_count(_ref(c_system(sys)), _ref(c_system(lazy)), _p(lazy_off), _p(sol), N, tol,
                                                        _p(n_rows), _p(n_ent), _p(status), seed))

    def fill(self, sys, lazy, lazy_off, sol, N, tol, ent_off, ent_cap, key, val, status, seed=0):
        return int(self.lib.cave_simt_tight_cones_fill(_ref(c_system(sys)), _ref(c_system(lazy)), _p(lazy_off), _p(sol), N, tol,
                                                       _p(ent_off), ent_cap, _p(key), _p(val), _p(status), seed))

    def run(self, case, seed=0):
        """both passes of a tight_cones_cases.Case on sentinel-filled outputs -> (rc, outputs dict as tight_cones_cases.check
        takes it)"""
        import tight_cones_cases as TC

        return TC.two_passes(case, lambda *a: self.count(*a, seed=seed), lambda *a: self.fill(*a, seed=seed), lambda a: a, lambda a: a)


def run_asan(cases, workdir: str, seed: int = 11):
    """`cases`: (tight_cones_cases.Case, cap) pairs, cap the entries of the key / val blocks.  Runs them in ONE process of
    the sanitizer build and returns a list of (rc, outputs dict)."""
    records = []
    for case, cap in cases:
        s, lz = case.sys, case.lazy
        N = case.sol.shape[0]
        flags = (1 if lz is not None else 0) | (2 if case.lazy_off is not None else 0)
        hdr = [N, s.d, s.R, s.Z, lz.R if lz is not None else 0, lz.Z if lz is not None else 0, flags, seed, cap,
               int(np.float64(case.tol).view(np.int64))]
        blobs = []
        for t in (s, lz):
            if t is not None:
                blobs += [t.row_off, t.col, t.coef, t.sense, t.rhs]
        if case.lazy_off is not None:
            blobs.append(case.lazy_off)
        blobs.append(case.sol)
        records.append((hdr, blobs, 1, (N, cap)))
    return common.run_asan(build(asan=True), "tight_cones", "tight-cones-ok", TABLE, records, workdir)
