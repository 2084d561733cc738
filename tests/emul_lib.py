"""ctypes loader for the serial gcc build of cave_amd/csrc (TEST INFRASTRUCTURE ONLY).

The build in tests/emul runs the per-instance algorithm code shared with the
HIP kernels on one serial lane, on host memory.  It exists so the CPU-only test
tier (and ASan/UBSan) can exercise that code; the cave_amd package never
imports it.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from cave_amd import _build
from cave_amd._lib import LiteStore, Store, WarmCacheC  # the structs of include/cave_hip.h, here over host arrays

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emul", "emul_abi.cpp")


def build(asan: bool = False) -> str:
    out = os.path.join(_HERE, "emul", "_emul_asan.so" if asan else "_emul.so")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    return _build.make(["g++", "-std=c++17", "-fPIC", "-shared", "-w", *flags, _SRC, "-o", out], _SRC, out)


def outs(B, d):
    """the seven outputs of a cone entry point, zeroed"""
    return {
        "proj": np.zeros((B, d), np.float32), "rnorm": np.zeros(B, np.float32),
        "target": np.zeros((B, d), np.float32), "loss": np.zeros(B, np.float32),
        "grad": np.zeros((B, d), np.float32), "status": np.zeros(B, np.int32),
        "iters": np.zeros(B, np.int32),
    }


def host_store(n_rows, n_nnz, d):
    """Exact-fit host store for the given per-instance counts: (Store, arrays)."""
    B = len(n_rows)
    row_off = np.concatenate([[0], np.cumsum(n_rows, dtype=np.int64)]).astype(np.int64)
    nnz_off = np.concatenate([[0], np.cumsum(n_nnz, dtype=np.int64)]).astype(np.int64)
    R, Z = int(row_off[-1]), int(nnz_off[-1])
    arrs = {
        "row_off": row_off, "nnz_off": nnz_off, "n_valid": np.zeros(B, np.int32), "flags": np.zeros(B, np.uint8),
        "usign": np.zeros(B * d, np.uint8), "avg": np.zeros(B * d, np.float32),
        "vkind": np.zeros(max(R, 1), np.uint8), "rlo": np.zeros(max(R, 1), np.uint32),
        "rhi": np.zeros(max(R, 1), np.uint32), "ccol": np.zeros(max(Z, 1), np.uint16),
        "cval": np.zeros(max(Z, 1), np.float32), "cptr": np.zeros(B * (d + 1), np.uint32),
        "cvar": np.zeros(max(Z, 1), np.uint16), "cvalc": np.zeros(max(Z, 1), np.float32),
    }
    return Store(n=B, d=d, reserved=0, **{k: v.ctypes.data for k, v in arrs.items()}), arrs


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Emul:
    def __init__(self, asan: bool = False):
        self.lib = C.CDLL(build(asan))

    def path_counters(self):
        """[dense-LDL^T instances, ...] since the last call (tests assert that a case took the path it is meant for)."""
        out = (C.c_long * 8)()
        self.lib.cave_emul_path_counters(out)
        return list(out)

    def cone_dense(self, ctrs, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0, nnz_cap=0, lds_bytes=0):
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        B, m, d = ctrs.shape
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        out = outs(B, d)
        rc = self.lib.cave_emul_cone_dense(
            _p(ctrs), _p(pred), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int32(mode),
            C.c_float(sign), C.c_float(inner_ratio), C.c_int32(max_iter), C.c_int32(nnz_cap), C.c_int32(lds_bytes),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out

    def pack(self, ctrs, nnz_cap=0, lds_bytes=0):
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        B, m, d = ctrs.shape
        n_rows = np.zeros(B, np.int32); n_nnz = np.zeros(B, np.int32); status = np.zeros(B, np.int32)
        rc = self.lib.cave_emul_pack_count(_p(ctrs), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int32(nnz_cap),
                                           C.c_int32(lds_bytes), _p(n_rows), _p(n_nnz), _p(status))
        assert rc == 0 and (status == 0).all(), (rc, status)
        st, arrs = host_store(n_rows, n_nnz, d)
        rc = self.lib.cave_emul_pack_fill(_p(ctrs), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int32(nnz_cap),
                                          C.c_int32(lds_bytes), C.byref(st), C.c_int64(0), _p(status))
        assert rc == 0 and (status == 0).all(), (rc, status)
        return st, arrs, int(n_rows.max(initial=0)), int(n_nnz.max(initial=0))

    def cone_packed(self, store, arrs, max_rows, max_nnz, ids, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0):
        d = store.d
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B = len(ids)
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        all_pm1 = int(bool((arrs["flags"] & 1).all()))
        lds = self.lib.cave_emul_packed_lds_bytes(C.c_int64(d), C.c_int32(max_rows), C.c_int32(max_nnz), C.c_int32(all_pm1))
        assert lds > 0
        out = outs(B, d)
        rc = self.lib.cave_emul_cone_packed(
            C.byref(store), _p(ids), _p(pred), C.c_int64(B), C.c_int32(mode), C.c_float(sign),
            C.c_float(inner_ratio), C.c_int32(max_iter), C.c_int32(lds),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out

    # ---- large-cone path (global-workspace arena, band Newton systems)
    def large_slice_bytes(self, m, d, nnz_cap, band):
        self.lib.cave_emul_large_slice_bytes.restype = C.c_int64
        return int(self.lib.cave_emul_large_slice_bytes(C.c_int64(m), C.c_int64(d), C.c_int64(nnz_cap), C.c_int64(band)))

    def cone_dense_large(self, ctrs, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0, nnz_cap=0, band=0,
                         lds_bytes=64 * 1024, slice_bytes=0):
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        B, m, d = ctrs.shape
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        nnz_cap = nnz_cap or max(64, int((ctrs != 0).reshape(B, -1).sum(1).max(initial=0)))
        band = band or 32 * d + 4096
        slice_bytes = slice_bytes or self.large_slice_bytes(m, d, nnz_cap, band)
        out = outs(B, d)
        rc = self.lib.cave_emul_cone_dense_large(
            _p(ctrs), _p(pred), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int32(mode), C.c_float(sign),
            C.c_float(inner_ratio), C.c_int32(max_iter), C.c_int64(nnz_cap), C.c_int32(lds_bytes), C.c_int64(slice_bytes),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out

    def pack_large(self, ctrs, nnz_cap=0, band=0):
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        B, m, d = ctrs.shape
        nnz_cap = nnz_cap or max(64, int((ctrs != 0).reshape(B, -1).sum(1).max(initial=0)))
        slice_bytes = self.large_slice_bytes(m, d, nnz_cap, band or 1)
        n_rows = np.zeros(B, np.int32); n_nnz = np.zeros(B, np.int32); status = np.zeros(B, np.int32)
        rc = self.lib.cave_emul_pack_large(_p(ctrs), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int64(nnz_cap),
                                           C.c_int64(slice_bytes), _p(n_rows), _p(n_nnz), None, C.c_int64(0), _p(status))
        assert rc == 0 and (status == 0).all(), (rc, status)
        st, arrs = host_store(n_rows, n_nnz, d)
        rc = self.lib.cave_emul_pack_large(_p(ctrs), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int64(nnz_cap),
                                           C.c_int64(slice_bytes), None, None, C.byref(st), C.c_int64(0), _p(status))
        assert rc == 0 and (status == 0).all(), (rc, status)
        return st, arrs, int(n_rows.max(initial=0)), int(n_nnz.max(initial=0))

    def cone_packed_large(self, store, arrs, max_rows, ids, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0,
                          band=0, lds_bytes=64 * 1024):
        d = store.d
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B = len(ids)
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        self.lib.cave_emul_packed_large_slice_bytes.restype = C.c_int64
        band = band or max_rows * max_rows
        slice_bytes = int(self.lib.cave_emul_packed_large_slice_bytes(C.c_int64(d), C.c_int64(max_rows), C.c_int64(band)))
        out = outs(B, d)
        rc = self.lib.cave_emul_cone_packed_large(
            C.byref(store), _p(ids), _p(pred), C.c_int64(B), C.c_int32(mode), C.c_float(sign), C.c_float(inner_ratio),
            C.c_int32(max_iter), C.c_int32(lds_bytes), C.c_int64(slice_bytes),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out


# ---- the fused step kernel (cave_amd/csrc/cone_step.h) under the SIMT emulation
LITE_HDR, LITE_ROWPTR, LITE_CSR_WORDS, LITE_RL = 8, 33, 768, 32  # per-slot extents of cave_lite_store
ST_TOO_LARGE, ST_BAD_INPUT, STEP_ZERO_FAILED = 2, 3, 1


def _aligned(n, dtype, fill=0):
    """n elements of dtype on a 16-byte boundary (ell / csr16 / the cache's multipliers)."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + n * item].view(dtype)
    a[...] = fill
    return a


def lite_store(n, d, fill=0):
    """An n-slot lite store of host arrays: (struct, {name: array}).  `fill`: a byte pattern for every array (a test
    then sees what a pack leaves untouched); hdr is zero (state 0: never packed) either way."""
    arrs = {
        "hdr": np.zeros(n * LITE_HDR, np.int32),
        "usign": np.full(n * d, fill, np.uint8),
        "avg": np.zeros(n * d, np.float32),
        "rowptr": np.full(n * LITE_ROWPTR, fill * 0x01010101, np.uint32),
        "ell": _aligned(n * 4 * d, np.uint32, fill * 0x01010101),
        "csr16": _aligned(n * LITE_CSR_WORDS, np.uint32, fill * 0x01010101),
        "rl": np.full(n * LITE_RL, fill, np.uint8),
    }
    st = LiteStore(n=n, d=d, reserved=0, **{k: v.ctypes.data for k, v in arrs.items()})
    return st, arrs


def warm_cache(n):
    arrs = {"key": np.zeros(n, np.uint64), "theta": _aligned(n * 32, np.float32)}
    return WarmCacheC(n_entries=n, key=arrs["key"].ctypes.data, theta=arrs["theta"].ctypes.data), arrs


# ---------------------------------------------------------------------------------------------------------------
# SIMT emulation build (tests/emul/simt_abi.cpp): the GPU-only code paths -- wave contexts, DPP / readlane /
# ballot primitives, the one-wave lite solver, the one-/two-wave band elimination, the blocked dense LDL^T --
# compiled by g++ against a shim <hip/hip_runtime.h> in which every lane is a fiber.  TEST INFRASTRUCTURE ONLY.
_SIMT_SRC = os.path.join(_HERE, "emul", "simt_abi.cpp")


def build_simt(asan: bool = False, defines: tuple = (), tag: str = "", ops: bool = False) -> str:
    """`defines` / `tag`: a variant build (e.g. a tiny spin limit + a withheld hand-over flag) under its own name."""
    out = os.path.join(_HERE, "emul", f"_simt{tag}_asan.so" if asan else f"_simt{tag}.so")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    if not asan and (not defines or ops):  # the operators alone (tests/prims/op_entries.h): the plain build, or on request
        flags.append("-DCAVE_SIMT_OPS")
    cmd = ["g++", "-std=c++17", "-fPIC", "-shared", "-w", *flags, *["-D" + x for x in defines],
           "-I" + os.path.join(_HERE, "emul", "simt"), _SIMT_SRC, "-o", out]
    return _build.make(cmd, _SIMT_SRC, out)


class Simt:
    """Runs the kernels' per-instance code with their real workgroup shapes (1 / 2 / 4 waves of 64 lanes).
    Stores come from Emul.pack / Emul.pack_large (host arrays).  `seed` != 0 shuffles the order in which the lanes
    run between two rendezvous (a hand-over the source does not order then shows up as wrong numbers)."""

    def __init__(self, asan: bool = False, defines: tuple = (), tag: str = "", ops: bool = False):
        self.lib = C.CDLL(build_simt(asan, defines, tag, ops))
        self.lib.cave_simt_packed_large_slice_bytes.restype = C.c_int64

    def path_counters(self):
        out = (C.c_long * 8)()
        self.lib.cave_simt_path_counters(out)
        return list(out)

    def cone_dense(self, ctrs, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0, waves=1, seed=0):
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        B, m, d = ctrs.shape
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        out = outs(B, d)
        rc = self.lib.cave_simt_cone_dense(
            _p(ctrs), _p(pred), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int32(mode), C.c_float(sign),
            C.c_float(inner_ratio), C.c_int32(max_iter), C.c_int32(0), C.c_int32(0), C.c_int32(waves), C.c_uint64(seed),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out

    def pack(self, ctrs, nnz_cap=0, lds_bytes=0, waves=1, seed=0):
        """run_pack_instance on the real workgroup shapes (cave_simt_pack_fill: WaveCtx, BlockCtx<2>, BlockCtx<4>, the
        wide four-wave shape for waves = 8): count pass, then the fill into an exact-fit store of host arrays, as
        Emul.pack does on the serial context -> (store, arrays, status of the count pass, status of the fill pass).
        The multi-thread forms of build_cone -- the team-shared signature scan, the compactions, one wave per long
        row, the atomic CSC fill and its sort -- write this store."""
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        B, m, d = ctrs.shape
        n_rows = np.zeros(B, np.int32); n_nnz = np.zeros(B, np.int32)
        st1 = np.full(B, -7, np.int32); st2 = np.full(B, -7, np.int32)
        head = (_p(ctrs), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_int32(nnz_cap), C.c_int32(lds_bytes),
                C.c_int32(waves), C.c_uint64(seed))
        rc = self.lib.cave_simt_pack_fill(*head, None, C.c_int64(0), _p(n_rows), _p(n_nnz), _p(st1))
        assert rc == 0, rc
        st, arrs = host_store(n_rows, n_nnz, d)
        rc = self.lib.cave_simt_pack_fill(*head, C.byref(st), C.c_int64(0), None, None, _p(st2))
        assert rc == 0, rc
        return st, arrs, st1, st2

    def cone_packed(self, store, arrs, max_rows, max_nnz, ids, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0,
                    waves=1, seed=0, diet=False):
        """diet: launch with the LDS figure of the diet layout (cave_hip_packed_lds_bytes mode 3): instances whose
        ordinary arena exceeds it take that layout (waves = 8 only; the store must carry the signs in its indices)."""
        d = store.d
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B = len(ids)
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        all_pm1 = int(bool((arrs["flags"] & 1).all()))
        lds = self.lib.cave_simt_packed_lds_bytes(C.c_int64(d), C.c_int32(max_rows), C.c_int32(max_nnz),
                                                  C.c_int32(3 if diet else all_pm1))
        assert lds > 0
        out = outs(B, d)
        rc = self.lib.cave_simt_cone_packed(
            C.byref(store), _p(ids), _p(pred), C.c_int64(B), C.c_int32(mode), C.c_float(sign), C.c_float(inner_ratio),
            C.c_int32(max_iter), C.c_int32(lds), C.c_int32(waves), C.c_uint64(seed),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out

    def cone_packed_large(self, store, arrs, max_rows, max_bw, ids, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0,
                          waves=2, seed=0, lds_bytes=0):
        d = store.d
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        B = len(ids)
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        band = max_rows * (max_bw + 1)
        slice_bytes = int(self.lib.cave_simt_packed_large_slice_bytes(C.c_int64(d), C.c_int64(max_rows), C.c_int64(band)))
        lds = lds_bytes or int(self.lib.cave_simt_packed_large_lds_bytes(C.c_int32(max_rows), C.c_int32(max_bw)))
        out = outs(B, d)
        rc = self.lib.cave_simt_cone_packed_large(
            C.byref(store), _p(ids), _p(pred), C.c_int64(B), C.c_int32(mode), C.c_float(sign), C.c_float(inner_ratio),
            C.c_int32(max_iter), C.c_int32(lds), C.c_int32(waves), C.c_int64(slice_bytes), C.c_uint64(seed),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out

    def op_run(self, op, ctx, pm1, cases, seed=0):
        return op_run_host(self.lib, op, ctx, pm1, cases, seed)

    def exact_step(self, x, y, psi0, amax):
        return exact_step_host(self.lib, x, y, psi0, amax)

    def psitol(self):
        self.lib.cave_simt_psitol.restype = C.c_double
        return float(self.lib.cave_simt_psitol())

    def prim_run(self, kind, H, rhs, **kw):
        """one solver alone on a batch of systems (prim_run_host)"""
        return prim_run_host(self.lib, kind, H, rhs, **kw)

    def model_run(self, kind, H, theta, g, nF, **kw):
        """one model minimisation alone on a batch (model_run_host)"""
        return model_run_host(self.lib, kind, H, theta, g, nF, **kw)

    # ---- the fused step kernel (cone_step.h): pack half, solve half (cold / warm), lite_from_packed
    def step_lds_bytes(self, m_max, d):
        """cave_hip_step_lds_bytes of the product (the same step_limits): < 0 = the shape has no such launch."""
        return int(self.lib.cave_simt_step_lds_bytes(C.c_int64(m_max), C.c_int64(d)))

    def lite_scratch_fits(self, d, p, nI):
        """lite_scratch_fits of cone_step.h: does write_lite_slot accept p reduced rows, nI of them with bounds, at dimension d"""
        r = int(self.lib.cave_simt_lite_scratch_fits(C.c_int32(d), C.c_int32(p), C.c_int32(nI)))
        assert r in (0, 3), (d, p, nI, r)   # the rule itself and the table the kernels read say the same
        return r == 3

    def step_pack(self, ctrs, seed=0, fill=0):
        """Pack half of the step kernel (run_pack_lite_instance, two waves): -> (store, arrays, pack status [B])."""
        ctrs = np.ascontiguousarray(ctrs, dtype=np.float32)
        B, m, d = ctrs.shape
        st, arrs = lite_store(B, d, fill)
        status = np.full(B, -7, np.int32)
        rc = self.lib.cave_simt_step_pack(_p(ctrs), C.c_int64(B), C.c_int64(m), C.c_int64(d), C.c_uint64(seed), C.byref(st),
                                          _p(status))
        assert rc == 0, rc
        return st, arrs, status

    def lite_from_packed(self, store, seed=0, fill=0):
        """run_lite_from_packed over every slot of a packed store (Emul.pack): -> (lite store, arrays, status [n])."""
        st, arrs = lite_store(store.n, store.d, fill)
        status = np.full(store.n, -7, np.int32)
        rc = self.lib.cave_simt_lite_from_packed(C.byref(store), C.byref(st), _p(status), C.c_uint64(seed))
        assert rc == 0, rc
        return st, arrs, status

    def step_solve(self, store, pred, mode, sign=-1.0, inner_ratio=0.2, max_iter=0, ids=None, B=None, flags=0,
                         lds_bytes=0, m_max=0, warm=None, keys=None, lds_extra=None, seed=0):
        """Solve half of the step kernel (run_lite_instance on one 64-lane wave per instance).  LDS: `lds_bytes`, or the
        product's figure for a launch with a pack half of m_max rows (0: solve-only).  warm: a WarmCacheC (the warm kernel;
        lds_extra as cave_hip.hip chooses it unless given) -> out["warm_hit"]."""
        d = store.d
        pred = None if pred is None else np.ascontiguousarray(pred, dtype=np.float32)
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int64)
        if B is None:
            B = len(ids) if ids is not None else (len(pred) if pred is not None else store.n)
        lds = lds_bytes or self.step_lds_bytes(m_max, d)
        assert lds > 0, (m_max, d, lds)
        if lds_extra is None:  # what cave_hip.hip launches the warm kernel with (step_warm_lds_extra, cone_step.h)
            lds_extra = int(self.lib.cave_simt_step_warm_lds_extra(C.c_int32(lds), C.c_int32(m_max > 0))) if warm is not None else 0
        keys = None if keys is None else np.ascontiguousarray(keys, dtype=np.int64)
        out = outs(B, d)
        for k in ("proj", "target", "grad"):   # sentinels: what an instance does not write stays visible
            out[k][...] = 77.0
        out["rnorm"][...] = 77.0
        out["loss"][...] = 77.0
        out["status"][...] = -7
        out["iters"][...] = -7
        out["warm_hit"] = np.full(B, 9, np.uint8)
        rc = self.lib.cave_simt_step_solve(
            C.byref(store), _p(ids), _p(pred), C.c_int64(B), C.c_int32(mode), C.c_float(sign), C.c_float(inner_ratio),
            C.c_int32(max_iter), C.c_int32(flags), C.c_int32(lds), C.c_int32(lds_extra),
            None if warm is None else C.byref(warm), _p(keys), _p(out["warm_hit"]), C.c_uint64(seed),
            _p(out["proj"]), _p(out["rnorm"]), _p(out["target"]), _p(out["loss"]), _p(out["grad"]),
            _p(out["status"]), _p(out["iters"]))
        assert rc == 0, rc
        return out


# ---- the linear solvers alone (tests/prims/prim_entries.h): one ABI for the emulation and for tests/prims/_prims.so
class PrimBatch(C.Structure):
    """struct PrimBatch (tests/prims/prim_entries.h)."""
    _fields_ = [
        ("B", C.c_int64), ("p", C.c_int32), ("nF", C.c_int32), ("bw", C.c_int32), ("n_ex", C.c_int32),
        ("reg_rel", C.c_double), ("H", C.c_void_p), ("h_stride", C.c_int64), ("rhs", C.c_void_p), ("act", C.c_void_p),
        ("ex", C.c_void_p), ("x", C.c_void_p), ("M", C.c_void_p), ("m_stride", C.c_int64), ("aux", C.c_void_p),
        ("ws", C.c_void_p), ("ws_stride", C.c_int64), ("fail", C.c_void_p),
        # the model minimisation alone (tests/prims/model_entries.h); NULL for the other entries
        ("theta", C.c_void_p), ("g", C.c_void_p), ("ord", C.c_void_p), ("tc", C.c_void_p), ("moved", C.c_void_p),
        ("sact_out", C.c_void_p), ("ss_out", C.c_void_p),
    ]


PRIM_KINDS = {  # enum of prim_entries.h
    "gj": 0, "gj_lower": 1, "gjs": 2, "gjs_tri": 3, "spd_b2": 4, "spd_b4": 5, "spd_l2": 6, "spd_l4": 7, "spd_solo": 8,
    "tri_l4": 9, "tri_b4": 10, "tri_b2": 11, "partial": 12, "tableau": 13, "dense_w2": 14, "dense_w4": 15,
    "bandw1": 16, "bandw2": 17, "band_hot_w1": 18, "band_hot_l2": 19, "band_hot_l4": 20, "band_cold_l4": 21,
    "lite_model": 22, "dense_model_w1": 23, "dense_model_w2": 24, "dense_model_w4": 25,
}


def prim_m_entries(kind, p, nF):
    """entries per system of the matrix output M of an entry"""
    if kind == "partial":
        return max(1, p * (p - nF))
    if kind == "tableau":
        return 72
    if kind == "lite_model":
        return p * (p | 1)
    if kind.startswith("dense_model"):
        return 1
    if kind.startswith("dense"):
        return ((p + 1) // 2) * (p + 1)
    return 1


def prim_run_host(lib, kind, H, rhs, act=None, reg_rel=0.0, nF=0, bw=0, ex=(), x_in=None, seed=0):
    """One batch through cave_simt_prim_run on host arrays.  H [B, h] in the entry's layout, rhs [B, p]
    -> dict(x [B, p], M [B, m], aux [B, 2 p], fail [B])."""
    k = PRIM_KINDS[kind]
    rhs = np.ascontiguousarray(rhs, np.float64)
    B, p = rhs.shape
    lib.cave_simt_prim_info.restype = C.c_int64
    info = lambda what: int(lib.cave_simt_prim_info(C.c_int32(k), C.c_int32(what), C.c_int32(p), C.c_int32(nF), C.c_int32(bw)))
    hs, ws = info(0), info(1)
    assert hs >= 0, (kind, p, nF, bw)
    H = np.ascontiguousarray(H, np.float64).reshape(B, -1)
    assert H.shape[1] == hs, (H.shape, hs)
    act = np.zeros((B, p), np.uint8) if act is None else np.ascontiguousarray(act, np.uint8)
    ex = np.ascontiguousarray(ex, np.int32)
    m = prim_m_entries(kind, p, nF)
    out = {"x": np.full((B, p), np.nan), "M": np.full((B, m), np.nan), "aux": np.full((B, 2 * p), np.nan),
           "fail": np.full(B, -7, np.int32)}
    if x_in is not None:
        out["x"][...] = x_in
    wsa = np.full((B, max(ws, 1)), np.nan)
    a = PrimBatch(B=B, p=p, nF=nF, bw=bw, n_ex=len(ex), reg_rel=reg_rel, H=H.ctypes.data, h_stride=hs,
                  rhs=rhs.ctypes.data, act=act.ctypes.data, ex=ex.ctypes.data if len(ex) else None, x=out["x"].ctypes.data,
                  M=out["M"].ctypes.data, m_stride=m, aux=out["aux"].ctypes.data, ws=wsa.ctypes.data, ws_stride=max(ws, 1),
                  fail=out["fail"].ctypes.data)
    rc = lib.cave_simt_prim_run(C.c_int32(k), C.byref(a), C.c_uint64(seed))
    assert rc == 0, (rc, kind, p, nF, bw)
    return out


POISON_BITS = 0x7FF8000000ABCDEF  # poison_f64 of tests/prims/prim_entries.h


def model_buffers(kind, H, theta, g, ord_, nF):
    """the arrays of one launch of a model-step entry: inputs as contiguous numpy arrays, outputs preset (tc poisoned,
    moved = -7, sact_out = 0xee, ss_out and M poisoned) -> (inputs, outputs, m)"""
    theta = np.ascontiguousarray(theta, np.float64)
    B, p = theta.shape
    g = np.ascontiguousarray(g, np.float64)
    H = np.ascontiguousarray(H, np.float64).reshape(B, -1)
    ord_ = np.ascontiguousarray(np.tile(np.arange(p, dtype=np.uint16), (B, 1)) if ord_ is None else ord_, np.uint16)
    assert g.shape == (B, p) and ord_.shape == (B, p) and (np.sort(ord_, axis=1) == np.arange(p)).all()
    m, nI = prim_m_entries(kind, p, nF), p - nF
    poison = np.array([POISON_BITS], np.uint64).view(np.float64)[0]
    out = {"tc": np.full((B, p), poison), "moved": np.full(B, -7, np.int32), "sact": np.full((B, max(nI, 1)), 0xEE, np.uint8),
           "ss": np.full((B, max(nI, 1)), poison), "M": np.full((B, m), poison)}
    return {"H": H, "theta": theta, "g": g, "ord": ord_}, out, m


def model_run_host(lib, kind, H, theta, g, nF, reg_rel=0.0, ord_=None, seed=0):
    """One batch through a model-step entry of cave_simt_prim_run on host arrays.  H [B, h]: full rows (lite_model) or
    the folded triangle in elimination order (dense_model_*); theta, g [B, p] in reduced-row order; ord_ [B, p] uint16
    -> dict(tc [B, p], moved [B], sact [B, nI], ss [B, nI], M [B, m])."""
    k = PRIM_KINDS[kind]
    ins, out, m = model_buffers(kind, H, theta, g, ord_, nF)
    B, p = ins["theta"].shape
    lib.cave_simt_prim_info.restype = C.c_int64
    hs = int(lib.cave_simt_prim_info(C.c_int32(k), C.c_int32(0), C.c_int32(p), C.c_int32(nF), C.c_int32(0)))
    assert hs >= 0 and ins["H"].shape[1] == hs, (kind, p, nF, ins["H"].shape, hs)
    a = PrimBatch(B=B, p=p, nF=nF, bw=0, n_ex=0, reg_rel=reg_rel, H=ins["H"].ctypes.data, h_stride=hs, M=out["M"].ctypes.data,
                  m_stride=m, theta=ins["theta"].ctypes.data, g=ins["g"].ctypes.data, ord=ins["ord"].ctypes.data,
                  tc=out["tc"].ctypes.data, moved=out["moved"].ctypes.data, sact_out=out["sact"].ctypes.data,
                  ss_out=out["ss"].ctypes.data)
    rc = lib.cave_simt_prim_run(C.c_int32(k), C.byref(a), C.c_uint64(seed))
    assert rc == 0, (rc, kind, p, nF)
    return out


def store_bandwidth(arrs, B, d):
    """max over instances of the half bandwidth of M M^T in the stored row order (as ConeStore._max_band_entries)."""
    bw = 0
    for b in range(B):
        cp = arrs["cptr"][b * (d + 1):(b + 1) * (d + 1)].astype(np.int64) + int(arrs["nnz_off"][b])
        for k in range(d):
            if cp[k + 1] > cp[k] + 1:
                bw = max(bw, int(arrs["cvar"][cp[k + 1] - 1]) - int(arrs["cvar"][cp[k]]))
    return bw


# ---------------------------------------------------------------------------------------------------------------
# The operators of the Newton loop alone (tests/prims/op_entries.h): struct OpCase, the packing of a list of cases
# into one input blob and the output buffers, and the host runner.  tests/prims/prims_lib.py runs the same blob on cuda:0.
class OpCase(C.Structure):
    """struct OpCase (tests/prims/op_entries.h)."""
    _fields_ = [(n, C.c_int32) for n in ("d", "p", "nnz", "nlong", "nteam", "mode", "flags", "n_seq", "ldh", "empty",
                                         "n_outf", "n_out")] + [
        ("n_in", C.c_int32 * 4), ("s", C.c_double * 4)] + [
        (n, C.c_uint64) for n in ("mptr", "mcol", "mval", "cptr", "cvar", "cvalc", "usign", "vkind", "longrow", "teamrow",
                                  "fin")] + [("in_", C.c_uint64 * 4), ("out", C.c_uint64), ("outf", C.c_uint64),
                                             ("outi", C.c_uint64)]


OP_KINDS = {n: i for i, n in enumerate((
    "gather", "gather_st", "gather_diet", "refresh", "refresh_rb", "dphi", "dphi_rb", "update", "update_rb", "grad",
    "grad_st", "grad_dense", "weight", "band_h", "dense_h", "epilogue", "lite_gather", "lite_grad", "lite_hess",
    "lite_hess_ipm", "ipm_iter", "ipm_lite"))}
OP_CTX = {"w1": 0, "b2": 1, "b4": 2, "l2": 3, "l4": 4, "solo": 5}
OP_VIEW = (("mptr", np.uint32), ("mcol", np.uint16), ("mval", np.float32), ("cptr", np.uint32), ("cvar", np.uint16),
           ("cvalc", np.float32), ("usign", np.uint8), ("vkind", np.uint8), ("longrow", np.uint32), ("teamrow", np.uint32),
           ("fin", np.float32))


def op_kind(op, ctx, pm1):
    return (OP_KINDS[op] * len(OP_CTX) + OP_CTX[ctx]) * 2 + int(bool(pm1))


def op_check_case(c):
    """the index ranges the operators rely on (the kernels do not check them: a bad case must not reach the device)"""
    d, p = int(c["d"]), int(c["p"])
    mptr, cptr = np.asarray(c["mptr"], np.int64), np.asarray(c["cptr"], np.int64)
    nnz = int(mptr[-1])
    assert 1 <= d <= 32767 and 0 <= p <= 32767 and len(mptr) == p + 1 and len(cptr) == d + 1
    assert mptr[0] == 0 and cptr[0] == 0 and (np.diff(mptr) >= 0).all() and (np.diff(cptr) >= 0).all() and cptr[-1] == nnz
    mask = 0x7fff if c["pm1"] else 0xffff
    assert len(c["mcol"]) == nnz and len(c["cvar"]) == nnz
    assert nnz == 0 or ((np.asarray(c["mcol"], np.int64) & mask).max() < d and (np.asarray(c["cvar"], np.int64) & mask).max() < max(p, 1))
    if not c["pm1"]:
        assert len(c["mval"]) == nnz and len(c["cvalc"]) == nnz
    assert len(c["usign"]) == d and len(c["vkind"]) == p and np.asarray(c["usign"]).max(initial=0) <= 3
    assert all(0 <= i < p for i in c["longrow"]) and all(0 <= i < p for i in c["teamrow"])
    assert len(c["fin"]) == 2 * d and len(c["ins"]) <= 4


def op_pack(cases):
    """-> (blob uint8 [n], recs: per case a dict of field -> byte offset into blob, out offsets, sizes).  Every array
    is 16-byte aligned and padded by one element."""
    parts, off, recs = [], 0, []
    n_out = n_outf = 0

    def put(a, dt):
        nonlocal off
        a = np.ascontiguousarray(a, dt).ravel()
        b = np.concatenate([a, np.zeros(1, dt)]).view(np.uint8)
        pad = (-len(b)) % 16
        at = off
        parts.append(np.concatenate([b, np.zeros(pad, np.uint8)]))
        off += len(b) + pad
        return at

    for c in cases:
        op_check_case(c)
        r = {}
        for name, dt in OP_VIEW:
            a = c.get(name)
            r[name] = put(a if a is not None else np.zeros(0, dt), dt)
        r["in_"] = [put(c["ins"][i] if i < len(c["ins"]) else np.zeros(0), np.float64) for i in range(4)]
        r["out"], r["outf"] = n_out, n_outf
        n_out += int(c["n_out"]) + 2
        n_outf += int(c.get("n_outf", 0)) + 2
        recs.append(r)
    return np.concatenate(parts), recs, n_out, n_outf


def op_structs(cases, recs, base, out_base, outf_base, outi_base):
    arr = (OpCase * len(cases))()
    for i, (c, r) in enumerate(zip(cases, recs)):
        k = arr[i]
        k.d, k.p, k.nnz = int(c["d"]), int(c["p"]), int(np.asarray(c["mptr"])[-1])
        k.nlong, k.nteam = len(c["longrow"]), len(c["teamrow"])
        k.mode, k.flags, k.n_seq = int(c.get("mode", 0)), int(c.get("flags", 0)), int(c.get("n_seq", 0))
        k.ldh, k.empty, k.n_outf, k.n_out = int(c.get("ldh", 0)), int(c.get("empty", 0)), int(c.get("n_outf", 0)), int(c["n_out"])
        for j in range(4):
            k.n_in[j] = len(np.ravel(c["ins"][j])) if j < len(c["ins"]) else 0
            k.s[j] = float(c.get("s", (0, 0, 0, 0))[j])
            k.in_[j] = base + r["in_"][j]
        for name, _ in OP_VIEW:
            setattr(k, name, base + r[name])
        k.out, k.outf, k.outi = out_base + 8 * r["out"], outf_base + 4 * r["outf"], outi_base + 16 * i
    return arr


def op_unpack(cases, recs, out, outf, outi):
    return [{"out": out[r["out"]:r["out"] + int(c["n_out"])].copy(),
             "outf": outf[r["outf"]:r["outf"] + int(c.get("n_outf", 0))].copy(), "outi": outi[4 * i:4 * i + 4].copy()}
            for i, (c, r) in enumerate(zip(cases, recs))]


def op_run_host(lib, op, ctx, pm1, cases, seed=0):
    """A batch of cases (dicts, tests/ops_cases.py) through cave_simt_op_run on host arrays -> per case {"out", "outf",
    "outi"}; outputs start as NaN (out, outf) / -7 (outi), so an element that is never written is caught."""
    assert lib.cave_simt_op_case_bytes() == C.sizeof(OpCase)
    blob, recs, n_out, n_outf = op_pack(cases)
    out = np.full(n_out, np.nan)
    outf = np.full(n_outf, np.nan, np.float32)
    outi = np.full(4 * len(cases), -7, np.int32)
    arr = op_structs(cases, recs, blob.ctypes.data, out.ctypes.data, outf.ctypes.data, outi.ctypes.data)
    rc = lib.cave_simt_op_run(C.c_int32(op_kind(op, ctx, pm1)), arr, C.c_int64(len(cases)), C.c_uint64(seed))
    assert rc == 0, (rc, op, ctx, pm1)
    return op_unpack(cases, recs, out, outf, outi)


def exact_step_host(lib, x, y, psi0, amax):
    """exact_step on a piecewise-linear phi' given by its breakpoints -> (alpha, evaluations)"""
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    lib.cave_simt_exact_step.restype = C.c_double
    ne = C.c_int32(0)
    a = lib.cave_simt_exact_step(_p(x), _p(y), C.c_int32(len(x)), C.c_double(psi0), C.c_double(amax), C.byref(ne))
    return float(a), ne.value
