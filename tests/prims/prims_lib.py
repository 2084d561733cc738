"""ctypes loader of tests/prims/_prims.so: the linear solvers of the Newton loop as gfx950 kernels of their own
(TEST INFRASTRUCTURE ONLY; tests/prims/prim_entries.h + prims_abi.hip).  Built with the product's HIPCC_FLAGS against
cave_amd/csrc; torch owns the buffers and the stream.  Nothing under cave_amd/ imports this."""

from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SRC = os.path.join(_HERE, "prims_abi.hip")
_OBJ_DIR = os.path.join(_HERE, "build")
LIB_PATH = os.path.join(_HERE, "_prims.so")
# (object name, extra flags): the entries as the product compiles them, and the dense entries once more with the
# two-columns-per-lane trailing update of cone_dense.h instead of the MFMA one, under the symbol suffix _nomfma
# ... and the operators of the Newton loop (op_entries.h), a unit with a source file of its own
_UNITS = (("prims", ()), ("prims_nomfma", ("-DCAVE_DENSE_NO_MFMA", "-DCAVE_PRIMS_DENSE_ONLY", "-DCAVE_PRIMS_SUFFIX=_nomfma")),
          ("ops", (), "ops_abi.hip"))


def _unit_src(unit):
    return os.path.join(_HERE, unit[2]) if len(unit) > 2 else _SRC


def build(verbose: bool = False) -> str:
    from concurrent.futures import ThreadPoolExecutor

    from cave_amd import _build, _lib

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(_OBJ_DIR, exist_ok=True)
    objs = [os.path.join(_OBJ_DIR, u[0] + ".o") for u in _UNITS]
    todo = [(o, u[1], _unit_src(u)) for o, u in zip(objs, _UNITS) if _build.stale(o)]
    if not todo and not _build.older(LIB_PATH, objs):
        return LIB_PATH

    def compile_one(job):
        obj, extra, src = job
        cmd = [hipcc, *_lib.HIPCC_FLAGS, "-I" + _lib._CSRC, "-I" + os.path.join(_ROOT, "include"), "-I" + _HERE, *extra,
               "-c", src, "-o", obj]
        _build.run(cmd, src, obj, verbose)

    with ThreadPoolExecutor(max_workers=3) as ex:
        list(ex.map(compile_one, todo))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", *objs, "-o", LIB_PATH], check=True)
    return LIB_PATH


class Prims:
    """run(kind, ...) with the contract of emul_lib.prim_run_host, on cuda:0.  nomfma: the dense entries built with
    CAVE_DENSE_NO_MFMA (the other entries exist in one form only)."""

    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # torch first: _prims.so then binds to the HIP runtime torch has loaded.  Loaded before torch (a test file of this
        # tier run on its own), the library brings in a second copy of the runtime, whose calls return hipErrorNoDevice
        import torch  # noqa: F401

        self.lib = C.CDLL(LIB_PATH)
        self.lib.cave_prims_info.restype = C.c_int64

    def run(self, kind, H, rhs, act=None, reg_rel=0.0, nF=0, bw=0, ex=(), x_in=None, seed=0, nomfma=False):
        import torch

        from emul_lib import PRIM_KINDS, PrimBatch, prim_m_entries

        dev = torch.device("cuda:0")
        k = PRIM_KINDS[kind]
        rhs = np.ascontiguousarray(rhs, np.float64)
        B, p = rhs.shape
        info = lambda what: int(self.lib.cave_prims_info(C.c_int32(k), C.c_int32(what), C.c_int32(p), C.c_int32(nF), C.c_int32(bw)))
        hs, ws = info(0), max(info(1), 1)
        assert hs >= 0, (kind, p, nF, bw)
        H = np.ascontiguousarray(H, np.float64).reshape(B, -1)
        assert H.shape[1] == hs, (H.shape, hs)
        m = prim_m_entries(kind, p, nF)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        tH, trhs = t(H, np.float64), t(rhs, np.float64)
        tact = t(np.zeros((B, p), np.uint8) if act is None else act, np.uint8)
        tex = t(np.asarray(ex if len(ex) else [0], np.int32), np.int32)
        tx = t(np.full((B, p), np.nan) if x_in is None else x_in, np.float64)
        tM = torch.full((B, m), float("nan"), dtype=torch.float64, device=dev)
        taux = torch.full((B, 2 * p), float("nan"), dtype=torch.float64, device=dev)
        tws = torch.full((B, ws), float("nan"), dtype=torch.float64, device=dev)
        tfail = torch.full((B,), -7, dtype=torch.int32, device=dev)
        a = PrimBatch(B=B, p=p, nF=nF, bw=bw, n_ex=len(ex), reg_rel=reg_rel, H=tH.data_ptr(), h_stride=hs,
                      rhs=trhs.data_ptr(), act=tact.data_ptr(), ex=tex.data_ptr(), x=tx.data_ptr(), M=tM.data_ptr(),
                      m_stride=m, aux=taux.data_ptr(), ws=tws.data_ptr(), ws_stride=ws, fail=tfail.data_ptr())
        fn = self.lib.cave_prims_run_nomfma if nomfma else self.lib.cave_prims_run
        rc = fn(C.c_int32(k), C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (rc, kind, p, nF, bw)
        torch.cuda.synchronize()
        return {"x": tx.cpu().numpy(), "M": tM.cpu().numpy(), "aux": taux.cpu().numpy(), "fail": tfail.cpu().numpy()}

    def model_run(self, kind, H, theta, g, nF, reg_rel=0.0, ord_=None, seed=0, nomfma=False):
        """the contract of emul_lib.model_run_host, on cuda:0 (seed: ignored, the hardware schedules)"""
        import torch

        import emul_lib as E

        dev = torch.device("cuda:0")
        k = E.PRIM_KINDS[kind]
        ins, out, m = E.model_buffers(kind, H, theta, g, ord_, nF)
        B, p = ins["theta"].shape
        hs = int(self.lib.cave_prims_info(C.c_int32(k), C.c_int32(0), C.c_int32(p), C.c_int32(nF), C.c_int32(0)))
        assert hs >= 0 and ins["H"].shape[1] == hs, (kind, p, nF, ins["H"].shape, hs)
        assert not nomfma or kind.startswith("dense_model")
        ti = {n: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev) for n, a in ins.items()}  # (same bits)
        to = {n: torch.from_numpy(a).to(dev) for n, a in out.items()}
        a = E.PrimBatch(B=B, p=p, nF=nF, bw=0, n_ex=0, reg_rel=reg_rel, H=ti["H"].data_ptr(), h_stride=hs, M=to["M"].data_ptr(),
                        m_stride=m, theta=ti["theta"].data_ptr(), g=ti["g"].data_ptr(), ord=ti["ord"].data_ptr(),
                        tc=to["tc"].data_ptr(), moved=to["moved"].data_ptr(), sact_out=to["sact"].data_ptr(),
                        ss_out=to["ss"].data_ptr())
        fn = self.lib.cave_prims_run_nomfma if nomfma else self.lib.cave_prims_run
        rc = fn(C.c_int32(k), C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (rc, kind, p, nF)
        torch.cuda.synchronize()
        return {n: t.cpu().numpy() for n, t in to.items()}

    def op_run(self, op, ctx, pm1, cases, seed=0):
        """the contract of emul_lib.op_run_host, on cuda:0 (seed: ignored, the hardware schedules)"""
        import torch

        import emul_lib as E

        dev = torch.device("cuda:0")
        assert self.lib.cave_ops_case_bytes() == C.sizeof(E.OpCase)
        blob, recs, n_out, n_outf = E.op_pack(cases)
        tblob = torch.from_numpy(blob).to(dev)
        tout = torch.full((n_out,), float("nan"), dtype=torch.float64, device=dev)
        toutf = torch.full((max(n_outf, 1),), float("nan"), dtype=torch.float32, device=dev)
        touti = torch.full((4 * len(cases),), -7, dtype=torch.int32, device=dev)
        arr = E.op_structs(cases, recs, tblob.data_ptr(), tout.data_ptr(), toutf.data_ptr(), touti.data_ptr())
        raw = np.frombuffer(bytes(arr), np.uint8)
        tcases = torch.from_numpy(raw.copy()).to(dev)
        rc = self.lib.cave_ops_run(C.c_int32(E.op_kind(op, ctx, pm1)), arr, C.c_void_p(tcases.data_ptr()), C.c_int64(len(cases)),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (rc, op, ctx, pm1, self.lib.cave_ops_last_refusal(0), self.lib.cave_ops_last_refusal(1))
        torch.cuda.synchronize()
        return E.op_unpack(cases, recs, tout.cpu().numpy(), toutf.cpu().numpy(), touti.cpu().numpy())
