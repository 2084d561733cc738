"""The model-step entries under AddressSanitizer + UBSan (TEST INFRASTRUCTURE ONLY): tests/emul/model_asan_main.cpp,
the SIMT emulation build with the sanitizers' runtimes linked in, run as a program of its own -- one launch per run, the
batch in through a file, the outputs back through a file.  AsanRunner.run has the contract of emul_lib.model_run_host."""

from __future__ import annotations

import os
import subprocess

import numpy as np

import emul_lib as E
import emul_solver_common as common

_SRC = "model_asan_main.cpp"


def build() -> str:
    """the stand-alone sanitizer program, by the recipe the solver emulations share (emul_solver_common.build)"""
    return common.build(_SRC, "MODEL_ASAN_MAIN", asan=True)


class AsanRunner:
    def __init__(self, workdir: str):
        self.exe, self.workdir, self.n = build(), workdir, 0

    def run(self, kind, H, theta, g, nF, reg_rel=0.0, ord_=None, seed=0):
        ins, out, m = E.model_buffers(kind, H, theta, g, ord_, nF)
        B, p = ins["theta"].shape
        nI = p - nF
        self.n += 1
        fin, fout = (os.path.join(self.workdir, f"model_{self.n}_{w}.bin") for w in ("in", "out"))
        with open(fin, "wb") as fh:
            fh.write(np.array([E.PRIM_KINDS[kind], B, p, nF, seed], np.int64).tobytes())
            fh.write(np.float64(reg_rel).tobytes())
            for name in ("H", "theta", "g", "ord"):
                fh.write(ins[name].tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([self.exe, fin, fout], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0 and "model-asan-ok" in r.stdout, (kind, p, nF, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        buf, pos = open(fout, "rb").read(), 0

        def take(dtype, shape):
            nonlocal pos
            a = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape)), offset=pos).reshape(shape).copy()
            pos += a.nbytes
            return a

        rc = int(take(np.int32, (1,))[0])
        assert rc == 0, (rc, kind, p, nF)
        res = {"tc": take(np.float64, (B, p)), "moved": take(np.int32, (B,)), "sact": take(np.uint8, (B, nI)),
               "ss": take(np.float64, (B, nI)), "M": take(np.float64, (B, m))}
        assert pos == len(buf)
        return res
