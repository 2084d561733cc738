"""The interior-point entries under AddressSanitizer + UBSan (TEST INFRASTRUCTURE ONLY): tests/emul/ipm_asan_main.cpp,
the SIMT emulation build with the operators and the sanitizers' runtimes linked in, run as a program of its own -- one
launch per run, the cases in through a file, the outputs back through a file.  AsanRunner.op_run has the contract of
emul_lib.op_run_host for the entries of tests/prims/ipm_entries.h (double outputs only).  Nothing is loaded into Python."""

from __future__ import annotations

import os
import subprocess

import numpy as np

import emul_lib as E
import emul_solver_common as common

_SRC = "ipm_asan_main.cpp"


def build() -> str:
    """the stand-alone sanitizer program, by the recipe the solver emulations share (emul_solver_common.build)"""
    return common.build(_SRC, "IPM_ASAN_MAIN", asan=True)


class AsanRunner:
    def __init__(self, workdir: str):
        self.exe, self.workdir, self.n = build(), workdir, 0

    def op_run(self, op, ctx, pm1, cases, seed=0):
        blob, recs, n_out, n_outf = E.op_pack(cases)
        assert n_outf == 2 * len(cases), "double outputs only"
        self.n += 1
        fin, fout = (os.path.join(self.workdir, f"ipm_{self.n}_{w}.bin") for w in ("in", "out"))
        with open(fin, "wb") as fh:
            fh.write(np.array([E.op_kind(op, ctx, pm1), len(cases), len(blob), n_out, seed], np.int64).tobytes())
            for c, r in zip(cases, recs):
                ints = [c["d"], c["p"], int(np.asarray(c["mptr"])[-1]), len(c["longrow"]), len(c["teamrow"]), c.get("mode", 0),
                        c.get("flags", 0), c.get("n_seq", 0), c.get("ldh", 0), c.get("empty", 0), 0, c["n_out"]]
                ints += [len(np.ravel(c["ins"][j])) if j < len(c["ins"]) else 0 for j in range(4)]
                ints += [r[name] for name, _ in E.OP_VIEW] + list(r["in_"]) + [r["out"]]
                assert len(ints) == 32
                fh.write(np.array(ints, np.int64).tobytes())
            fh.write(blob.tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:detect_stack_use_after_return=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([self.exe, fin, fout], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and "ipm-asan-ok" in r.stdout, (op, ctx, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        buf = open(fout, "rb").read()
        rc = int(np.frombuffer(buf, np.int32, 1)[0])
        assert rc == 0, (rc, op, ctx, pm1)
        out = np.frombuffer(buf, np.float64, n_out, 4).copy()
        outi = np.frombuffer(buf, np.int32, 4 * len(cases), 4 + 8 * n_out).copy()
        assert 4 + 8 * n_out + 16 * len(cases) == len(buf)
        return E.op_unpack(cases, recs, out, np.zeros(n_outf, np.float32), outi)
