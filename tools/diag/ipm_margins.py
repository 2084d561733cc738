#!/usr/bin/env python
"""Margins of the interior-point fused step against the existing general kernel -> profiles/step_ipm_margins.json.

    python tools/diag/ipm_margins.py [--gpu] [--out profiles/step_ipm_margins.json]

Runs tests/test_step_ipm_emul.py (CPU tier, SIMT emulation) and, with --gpu, tests/test_gpu_step_ipm.py (MI355X) with
CAVE_IPM_MARGINS_OUT set: every comparison of those files records, per input, the worst normalised difference between
the new kernel and the general kernel (differences divided by max(1, |y|_inf), max(1, rnorm) or 1, as
tests/step_ipm_cases.py states: a figure of 2e-6 is the whole bound), the general kernel's own spread
between one wave and four waves per instance, and the bound that followed from it.  A tier that is not run keeps the
figures the output file already has.
"""

import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tier(test_file, extra):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "margins.json")
        env = dict(os.environ, CAVE_IPM_MARGINS_OUT=path)
        subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", os.path.join(ROOT, "tests", test_file), *extra], check=True,
                       env=env, cwd=ROOT)
        return json.load(open(path))


def summary(rec):
    return {"inputs": len(rec), "worst": max(v["worst"] for v in rec.values()), "spread": max(v["spread"] for v in rec.values()),
            "widened_bounds": sorted(k for k, v in rec.items() if any(b > 2e-6 for b in v["bound"].values()))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_ipm_margins.json"))
    args = ap.parse_args(argv)
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["tool"] = "tools/diag/ipm_margins.py"
    out["bound"] = "2e-6 on the normalised difference; 4 x the general kernel's 1-vs-4-wave spread where that exceeds 5e-7"
    if not args.no_cpu:
        rec = tier("test_step_ipm_emul.py", ["-k", "not asan"])
        out["cpu"] = {"reference": "Emul().cone_dense (serial build of the general kernel)", "summary": summary(rec), "per_input": rec}
    if args.gpu:
        rec = tier("test_gpu_step_ipm.py", ["-m", "gpu"])
        out["gpu"] = {"reference": "cone_op_dense(..., MODE_IPM, waves=1)", "summary": summary(rec), "per_input": rec}
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(json.dumps({k: out[k]["summary"] for k in ("cpu", "gpu") if k in out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
