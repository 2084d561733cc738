#!/usr/bin/env python
"""Margins of the interior-point iterate against its extended-precision restatement -> profiles/ipm_iterate_margins.json.

    python tools/diag/ipm_iterate_margins.py [--gpu] [--no-cpu] [--out profiles/ipm_iterate_margins.json]

Runs tests/test_ipm_iterate_emul.py (CPU tier: serial build, SIMT emulation, the `_rcp24` build) and, with --gpu,
tests/test_gpu_ipm_iterate.py (MI355X) with CAVE_IPM_ITERATE_MARGINS set: every comparison of those files records, per
entry, case family and step count, the worst (error / bound) -- the bound is 2^-24 |ref| + E_k for a float output and
E_k for the double state, E_k = 8 S_k + F_k (tests/ipm_cases.py) --, the largest E_k / sc met, the errors at 24 steps in
units of TOL sc, and whether scaling the prediction by 2^-20 / 2^10 held bit for bit.  Tiers: "emulation",
"emulation_rcp24" (the SIMT_APPROX_RCP build) and "mi355x".  A tier that is not run keeps the figures the file already has.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tier(test_file, extra, out):
    env = dict(os.environ, CAVE_IPM_ITERATE_MARGINS=out)
    subprocess.run([sys.executable, "-m", "pytest", "-q", os.path.join(ROOT, "tests", test_file), *extra], check=True, env=env, cwd=ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipm_iterate_margins.json"))
    args = ap.parse_args(argv)
    out = os.path.abspath(args.out)
    if not args.no_cpu:
        tier("test_ipm_iterate_emul.py", ["-k", "not asan"], out)
    if args.gpu:
        tier("test_gpu_ipm_iterate.py", ["-m", "gpu"], out)
    data = json.load(open(out))
    print(json.dumps({t: max((v for k, v in rec.items() if "|k=" in k and "TOL" not in k), default=0.0) for t, rec in data.items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
