#!/usr/bin/env python
"""The APGD projector (cave_hip_cone_apgd / cave_hip_cone_apgd_sparse) timed at TSP-20, B = 1024, beside the 'push' and
'ipm' steps of the same run.

    python tools/diag/apgd.py [--quick] [--out profiles/apgd.json]

Workload: TSP-20, B = 1024, four rotating batches of distinct cones out of 4096, predictions fixed per batch, CaVE+ loss +
gradient, check=False.

Forms (each a loop of calls):
  apgd_20_dense / apgd_20_sparse      one launch of 20 iterations (cone_op_apgd / cone_op_apgd_sparse, MODE_EXACT)
  apgd_200_dense / apgd_200_sparse    one launch of 200 iterations
  push_dense                          module(pred, ctrs) with the default inner='push' (the Newton solver)
  ipm_dense                           module(pred, ctrs) with inner='ipm', max_iter = 3

Timing (the method of tools/diag/ipm_step.py): HIP events around groups of `--group` calls; the figure of a repetition is
the median group time per call; every form is repeated `--reps` times, the forms alternating within the process;
reported per form: the median of the repetitions and their spread (max - min).  Every status is examined once per form.
No figure here is an acceptance criterion.
"""

import argparse
import json
import os
import sys


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small batches (a functional run of the driver, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--group", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

    import torch

    from cave_amd import _lib, qpsolver, synth
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.sparse import SparseCones

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, rotate = (128 if args.quick else 1024), 4

    class M:
        modelSense = EPO.MINIMIZE

    items, costs, _ = synth.coo_batch("tsp", 20, rotate * B, seed=0)
    d = int(costs.shape[1])
    m = max(it[3] for it in items)
    sparse = [SparseCones.from_coo(items[r * B:(r + 1) * B], d, m_max=m).cuda() for r in range(rotate)]
    dense = [s.densify() for s in sparse]
    preds = [torch.tensor(costs[r * B:(r + 1) * B], device=dev) for r in range(rotate)]
    cap = max(int(s.nnz_per_instance.max()) for s in sparse)

    def apgd(batches, n_iter):
        op = qpsolver.cone_op_apgd if isinstance(batches[0], torch.Tensor) else qpsolver.cone_op_apgd_sparse
        return lambda r, check=False: op(batches[r], preds[r], _lib.MODE_EXACT, -1.0, n_iter=n_iter, nnz_cap=cap, check=check,
                                         outputs=("loss", "grad"))["status"]

    def module(kw, **extra):
        mods = {c: innerConeAlignedCosine(M(), solver="hip", seed=0, reduction="none", solver_kwargs=dict(kw, check=c), **extra)
                for c in (False, True)}

        def call(r, check=False):
            mods[check](preds[r], dense[r])
            return None
        return call

    forms = {"apgd_20_dense": apgd(dense, 20), "apgd_20_sparse": apgd(sparse, 20), "apgd_200_dense": apgd(dense, 200),
             "apgd_200_sparse": apgd(sparse, 200), "push_dense": module({}), "ipm_dense": module({"inner": "ipm"}, max_iter=3)}
    for name, f in forms.items():  # one checked pass per form settles the shapes and examines every status
        for r in range(rotate):
            st = f(r, True)
            assert st is None or bool((st == 0).all()), name

    def rep_us(f):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        for i in range(2 * rotate):
            f(i % rotate)
        torch.cuda.synchronize()
        i = 0
        for a, b in ev:
            a.record()
            for _ in range(args.group):
                f(i % rotate)
                i += 1
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / args.group for a, b in ev)
        return 1e3 * t[len(t) // 2]

    samples = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, f in forms.items():
            samples[k].append(rep_us(f))
    res = {"tool": "tools/diag/apgd.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": f"TSP-20 (m_max {m}, d {d}, at most {cap} entries per instance) B={B}, {rotate} rotating batches of distinct "
                     "cones, loss + gradient, check=False",
           "lds_bytes_per_workgroup": int(lib.cave_hip_apgd_lds_bytes(m, d, cap)),
           "timing": f"HIP events around groups of {args.group} calls; per repetition the median of {args.groups} groups; "
                     f"{args.reps} repetitions per form, forms alternating in the process; spread = max - min of the repetitions",
           "us_per_call": {}}
    for k, v in samples.items():
        s = sorted(v)
        res["us_per_call"][k] = {"median": round(s[len(s) // 2], 2), "spread": round(s[-1] - s[0], 2), "repetitions": [round(x, 2) for x in v]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
