#!/usr/bin/env python
"""The fused step and the lite store in the interior-point mode (inner='ipm'), timed on two trees: one that has the
one-wave interior-point kernels (cave_hip_cone_step_ipm) and its parent, where the mode falls back to the general kernels.

    python tools/diag/ipm_step.py [--tree DIR] [--quick] [--out FILE]        one tree, one process -> one JSON line
    python tools/diag/ipm_step.py --merge P1 B1 P2 B2 ... --out profiles/step_ipm.json
                                                                             the runs of both trees, in the order they ran

`--tree DIR`: import cave_amd from DIR (a checkout of the parent commit with its own built library) instead of this tree.
The two trees are run alternately, process by process, on one device in one session; `--merge` puts their figures side
by side and evaluates the conditions.

Workload: TSP-20, B = 1024, CaVE+ loss + gradient through the loss module with solver_kwargs={'inner': 'ipm'},
max_iter = 3, check=False, four rotating batches of distinct cones out of 4096, predictions fixed per batch.

Forms (each a loop of module calls):
  ipm_chain_dense    module(pred, prep) with prep.then(next dense batch)   (a) on the parent: pack launch + general kernel
  ipm_chain_sparse   the same with SparseCones batches                      (b) on this tree: ONE launch per step
  ipm_store          module(pred, PackedBatch(store, ids))                  (c) the solve-only launch / the packed kernel
  inner_chain_dense  the dense chain in MODE_INNER (the Newton solver)      (d) for scale

Timing: HIP events around groups of `--group` steps; the figure of a repetition is the median group time per step; every
form is repeated `--reps` times, the forms alternating within the process; reported per form: the median of the
repetitions and their spread (max - min).  Every status is examined once per form (asserted OK).
"""

import argparse
import json
import os
import sys
import time


def measure(args):
    tree = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, tree)

    import numpy as np
    import torch

    from cave_amd import _lib, qpsolver, synth
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.dataset import ConeStore, PackedBatch
    from cave_amd.sparse import SparseCones

    assert os.path.abspath(_lib.__file__).startswith(tree), (_lib.__file__, tree)
    _lib.load()
    has_ipm_step = "cave_hip_cone_step_ipm" in _lib.ABI_SYMBOLS
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
    store = ConeStore.from_sparse(SparseCones.from_coo(items, d, m_max=m))
    assert store.lite_slots is not None
    ids = [torch.arange(r * B, (r + 1) * B, device=dev) for r in range(rotate)]

    def module(ipm, check=False):
        kw = dict({"inner": "ipm"} if ipm else {}, check=check)
        return innerConeAlignedCosine(M(), solver="hip", seed=0, reduction="none", solver_kwargs=kw, **({"max_iter": 3} if ipm else {}))

    class Chain:
        """step i solves batch i % rotate and hands batch (i + 1) % rotate to the same call"""

        def __init__(self, batches, ipm):
            self.batches, self.mod, self.i = batches, module(ipm), 0

        def restart(self):
            self.prep = qpsolver.prepare_cones(self.batches[self.i % rotate])
            assert isinstance(self.prep, qpsolver.PreparedCones)

        def step(self):
            r = self.i % rotate
            self.prep.then(self.batches[(r + 1) % rotate])
            loss = self.mod(preds[r], self.prep)
            self.prep, self.i = self.prep.next, self.i + 1
            return loss

    class Store:
        def __init__(self):
            self.mod, self.i = module(True), 0
            self.batches = [PackedBatch(store, i) for i in ids]

        def restart(self):
            pass

        def step(self):
            r = self.i % rotate
            self.i += 1
            return self.mod(preds[r], self.batches[r])

    # one checked pass per form settles the shapes; the losses of the three interior-point forms agree
    ref = {}
    for name, batches, ipm in (("ipm_chain_dense", dense, True), ("ipm_chain_sparse", sparse, True), ("inner_chain_dense", dense, False)):
        mod, outs = module(ipm, check=True), []
        prep = qpsolver.prepare_cones(batches[0])
        for r in range(rotate):
            prep.then(batches[(r + 1) % rotate])
            outs.append(mod(preds[r], prep))
            prep = prep.next
        ref[name] = torch.cat(outs)
    mod = module(True, check=True)
    ref["ipm_store"] = torch.cat([mod(preds[r], PackedBatch(store, ids[r])) for r in range(rotate)])
    agree = max(float((ref[k] - ref["ipm_chain_dense"]).abs().max()) for k in ("ipm_chain_sparse", "ipm_store"))
    assert agree <= 2e-6, agree
    assert bool(torch.isfinite(ref["inner_chain_dense"]).all())

    forms = {"ipm_chain_dense": Chain(dense, True), "ipm_chain_sparse": Chain(sparse, True), "ipm_store": Store(),
             "inner_chain_dense": Chain(dense, False)}

    def rep_us(form):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        form.restart()
        for _ in range(2 * rotate):
            form.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a, b in ev:
            a.record()
            for _ in range(args.group):
                form.step()
            b.record()
        host = (time.perf_counter() - t0) / (args.groups * args.group)
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / args.group for a, b in ev)
        return 1e3 * t[len(t) // 2], 1e6 * host

    samples = {k: [] for k in forms}
    host = {k: [] for k in forms}
    for rep in range(args.reps):
        for k, form in forms.items():
            us, h = rep_us(form)
            samples[k].append(us)
            host[k].append(h)
    res = {"tool": "tools/diag/ipm_step.py", "tree": args.label or ("this tree" if not args.tree else os.path.basename(tree)),
           "has_cave_hip_cone_step_ipm": bool(has_ipm_step), "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": f"TSP-20 B={B}, {rotate} rotating batches of distinct cones, CaVE+ loss + gradient, inner='ipm' max_iter=3, check=False",
           "timing": f"HIP events around groups of {args.group} steps; per repetition the median of {args.groups} groups; "
                     f"{args.reps} repetitions per form, forms alternating in the process; spread = max - min of the repetitions",
           "max_loss_difference_between_the_ipm_forms": agree, "us_per_step": {}}
    for k, v in samples.items():
        s = sorted(v)
        res["us_per_step"][k] = {"median": round(s[len(s) // 2], 2), "spread": round(s[-1] - s[0], 2),
                                 "repetitions": [round(x, 2) for x in v],
                                 "host_enqueue_us_per_step": round(float(np.median(host[k])), 1)}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


def merge(args):
    runs = [json.load(open(p)) for p in args.merge]
    new = [r for r in runs if r["has_cave_hip_cone_step_ipm"]]
    old = [r for r in runs if not r["has_cave_hip_cone_step_ipm"]]
    assert new and old, "need runs of both trees"

    def pooled(rs, form):
        reps = sorted(x for r in rs for x in r["us_per_step"][form]["repetitions"])
        return {"median": reps[len(reps) // 2], "spread": round(reps[-1] - reps[0], 2), "repetitions": reps}

    forms = list(new[0]["us_per_step"])
    out = {"tool": "tools/diag/ipm_step.py --merge", "device": new[0]["device"], "config": new[0]["config"], "timing": new[0]["timing"],
           "order_of_the_processes": [r["tree"] for r in runs],
           "parent": {f: pooled(old, f) for f in forms}, "branch": {f: pooled(new, f) for f in forms}, "runs": runs}
    p, b = out["parent"], out["branch"]

    def faster(x, y):   # x faster than y by more than the recorded spread
        return bool(x["median"] + max(x["spread"], y["spread"]) < y["median"])

    out["figures"] = {
        "a_parent_prefetch_chain_ipm": {"dense": p["ipm_chain_dense"]["median"], "sparse": p["ipm_chain_sparse"]["median"]},
        "b_branch_fused_chain_ipm": {"dense": b["ipm_chain_dense"]["median"], "sparse": b["ipm_chain_sparse"]["median"]},
        "c_store_solve_only": {"parent": p["ipm_store"]["median"], "branch": b["ipm_store"]["median"]},
        "d_inner_chain_dense": {"parent": p["inner_chain_dense"]["median"], "branch": b["inner_chain_dense"]["median"]}}
    out["conditions"] = {"b_faster_than_a_dense": faster(b["ipm_chain_dense"], p["ipm_chain_dense"]),
                         "b_faster_than_a_sparse": faster(b["ipm_chain_sparse"], p["ipm_chain_sparse"]),
                         "c_branch_faster_than_c_parent": faster(b["ipm_store"], p["ipm_store"])}
    print(json.dumps({k: out[k] for k in ("figures", "conditions")}))
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="", help="import cave_amd from this directory (default: the tree of this file)")
    ap.add_argument("--label", default="")
    ap.add_argument("--quick", action="store_true", help="small batches (a functional run of the driver, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--groups", type=int, default=5, help="timed groups per repetition")
    ap.add_argument("--group", type=int, default=40, help="steps per group")
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if args.merge:
        assert args.out
        return merge(args)
    return measure(args)


if __name__ == "__main__":
    sys.exit(main())
