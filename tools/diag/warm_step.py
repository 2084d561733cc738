"""Warm start of the fused step, timed: TSP-20 at B = 1024 with predictions drifting slowly (N(0, 0.01) per step),
cold against solver_kwargs={"warm_start": True}, in both forms of the fused step:
  prefetch   cave_amd.dataset.prefetch(loader): ONE step-kernel launch per loss call (solve of this batch + pack of the next)
  dense      a plain dense tensor per loss call: the split form (pack-only launch, then the solve launch; cold: the
             general operator's split form, warm: the step kernel's)
Prints one JSON line per form: wall-clock us per step (loss forward only, fastest of `--reps` timed runs), GPU kernel
time per step (torch.profiler: the sum of the device times of every kernel of a step, averaged over the steps of one
run), mean Newton iterations and, warm, the hit rate.

    python tools/diag/warm_step.py [--batch 1024] [--steps 20] [--reps 5]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch


def _kernel_us(fn, steps):
    """Device time of every kernel launched by fn(), per step (torch.profiler, device activity)."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    tot, names = 0.0, {}
    for e in prof.events():
        dt = getattr(e, "device_time", None)
        if dt is None:
            dt = getattr(e, "cuda_time", 0.0)
        if getattr(e, "device_type", None) is not None and "CUDA" in str(e.device_type) and dt:
            tot += dt
            k = e.name.split("(")[0][:60]
            names[k] = names.get(k, 0.0) + dt / steps
    return tot / steps, {k: round(v, 1) for k, v in sorted(names.items(), key=lambda kv: -kv[1])[:4]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    from cave_amd import synth
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.dataset import prefetch

    class M:
        modelSense = EPO.MINIMIZE

    ctrs, costs, _ = synth.tsp_batch(20, args.batch, seed=0)
    c = torch.tensor(ctrs, device="cuda")
    rng = np.random.default_rng(1)
    preds = [torch.tensor(costs, device="cuda")]
    for _ in range(args.steps - 1):
        preds.append(preds[-1] + torch.tensor(rng.normal(0, 0.01, costs.shape).astype(np.float32), device="cuda"))
    for form in ("prefetch", "dense"):
        res = {"metric": "warm_fused_step", "form": form, "batch": args.batch, "steps": args.steps}
        for tag, kw in (("cold", {}), ("warm", {"warm_start": True})):
            mod = innerConeAlignedCosine(M(), solver="hip", seed=0, solver_kwargs=dict(kw, check=False))
            its, hits = [], []

            def run(diag=False):
                batches = prefetch([(p, c) for p in preds]) if form == "prefetch" else [(p, c) for p in preds]
                for p, cones in batches:
                    mod(p, cones)
                    if diag and tag == "warm":
                        its.append(float(mod._warm.last_iters.float().mean()))
                        hits.append(float(mod._warm.last_hit.float().mean()))

            run()   # warm-up (warm: fills the cache)
            best = float("inf")
            for rep in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t0) / args.steps)
            kern, top = _kernel_us(run, args.steps)
            run(diag=True)
            if tag == "cold":   # iterations of the cold step kernel (no cache), per batch
                from cave_amd.qpsolver import MODE_INNER, cone_op_prepared, prepare_dense

                its = [float(cone_op_prepared(prepare_dense(c), p, MODE_INNER, -1.0, 0.2, check=False, outputs=("loss",))
                             ["iters"].float().mean()) for p in preds]
            res[f"{tag}_us_per_step"] = round(best * 1e6, 1)
            res[f"{tag}_kernel_us_per_step"] = round(kern, 1)
            res[f"{tag}_kernels"] = top
            res[f"{tag}_newton_iters_mean"] = round(float(np.mean(its)), 3)
            if hits:
                res["warm_hit_rate"] = round(float(np.mean(hits)), 4)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
