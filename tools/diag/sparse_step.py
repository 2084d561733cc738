#!/usr/bin/env python
"""The fused step on the sparse wire format, timed against the dense fused step and the sparse two-launch step.

    python tools/diag/sparse_step.py [--quick] [--out profiles/sparse_step.json]      -> one JSON line on stdout
    CAVE_LIB=cave_amd/libcave_hip_<NAME>.so python tools/diag/sparse_step.py             (an A/B build: build_variant.sh)

Workload: TSP-20, B = 1024, CaVE+ loss + gradient through the loss module (`check=False`), four rotating batches of
distinct cones out of 4096, predictions fixed per batch (cold forms) -- the rotating SPARSE inputs total about 36 MB, so
by size they are resident in the 256 MB Infinity Cache, as they are in training: these are not HBM-streaming figures
(the four dense batches are 4 x 183 MB and do stream).

Forms:
  a  dense fused chain        module(pred, prep) with prep.then(next dense batch): ONE launch per step
  b  sparse fused chain       the same with SparseCones batches (cave_hip_cone_step_sparse)
  c  sparse two-launch step   module(pred, cones): cave_hip_pack_fill_sparse + cave_hip_cone_packed (the route of a
                              SparseCones batch without this feature)
  d  dense fused chain, warm  a with solver_kwargs["warm_start"] (cache filled by the warm-up steps)
  e  sparse fused chain, warm b with it
  f  sparse pack-only launch  qpsolver.prepare_sparse alone

Timing: HIP events around groups of `--group` launches, the figure of a repetition is the median group time per step;
every form is repeated `--reps` times (>= 3), the forms alternating within one process; reported per form: the median
of its repetitions and their spread (max - min).  Side checks (asserted): every status is OK, b has the bits of a.
Conditions (evaluated, not assumed):  b faster than c by more than the spread;  b no slower than a, e no slower than d,
by more than the spread.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small batches (a functional run of the driver, not a measurement)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--groups", type=int, default=9, help="timed groups per repetition")
    ap.add_argument("--group", type=int, default=40, help="steps per group")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    assert args.reps >= 3

    from cave_amd import _lib, qpsolver, synth
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.sparse import SparseCones

    if os.environ.get("CAVE_LIB"):   # an A/B build of the library (tools/diag/build_variant.sh)
        _lib.LIB_PATH = os.path.abspath(os.environ["CAVE_LIB"])
    _lib.load()
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

    def module(warm):
        return innerConeAlignedCosine(M(), solver="hip", seed=0, reduction="none",
                                      solver_kwargs=dict({"warm_start": True} if warm else {}, check=False))

    class Chain:
        """a fused chain over the rotating batches: step i solves batch i % rotate and packs batch (i + 1) % rotate"""

        def __init__(self, batches, warm):
            self.batches, self.mod, self.i = batches, module(warm), 0

        def restart(self):
            # (the forms share the pool of lite stores: what another form ran in between has made this chain's store stale)
            self.prep = qpsolver.prepare_cones(self.batches[self.i % rotate])
            assert isinstance(self.prep, qpsolver.PreparedCones)

        def step(self):
            r = self.i % rotate
            self.prep.then(self.batches[(r + 1) % rotate])
            loss = self.mod(preds[r], self.prep)
            self.prep, self.i = self.prep.next, self.i + 1
            return loss

    class TwoLaunch:
        def __init__(self):
            self.mod, self.i = module(False), 0

        def restart(self):
            pass

        def step(self):
            r = self.i % rotate
            self.i += 1
            return self.mod(preds[r], sparse[r])

    class PackOnly:
        def __init__(self):
            self.i = 0

        def restart(self):
            pass

        def step(self):
            self.i += 1
            return qpsolver.prepare_sparse(sparse[self.i % rotate])

    # one checked call per wire format settles the shape; the side checks
    ref = {}
    for name, batches in (("a", dense), ("b", sparse)):
        outs = []
        prep = qpsolver.prepare_cones(batches[0])
        for r in range(rotate):
            prep.then(batches[(r + 1) % rotate])
            o = qpsolver.cone_op_prepared(prep, preds[r], qpsolver.MODE_INNER, -1.0, 0.2, outputs=("loss", "grad"))
            assert bool((o["status"] == 0).all())
            outs.append(o)
            prep = prep.next
        ref[name] = outs
    same_bits = all(torch.equal(x[k], y[k]) for x, y in zip(ref["a"], ref["b"]) for k in ("loss", "grad", "status", "iters"))
    assert same_bits, "the sparse fused chain does not reproduce the dense fused chain's bits"
    o = qpsolver.cone_op_sparse(sparse[0], preds[0], qpsolver.MODE_INNER, -1.0, 0.2, outputs=("loss", "grad"))
    assert bool((o["status"] == 0).all())

    forms = {"a_dense_fused": Chain(dense, False), "b_sparse_fused": Chain(sparse, False), "c_sparse_two_launch": TwoLaunch(),
             "d_dense_fused_warm": Chain(dense, True), "e_sparse_fused_warm": Chain(sparse, True), "f_sparse_pack_only": PackOnly()}

    def rep_us(form):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        form.restart()
        for _ in range(2 * rotate):   # warm-up: every batch through every slot of the pool (warm forms: the cache is full)
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
        for k, form in forms.items():   # alternating: one repetition of every form, then the next round
            us, h = rep_us(form)
            samples[k].append(us)
            host[k].append(h)
    # every status OK in the timed forms too (one more step each, examined)
    for k in ("a_dense_fused", "b_sparse_fused", "d_dense_fused_warm", "e_sparse_fused_warm"):
        f = forms[k]
        f.restart()
        f.step()
        if f.mod._warm is not None:
            assert bool((f.mod._warm.last_status == 0).all()), k
    hits = {k: float(forms[k].mod._warm.last_hit.float().mean()) for k in ("d_dense_fused_warm", "e_sparse_fused_warm")}
    iters = {k: float(forms[k].mod._warm.last_iters.float().mean()) for k in ("d_dense_fused_warm", "e_sparse_fused_warm")}

    res = {"tool": "tools/diag/sparse_step.py", "library": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": f"TSP-20 B={B}, {rotate} rotating batches of distinct cones, CaVE+ loss + gradient, check=False",
           "timing": f"HIP events around groups of {args.group} launches; per repetition the median of {args.groups} groups; "
                     f"{args.reps} repetitions per form, forms alternating in one process; spread = max - min of the repetitions",
           "memory_level": f"the {rotate} rotating SPARSE batches total {sum(s.nbytes for s in sparse) / 1e6:.1f} MB: resident in the "
                           "256 MB Infinity Cache by size (as in training), not an HBM-streaming figure; the dense batches are "
                           f"{rotate} x {4 * B * m * d / 1e6:.0f} MB and stream from HBM",
           "b_same_bits_as_a": bool(same_bits), "all_status_ok": True, "warm_hit_rate": hits, "warm_newton_iters_mean": iters,
           "us_per_step": {}}
    for k, v in samples.items():
        s = sorted(v)
        res["us_per_step"][k] = {"median": round(s[len(s) // 2], 2), "spread": round(s[-1] - s[0], 2),
                                 "repetitions": [round(x, 2) for x in v],
                                 "host_enqueue_us_per_step": round(float(np.median(host[k])), 1)}
    u = res["us_per_step"]

    def faster(x, y):     # x faster than y by more than the recorded spread
        return bool(u[x]["median"] + max(u[x]["spread"], u[y]["spread"]) < u[y]["median"])

    def no_slower(x, y):  # x no slower than y by more than the spread
        return bool(u[x]["median"] <= u[y]["median"] + max(u[x]["spread"], u[y]["spread"]))

    res["conditions"] = {"b_faster_than_c": faster("b_sparse_fused", "c_sparse_two_launch"),
                         "b_no_slower_than_a": no_slower("b_sparse_fused", "a_dense_fused"),
                         "e_no_slower_than_d": no_slower("e_sparse_fused_warm", "d_dense_fused_warm")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
