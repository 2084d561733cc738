#!/usr/bin/env python
"""The CVRP dynamic-program kernels (cave_hip_vrp_dp_solve, cave_amd/csrc/vrp_dp.h) timed beside the Held-Karp kernels
they build on and against the host path they replace, in one process on one device -> profiles/vrp_dp.json.

    python tools/diag/vrp_dp.py [--quick] [--out profiles/vrp_dp.json]

Kernel: n = 10, 12 (all tables in LDS) and 13, 14 (the Held-Karp table in the default workspace, min(N, 512) slots), K = 3,
N = 1024 instances of vrp_gen_data costs with one demand vector per size and the capacity ceil(1.3 total / K + 5), the form
vrp_regret(device=) launches (sol + obj + routes + eval + status, eval_costs given).  The Held-Karp kernel
(cave_hip_tsp_hk_solve) runs on the same cost tensors in the same run: the table sweep is the dynamic program's second
phase, so its time is the floor and the ratio is what the route costs, the partition layers and the walk back add.
Timing: HIP events around groups of `--group` launches; the launches of a group rotate over `--batches` different input
batches (pairs of cost tensors), so no launch finds its own inputs in the caches from the launch before; the figure of a
repetition is the median group time per launch; `--reps` repetitions per kernel and n, alternating; reported: the median
of the repetitions and their spread (max - min).  Every size is warmed up, and its status examined, before it is timed.

Regret evaluation end to end at `--regret-n` (default 10), N = 1024: vrp_regret(device=) timed by the wall clock around
the call, which ends in the read-back of the scalar, with inputs on the device and on the host; and the host vrp_regret
of the same run on a `--sample` of the instances, EXTRAPOLATED to N (labelled so).  The true objectives are the
device's, which are checked against the host's on the sample.

No speed threshold: the file records what was measured.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 64, n = 8 / 13 and a 2-instance host sample (a functional run of the driver)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--vehicles", type=int, default=3)
    ap.add_argument("--regret-n", type=int, default=10)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vrp_dp.json"))
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from cave_amd import _lib, tight

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    N = 64 if args.quick else 1024
    K = args.vehicles
    sizes = (8, 13) if args.quick else (10, 12, 13, 14)
    regret_n = 8 if args.quick else args.regret_n
    sample = 2 if args.quick else args.sample
    stream = _lib.current_stream()
    p = _lib.ptr

    def instance(n, seed):
        _, c, q = tight.vrp_gen_data(N, 5, n, seed=seed)
        return c, q

    def capacity_of(q):
        return float(np.ceil(1.3 * float(q.sum()) / K + 5.0))

    state = {}
    for n in sizes:
        d = n * (n - 1) // 2
        q = instance(n, 100)[1]
        batches = [(torch.tensor(instance(n, 100 + 2 * r)[0], device=dev), torch.tensor(instance(n, 101 + 2 * r)[0], device=dev))
                   for r in range(args.batches)]
        ws_bytes = int(lib.cave_hip_vrp_dp_workspace_bytes(n, K, N))
        hk_bytes = int(lib.cave_hip_tsp_hk_workspace_bytes(n, N))
        state[n] = {"batches": batches, "q": torch.tensor(q, device=dev), "cap": capacity_of(q),
                    "sol": torch.empty(N, d, device=dev), "obj": torch.empty(N, dtype=torch.float64, device=dev),
                    "ev": torch.empty(N, dtype=torch.float64, device=dev), "routes": torch.empty(N, n + K, dtype=torch.int32, device=dev),
                    "tour": torch.empty(N, n, dtype=torch.int32, device=dev), "status": torch.empty(N, dtype=torch.int32, device=dev),
                    "ws_bytes": ws_bytes, "hk_bytes": hk_bytes,
                    "ws": torch.empty(max(ws_bytes, hk_bytes) // 8, dtype=torch.float64, device=dev) if max(ws_bytes, hk_bytes) else None,
                    "turn": 0}

    def launch(n, which):
        s = state[n]
        pred, true = s["batches"][s["turn"] % args.batches]
        s["turn"] += 1
        if which == "vrp":
            _lib.check(lib.cave_hip_vrp_dp_solve(p(pred), p(true), p(s["q"]), s["cap"], K, N, n, p(s["sol"]), p(s["obj"]), p(s["ev"]),
                                                 p(s["routes"]), p(s["status"]), p(s["ws"]) if s["ws_bytes"] else None, s["ws_bytes"],
                                                 stream), "cave_hip_vrp_dp_solve")
        else:
            _lib.check(lib.cave_hip_tsp_hk_solve(p(pred), p(true), N, n, p(s["sol"]), p(s["obj"]), p(s["ev"]), p(s["tour"]), p(s["status"]),
                                                 p(s["ws"]) if s["hk_bytes"] else None, s["hk_bytes"], stream), "cave_hip_tsp_hk_solve")

    for n in sizes:
        for which in ("vrp", "hk"):
            for _ in range(args.batches):
                launch(n, which)
                torch.cuda.synchronize()
                assert bool((state[n]["status"] == 0).all()), (n, which)

    def rep_us(n, which):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        launch(n, which)
        torch.cuda.synchronize()
        for a, b in evs:
            a.record()
            for _ in range(args.group):
                launch(n, which)
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / args.group for a, b in evs)
        return 1e3 * t[len(t) // 2]

    samples = {(n, w): [] for n in sizes for w in ("vrp", "hk")}
    for _ in range(args.reps):
        for n in sizes:
            for which in ("vrp", "hk"):
                samples[(n, which)].append(rep_us(n, which))

    def summary(xs):
        s = sorted(xs)
        return s[len(s) // 2], s[-1] - s[0]

    kernel = {}
    for n in sizes:
        med, spread = summary(samples[(n, "vrp")])
        hk, hk_spread = summary(samples[(n, "hk")])
        slot = int(lib.cave_hip_vrp_dp_slot_bytes(n, K))
        kernel[f"n{n}"] = {"us": round(med, 2), "spread_us": round(spread, 2), "repetitions_us": [round(x, 2) for x in samples[(n, "vrp")]],
                           "us_per_instance": round(med / N, 4), "held_karp_us": round(hk, 2), "held_karp_spread_us": round(hk_spread, 2),
                           "ratio_to_held_karp": round(med / hk, 3), "slot_bytes": slot,
                           "workgroups": min(N, state[n]["ws_bytes"] // slot) if slot else min(N, 2048),
                           "workspace_bytes": state[n]["ws_bytes"], "capacity": state[n]["cap"]}

    # ---- regret evaluation end to end: the device route (wall clock, ends in the scalar's read-back) and the host route
    n = regret_n
    true, q = instance(n, 100)
    pred = instance(n, 101)[0]
    cap = capacity_of(q)
    c_true, c_pred = torch.tensor(true, device=dev), torch.tensor(pred, device=dev)
    objs_t = tight.vrp_solve_hip(c_true, n, q, cap, K)[1]
    z = np.asarray([tight.vrp_solve(c, n, q, cap, K)[1] for c in true[:sample]], np.float64)
    assert np.array_equal(objs_t[:sample].cpu().numpy(), z)   # the device's are the host's
    z32 = objs_t.to(torch.float32)
    z32_host = z32.cpu().numpy()

    def wall(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            out.append(time.perf_counter() - t0)
        return r, sorted(out)[len(out) // 2], out

    tight.vrp_regret(c_pred, c_true, z32, n, q, cap, K, device=dev)  # warm-up
    r_dev, t_dev, all_dev = wall(lambda: tight.vrp_regret(c_pred, c_true, z32, n, q, cap, K, device=dev), 9)
    r_dev_h, t_dev_h, all_dev_h = wall(lambda: tight.vrp_regret(pred, true, z32_host, n, q, cap, K, device=dev), 9)
    r_host_s, t_host_s, _ = wall(lambda: tight.vrp_regret(pred[:sample], true[:sample], z32_host[:sample], n, q, cap, K), 1)
    r_dev_s = tight.vrp_regret(pred[:sample], true[:sample], z32_host[:sample], n, q, cap, K, device=dev)
    bound = (n + K) * 2.0 ** -23 * (1.0 + abs(r_host_s))   # positive costs: sum c . w(c_hat) / sum z = 1 + regret
    assert abs(r_dev_s - r_host_s) <= bound and r_dev == r_dev_h, (r_dev_s, r_host_s, r_dev, r_dev_h)

    res = {"tool": "tools/diag/vrp_dp.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": f"CVRP, K = {K}, N = {N}, vrp_gen_data costs and demands, capacity ceil(1.3 total / K + 5); sol + obj + routes + "
                     "eval + status per launch; the Held-Karp kernel on the same cost tensors (sol + obj + tour + eval + status)",
           "timing": f"kernel: HIP events around groups of {args.group} launches rotating over {args.batches} input batches, per "
                     f"repetition the median of {args.groups} groups, {args.reps} repetitions per kernel and size, alternating, spread "
                     "= max - min; end to end: wall clock around calls that end in the scalar's read-back, median of 9 (device) / "
                     "one run on a sample (host)",
           "kernel": kernel,
           "regret_evaluation": {"n": n, "K": K, "N": N, "capacity": cap, "device_vrp_regret_inputs_on_device_s": round(t_dev, 6),
                                 "device_vrp_regret_inputs_on_device_spread_s": round(max(all_dev) - min(all_dev), 6),
                                 "device_vrp_regret_inputs_on_host_s": round(t_dev_h, 6),
                                 "device_vrp_regret_inputs_on_host_spread_s": round(max(all_dev_h) - min(all_dev_h), 6),
                                 "host_sample_instances": sample, "host_sample_s": round(t_host_s, 3),
                                 "host_extrapolated_to_N_s": round(t_host_s * N / sample, 1),
                                 "regret_device_full_set": r_dev, "regret_host_sample": r_host_s, "regret_device_sample": r_dev_s,
                                 "sample_difference": abs(r_dev_s - r_host_s), "sample_bound": bound}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
