#!/usr/bin/env python
"""The Held-Karp kernels (cave_hip_tsp_hk_solve, cave_amd/csrc/tsp_hk.h) timed against the host path they replace, in one
process on one device -> profiles/tsp_hk.json.

    python tools/diag/tsp_hk.py [--quick] [--out profiles/tsp_hk.json]

Kernel: n = 10, 12 (table in LDS) and 13, 14 (table in the default workspace, min(N, 512) slots), N = 1024 instances of
tsp_gen_data costs, the form tsp_regret(device=) launches (sol + obj + tour + eval + status, eval_costs given).
Timing: HIP events around groups of `--group` launches; the launches of a group rotate over `--batches` different input
batches (pairs of cost tensors), so no launch finds its own inputs in the caches from the launch before; the figure of a
repetition is the median group time per launch; `--reps` repetitions per n, the sizes alternating; reported: the median
of the repetitions and their spread (max - min).  Every size is warmed up, and its status examined, before it is timed.

Regret evaluation end to end at `--regret-n` (default 12), N = 1024: tsp_regret(device=) timed by the wall clock around
the call, which ends in the read-back of the scalar, with inputs on the device and on the host; and the host tsp_regret
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
    ap.add_argument("--regret-n", type=int, default=12)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_hk.json"))
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from cave_amd import _lib, tight

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    N = 64 if args.quick else 1024
    sizes = (8, 13) if args.quick else (10, 12, 13, 14)
    regret_n = 8 if args.quick else args.regret_n
    sample = 2 if args.quick else args.sample
    stream = _lib.current_stream()
    p = _lib.ptr

    state = {}
    for n in sizes:
        d = n * (n - 1) // 2
        batches = [(torch.tensor(tight.tsp_gen_data(N, 5, n, seed=100 + 2 * r)[1], device=dev),
                    torch.tensor(tight.tsp_gen_data(N, 5, n, seed=101 + 2 * r)[1], device=dev)) for r in range(args.batches)]
        ws_bytes = int(lib.cave_hip_tsp_hk_workspace_bytes(n, N))
        state[n] = {"batches": batches, "sol": torch.empty(N, d, device=dev), "obj": torch.empty(N, dtype=torch.float64, device=dev),
                    "ev": torch.empty(N, dtype=torch.float64, device=dev), "tour": torch.empty(N, n, dtype=torch.int32, device=dev),
                    "status": torch.empty(N, dtype=torch.int32, device=dev), "ws_bytes": ws_bytes,
                    "ws": torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev) if ws_bytes else None, "turn": 0}

    def launch(n):
        s = state[n]
        pred, true = s["batches"][s["turn"] % args.batches]
        s["turn"] += 1
        _lib.check(lib.cave_hip_tsp_hk_solve(p(pred), p(true), N, n, p(s["sol"]), p(s["obj"]), p(s["ev"]), p(s["tour"]), p(s["status"]),
                                             p(s["ws"]), s["ws_bytes"], stream), "cave_hip_tsp_hk_solve")

    for n in sizes:
        for _ in range(args.batches):
            launch(n)
            torch.cuda.synchronize()
            assert bool((state[n]["status"] == 0).all()), n

    def rep_us(n):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        launch(n)
        torch.cuda.synchronize()
        for a, b in evs:
            a.record()
            for _ in range(args.group):
                launch(n)
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / args.group for a, b in evs)
        return 1e3 * t[len(t) // 2]

    samples = {n: [] for n in sizes}
    for _ in range(args.reps):
        for n in sizes:
            samples[n].append(rep_us(n))
    kernel = {}
    for n in sizes:
        s = sorted(samples[n])
        med = s[len(s) // 2]
        slot = int(lib.cave_hip_tsp_hk_slot_bytes(n))
        kernel[f"n{n}"] = {"us": round(med, 2), "spread_us": round(s[-1] - s[0], 2), "repetitions_us": [round(x, 2) for x in samples[n]],
                           "us_per_instance": round(med / N, 4), "tier": "workspace" if slot else "lds",
                           "workgroups": min(N, state[n]["ws_bytes"] // slot) if slot else min(N, 2048),
                           "workspace_bytes": state[n]["ws_bytes"]}

    # ---- regret evaluation end to end: the device route (wall clock, ends in the scalar's read-back) and the host route
    n = regret_n
    true = tight.tsp_gen_data(N, 5, n, seed=100)[1]
    pred = tight.tsp_gen_data(N, 5, n, seed=101)[1]
    c_true, c_pred = torch.tensor(true, device=dev), torch.tensor(pred, device=dev)
    objs_t = tight.tsp_solve_hip(c_true, n)[1]
    z = np.asarray([tight.tsp_solve(c, n)[1] for c in true[:sample]], np.float64)
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

    tight.tsp_regret(c_pred, c_true, z32, n, device=dev)  # warm-up
    r_dev, t_dev, all_dev = wall(lambda: tight.tsp_regret(c_pred, c_true, z32, n, device=dev), 9)
    r_dev_h, t_dev_h, all_dev_h = wall(lambda: tight.tsp_regret(pred, true, z32_host, n, device=dev), 9)
    r_host_s, t_host_s, _ = wall(lambda: tight.tsp_regret(pred[:sample], true[:sample], z32_host[:sample], n), 1)
    r_dev_s = tight.tsp_regret(pred[:sample], true[:sample], z32_host[:sample], n, device=dev)
    bound = n * 2.0 ** -23 * (1.0 + abs(r_host_s))   # positive costs: sum c . w(c_hat) / sum z = 1 + regret
    assert abs(r_dev_s - r_host_s) <= bound and r_dev == r_dev_h, (r_dev_s, r_host_s, r_dev, r_dev_h)

    res = {"tool": "tools/diag/tsp_hk.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": f"TSP, N = {N}, tsp_gen_data costs; sol + obj + tour + eval + status per launch",
           "timing": f"kernel: HIP events around groups of {args.group} launches rotating over {args.batches} input batches, per "
                     f"repetition the median of {args.groups} groups, {args.reps} repetitions per size, sizes alternating, spread = "
                     "max - min; end to end: wall clock around calls that end in the scalar's read-back, median of 9 (device) / "
                     "one run on a sample (host)",
           "kernel": kernel,
           "regret_evaluation": {"n": n, "N": N, "device_tsp_regret_inputs_on_device_s": round(t_dev, 6),
                                 "device_tsp_regret_inputs_on_device_spread_s": round(max(all_dev) - min(all_dev), 6),
                                 "device_tsp_regret_inputs_on_host_s": round(t_dev_h, 6),
                                 "device_tsp_regret_inputs_on_host_spread_s": round(max(all_dev_h) - min(all_dev_h), 6),
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
