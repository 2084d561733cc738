#!/usr/bin/env python
"""The wide Held-Karp tier (cave_hip_tsp_hk_wide_solve, cave_amd/csrc/tsp_hk_wide.h) timed against the first tier where
both apply, against the HBM rate, and against the host path it replaces, in one process on one device ->
profiles/tsp_hk_wide.json.

    python tools/diag/tsp_hk_wide.py [--quick] [--out profiles/tsp_hk_wide.json]

Kernel: tsp_gen_data costs, the form tsp_regret(device=) launches (sol + obj + tour + eval + status, eval_costs given),
default workspaces.  n = 13, 14, N = 1024: cave_hip_tsp_hk_solve and cave_hip_tsp_hk_wide_solve on the same inputs, in
the same run, alternating; their outputs are compared byte for byte first.  n = 15 ... 20: the wide entry alone, N = 1024
up to n = 18 and N = 256 at n = 19, 20.  A launch of the wide entry is its two kernels: the list kernel and the sweep.
Timing (the method of tools/diag/tsp_hk.py): HIP events around groups of launches (8 up to n = 16, 2 beyond); the
launches of a group rotate over `--batches` different input batches; the figure of a repetition is the median group time
per launch; `--reps` repetitions per (entry, n), all of them alternating; reported: the median of the repetitions and
their spread (max - min).  Every case is warmed up, and its status examined, before it is timed.
Table traffic: every table entry is stored once and loaded once per instance, 2 * slot_bytes * N bytes per launch, over
the launch time, beside the 6.3 TB/s a streaming kernel reaches on this device (a rate of the whole launch: the list
kernel, the staging and the walk back are in the time, their bytes are not in the count).

Regret evaluation end to end at n = 20, N = 256: tsp_regret(device=) by the wall clock around the call, which ends in
the read-back of the scalar; and the host alternative of the same run, the only exact host solver at that size: a
tight.tsp_dfj_cuts loop (HiGHS) over a `--sample` of the predictions, EXTRAPOLATED to N (labelled so).

No speed threshold: the file records what was measured.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_TBS = 6.3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 8, n = 13 / 15 and a 2-instance host sample (a functional run of the driver)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsp_hk_wide.json"))
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from cave_amd import _lib, tight

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.quick:
        cases = [("tsp_hk", 13, 8), ("tsp_hk_wide", 13, 8), ("tsp_hk_wide", 15, 8)]
        regret_n, regret_N, sample = 15, 8, 2
    else:
        cases = [(e, n, 1024) for n in (13, 14) for e in ("tsp_hk", "tsp_hk_wide")] + \
                [("tsp_hk_wide", n, 1024 if n <= 18 else 256) for n in range(15, 21)]
        regret_n, regret_N, sample = 20, 256, args.sample
    stream = _lib.current_stream()
    p = _lib.ptr

    inputs, state = {}, {}
    for entry, n, N in cases:
        d = n * (n - 1) // 2
        if (n, N) not in inputs:
            inputs[(n, N)] = [(torch.tensor(tight.tsp_gen_data(N, 5, n, seed=100 + 2 * r)[1], device=dev),
                               torch.tensor(tight.tsp_gen_data(N, 5, n, seed=101 + 2 * r)[1], device=dev)) for r in range(args.batches)]
        ws_bytes = int(getattr(lib, f"cave_hip_{entry}_workspace_bytes")(n, N))
        state[(entry, n)] = {"N": N, "batches": inputs[(n, N)], "sol": torch.empty(N, d, device=dev),
                             "obj": torch.empty(N, dtype=torch.float64, device=dev), "ev": torch.empty(N, dtype=torch.float64, device=dev),
                             "tour": torch.empty(N, n, dtype=torch.int32, device=dev), "status": torch.empty(N, dtype=torch.int32, device=dev),
                             "ws_bytes": ws_bytes, "ws": torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev), "turn": 0,
                             "solve": getattr(lib, f"cave_hip_{entry}_solve"), "group": 8 if n <= 16 else 2}

    def launch(key):
        s = state[key]
        pred, true = s["batches"][s["turn"] % args.batches]
        s["turn"] += 1
        _lib.check(s["solve"](p(pred), p(true), s["N"], key[1], p(s["sol"]), p(s["obj"]), p(s["ev"]), p(s["tour"]), p(s["status"]),
                              p(s["ws"]), s["ws_bytes"], stream), f"cave_hip_{key[0]}_solve")

    for key in state:  # warm-up over every input batch; the two entries agree byte for byte where both run
        for _ in range(args.batches):
            launch(key)
            torch.cuda.synchronize()
            assert bool((state[key]["status"] == 0).all()), key
        other = ("tsp_hk", key[1])
        if key[0] == "tsp_hk_wide" and other in state:
            for k in ("sol", "obj", "ev", "tour"):   # (both have just run the last batch of the rotation)
                assert torch.equal(state[key][k].view(torch.uint8), state[other][k].view(torch.uint8)), (key, k)

    def rep_us(key):
        group = state[key]["group"]
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        launch(key)
        torch.cuda.synchronize()
        for a, b in evs:
            a.record()
            for _ in range(group):
                launch(key)
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / group for a, b in evs)
        return 1e3 * t[len(t) // 2]

    samples = {key: [] for key in state}
    for _ in range(args.reps):
        for key in state:
            samples[key].append(rep_us(key))
    kernel = {}
    for (entry, n), s in state.items():
        r = sorted(samples[(entry, n)])
        med, N = r[len(r) // 2], s["N"]
        slot = int(getattr(lib, f"cave_hip_{entry}_slot_bytes")(n))
        header = s["ws_bytes"] - slot * min(N, s["ws_bytes"] // slot)
        rec = {"N": N, "us": round(med, 2), "spread_us": round(r[-1] - r[0], 2), "repetitions_us": [round(x, 2) for x in samples[(entry, n)]],
               "us_per_instance": round(med / N, 4), "workgroups": min(N, (s["ws_bytes"] - header) // slot),
               "workspace_bytes": s["ws_bytes"], "launches_per_group": s["group"]}
        if entry == "tsp_hk_wide":
            tbs = 2.0 * slot * N / (med * 1e-6) / 1e12
            rec.update({"table_bytes_stored_and_loaded": 2 * slot * N, "table_tb_per_s": round(tbs, 4),
                        "share_of_achievable_hbm_rate": round(tbs / HBM_ACHIEVABLE_TBS, 4)})
        kernel[f"{entry}_n{n}"] = rec
    both = {f"n{n}": round(kernel[f"tsp_hk_wide_n{n}"]["us"] / kernel[f"tsp_hk_n{n}"]["us"], 4)
            for n in (13, 14) if f"tsp_hk_n{n}" in kernel}

    # ---- regret evaluation end to end: the device route (wall clock, ends in the scalar's read-back) and the host route
    n, N = regret_n, regret_N
    true = tight.tsp_gen_data(N, 5, n, seed=100)[1]
    pred = tight.tsp_gen_data(N, 5, n, seed=101)[1]
    c_true, c_pred = torch.tensor(true, device=dev), torch.tensor(pred, device=dev)
    z32 = tight.tsp_solve_hip_wide(c_true, n)[1].to(torch.float32)
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

    def host_sample():  # tsp_regret's arithmetic with the cut loop's tours
        loss = 0.0
        for cp, c, z in zip(pred[:sample], true[:sample], z32_host[:sample]):
            loss += float(c @ tight.tsp_dfj_cuts(cp, n)[0]) - float(z)
        return loss / float(np.abs(z32_host[:sample]).sum() + 1e-7)

    r_host_s, t_host_s, _ = wall(host_sample, 1)
    r_dev_s = tight.tsp_regret(pred[:sample], true[:sample], z32_host[:sample], n, device=dev)
    bound = n * 2.0 ** -23 * (1.0 + abs(r_host_s))   # positive costs: sum c . w(c_hat) / sum z = 1 + regret
    assert abs(r_dev_s - r_host_s) <= bound and r_dev == r_dev_h, (r_dev_s, r_host_s, r_dev, r_dev_h)

    res = {"tool": "tools/diag/tsp_hk_wide.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": "TSP, tsp_gen_data costs; sol + obj + tour + eval + status per launch; default workspaces; a launch of the "
                     "wide entry is the list kernel and the sweep kernel",
           "timing": f"kernel: HIP events around groups of launches (8 up to n = 16, 2 beyond) rotating over {args.batches} input "
                     f"batches, per repetition the median of {args.groups} groups, {args.reps} repetitions per case, all cases "
                     "alternating, spread = max - min; end to end: wall clock around calls that end in the scalar's read-back, "
                     "median of 9 (device) / one run on a sample (host)",
           "achievable_hbm_tb_per_s": HBM_ACHIEVABLE_TBS,
           "kernel": kernel, "wide_over_first_tier_time": both,
           "regret_evaluation": {"n": n, "N": N, "device_tsp_regret_inputs_on_device_s": round(t_dev, 6),
                                 "device_tsp_regret_inputs_on_device_spread_s": round(max(all_dev) - min(all_dev), 6),
                                 "device_tsp_regret_inputs_on_host_s": round(t_dev_h, 6),
                                 "device_tsp_regret_inputs_on_host_spread_s": round(max(all_dev_h) - min(all_dev_h), 6),
                                 "host_route": "tight.tsp_dfj_cuts per prediction (HiGHS cut loop)",
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
