#!/usr/bin/env python
"""The wide CVRP tier (cave_hip_vrp_dp_wide_solve, cave_amd/csrc/vrp_dp_wide.h) timed beside the first tier where both
run, beside the wide Held-Karp launch whose sweep is its phase 1, and against the only host alternative above 14 nodes,
in one process on one device -> profiles/vrp_dp_wide.json.

    python tools/diag/vrp_dp_wide.py [--quick] [--out profiles/vrp_dp_wide.json]

Kernel cases (n, K): 13 and 14 at K = 3 with the first tier (cave_hip_vrp_dp_solve) in the same run; 15 .. 20 at K = 2
(no stored layer) and K = 3 (one); n = 20 at `--big-k` (default 5: three stored layers).  With `--variant-lib` the wide
entry of an A/B build that deals every set of a layer to one thread (no class goes to the whole workgroup) is timed
beside n = 18, 19, 20 at K = 3.  N instances of vrp_gen_data
costs with one demand vector per size and the capacity ceil(1.3 total / K' + 5), the form vrp_regret(device=) launches
(sol + obj + routes + eval + status, eval_costs given), default workspaces.  N = 1024 up to n = 15, 512 at 16 and 17, 128
from 18 on: there every instance has a workgroup and a compute unit of its own, so the launch time IS the time of one
instance.  The wide Held-Karp entry (cave_hip_tsp_hk_wide_solve) runs on the same cost tensors with the same N beside
every size: its sweep is the dynamic program's phase 1, so its time is the floor.
Timing (the method of tools/diag/vrp_dp.py): HIP events around groups of launches (4 up to n = 15, 2 at 16 and 17, 1
beyond) that rotate over `--batches` different input batches; the figure of a repetition is the median group time per
launch; `--reps` repetitions of every case, all cases alternating; reported: the median of the repetitions and their
spread (max - min).  Every case is warmed up, and its status examined, before it is timed.

Regret evaluation end to end at `--regret-n` (default 16), K = 3, N = 256: vrp_regret(device=) by the wall clock around
the call, which ends in the read-back of the scalar.  The host has no exact solver there but the HiGHS cut loop: the
time of tight.vrp_rcc_cuts on a `--sample` of the instances, EXTRAPOLATED to N (labelled so), its objectives checked
against the device's.

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
    ap.add_argument("--quick", action="store_true", help="n = 13, 15 and 18 only, small N, 2 repetitions (a functional run of the driver)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--big-k", type=int, default=5)
    ap.add_argument("--regret-n", type=int, default=16)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--variant-lib", default=None,
                    help="an A/B build of the library (tools/diag/build_variant.sh nogroup -DCAVE_VRP_DP_WIDE_GROUP_PAIRS=0x80000000u "
                         "k_vrp_dp_wide: every set of a layer to one thread, popcount order throughout): its wide entry is timed at "
                         "n = 18, 19, 20, K = 3 in the same run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vrp_dp_wide.json"))
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from cave_amd import _lib, tight

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = _lib.current_stream()
    p = _lib.ptr
    reps = 2 if args.quick else args.reps
    vlib = None
    if args.variant_lib:
        import ctypes as C

        vlib = C.CDLL(args.variant_lib)
        vlib.cave_hip_vrp_dp_wide_solve.argtypes = lib.cave_hip_vrp_dp_wide_solve.argtypes
        vlib.cave_hip_vrp_dp_wide_solve.restype = C.c_int32
    if args.quick:
        cases = [(13, 3), (15, 2), (15, 3), (18, 3)]
    else:
        cases = [(13, 3), (14, 3)] + [(n, K) for n in range(15, 21) for K in (2, 3)] + [(20, args.big_k)]
    sizes = sorted({n for n, _ in cases})

    def n_of(n):
        full = 1024 if n <= 15 else 512 if n <= 17 else 128
        return min(full, 32) if args.quick else full

    def group_of(n):
        return 4 if n <= 15 else 2 if n <= 17 else 1

    def kmax(n, K):
        return min(K, (n - 1) // 2)

    data = {}
    for n in sizes:
        N, d = n_of(n), n * (n - 1) // 2
        q = tight.vrp_gen_data(N, 5, n, seed=100)[2]
        batches = [(torch.tensor(tight.vrp_gen_data(N, 5, n, seed=100 + 2 * r)[1], device=dev),
                    torch.tensor(tight.vrp_gen_data(N, 5, n, seed=101 + 2 * r)[1], device=dev)) for r in range(args.batches)]
        data[n] = {"N": N, "q": q, "qd": torch.tensor(q, device=dev), "batches": batches, "turn": 0,
                   "sol": torch.empty(N, d, device=dev), "obj": torch.empty(N, dtype=torch.float64, device=dev),
                   "ev": torch.empty(N, dtype=torch.float64, device=dev), "routes": torch.empty(N, n + 8, dtype=torch.int32, device=dev),
                   "status": torch.empty(N, dtype=torch.int32, device=dev)}
    ws_need = [int(lib.cave_hip_vrp_dp_wide_workspace_bytes(n, K, n_of(n))) for n, K in cases]
    ws_need += [int(lib.cave_hip_tsp_hk_wide_workspace_bytes(n, n_of(n))) for n in sizes]
    ws_need += [int(lib.cave_hip_vrp_dp_workspace_bytes(n, K, n_of(n))) for n, K in cases if n <= 14]
    ws = torch.empty(max(ws_need) // 8, dtype=torch.float64, device=dev)   # one buffer, every launch takes its own size of it

    def capacity(n, K):
        return float(np.ceil(1.3 * float(data[n]["q"].sum()) / kmax(n, K) + 5.0))

    def launch(which, n, K):
        s = data[n]
        N = s["N"]
        pred, true = s["batches"][s["turn"] % args.batches]
        s["turn"] += 1
        if which == "hk_wide":
            wsb = int(lib.cave_hip_tsp_hk_wide_workspace_bytes(n, N))
            _lib.check(lib.cave_hip_tsp_hk_wide_solve(p(pred), p(true), N, n, p(s["sol"]), p(s["obj"]), p(s["ev"]), p(s["routes"]), p(s["status"]),
                                                      p(ws), wsb, stream), "cave_hip_tsp_hk_wide_solve")
            return
        entry = "vrp_dp" if which == "first" else "vrp_dp_wide"
        wsb = int(getattr(lib, f"cave_hip_{entry}_workspace_bytes")(n, K, N))
        _lib.check(getattr(vlib if which == "variant" else lib, f"cave_hip_{entry}_solve")(p(pred), p(true), p(s["qd"]), capacity(n, K), K, N, n, p(s["sol"]), p(s["obj"]),
                                                           p(s["ev"]), p(s["routes"]), p(s["status"]), p(ws), wsb, stream),
                   f"cave_hip_{entry}_solve")

    runs = [("wide", n, K) for n, K in cases] + [("first", n, K) for n, K in cases if n <= 14] + [("hk_wide", n, 0) for n in sizes]
    if vlib is not None:
        runs += [("variant", n, K) for n, K in cases if n >= 18 and K == 3]
    for r in runs:
        for _ in range(2):
            launch(*r)
            torch.cuda.synchronize()
            assert bool((data[r[1]]["status"] == 0).all()), r

    def rep_us(which, n, K):
        g = group_of(n)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        for a, b in evs:
            a.record()
            for _ in range(g):
                launch(which, n, K)
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / g for a, b in evs)
        return 1e3 * t[len(t) // 2]

    samples = {r: [] for r in runs}
    for _ in range(reps):
        for r in runs:
            samples[r].append(rep_us(*r))

    def summary(xs):
        s = sorted(xs)
        return s[len(s) // 2], s[-1] - s[0]

    kernel = {}
    for n, K in cases:
        N = n_of(n)
        med, spread = summary(samples[("wide", n, K)])
        hk, hk_spread = summary(samples[("hk_wide", n, 0)])
        slot = int(lib.cave_hip_vrp_dp_wide_slot_bytes(n, K))
        wsb = int(lib.cave_hip_vrp_dp_wide_workspace_bytes(n, K, N))
        e = {"N": N, "us": round(med, 2), "spread_us": round(spread, 2), "repetitions_us": [round(x, 2) for x in samples[("wide", n, K)]],
             "us_per_instance": round(med / N, 3), "stored_layers": max(kmax(n, K) - 2, 0),
             "pairs_per_stored_layer": 3 ** (n - 1) // 2, "held_karp_wide_us": round(hk, 2), "held_karp_wide_spread_us": round(hk_spread, 2),
             "ratio_to_held_karp_wide": round(med / hk, 3), "slot_bytes": slot, "workgroups": min(N, (wsb - 4 * 2 ** (n - 1)) // slot),
             "workspace_bytes": wsb, "capacity": capacity(n, K), "launches_per_group": group_of(n)}
        if n <= 14:
            f, f_spread = summary(samples[("first", n, K)])
            e.update({"first_tier_us": round(f, 2), "first_tier_spread_us": round(f_spread, 2), "ratio_to_first_tier": round(med / f, 3)})
        if ("variant", n, K) in samples:
            v, v_spread = summary(samples[("variant", n, K)])
            e.update({"one_set_per_thread_throughout_us": round(v, 2), "one_set_per_thread_throughout_spread_us": round(v_spread, 2)})
        kernel[f"n{n}_K{K}"] = e

    # ---- regret evaluation end to end (wall clock, ends in the scalar's read-back), and the host's cut loop on a sample
    n, K = (15 if args.quick else args.regret_n), 3
    N = 16 if args.quick else 256
    sample = 2 if args.quick else args.sample
    _, true, q = tight.vrp_gen_data(N, 5, n, seed=100)
    pred = tight.vrp_gen_data(N, 5, n, seed=101)[1]
    cap = float(np.ceil(1.3 * float(q.sum()) / kmax(n, K) + 5.0))
    c_true, c_pred = torch.tensor(true, device=dev), torch.tensor(pred, device=dev)
    objs_t = tight.vrp_solve_hip_wide(c_true, n, q, cap, K)[1]
    z32 = objs_t.to(torch.float32)

    def wall(fn, k):
        out = []
        for _ in range(k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            out.append(time.perf_counter() - t0)
        return r, sorted(out)[len(out) // 2], out

    tight.vrp_regret(c_pred, c_true, z32, n, q, cap, K, device=dev)  # warm-up
    r_dev, t_dev, all_dev = wall(lambda: tight.vrp_regret(c_pred, c_true, z32, n, q, cap, K, device=dev), 5)
    t0 = time.perf_counter()
    z_host = [tight.vrp_rcc_cuts(c, n, q, cap, K)[1] for c in true[:sample]]
    t_host = time.perf_counter() - t0
    z_dev = objs_t[:sample].cpu().numpy()
    assert all(abs(a - b) <= (n + K) * 2.0 ** -52 * abs(b) for a, b in zip(z_host, z_dev)), (z_host, z_dev)   # the same optima

    res = {"tool": "tools/diag/vrp_dp_wide.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": "CVRP, vrp_gen_data costs and demands, capacity ceil(1.3 total / K' + 5); sol + obj + routes + eval + status per "
                     "launch; default workspaces; a launch of a wide entry is the list kernel and its main kernel; the wide Held-Karp "
                     "entry and, up to n = 14, the first CVRP tier on the same cost tensors with the same N",
           "timing": f"kernel: HIP events around groups of launches (4 up to n = 15, 2 at 16 and 17, 1 beyond) rotating over {args.batches} "
                     f"input batches, per repetition the median of {args.groups} groups, {reps} repetitions per case, all cases alternating, "
                     "spread = max - min; end to end: wall clock around calls that end in the scalar's read-back, median of 5",
           "kernel": kernel,
           "regret_evaluation": {"n": n, "K": K, "N": N, "capacity": cap, "device_vrp_regret_inputs_on_device_s": round(t_dev, 6),
                                 "device_vrp_regret_inputs_on_device_spread_s": round(max(all_dev) - min(all_dev), 6),
                                 "regret_device_full_set": r_dev,
                                 "host_alternative": "tight.vrp_rcc_cuts (HiGHS cut loop): the objectives alone, one instance after the other",
                                 "host_sample_instances": sample, "host_sample_s": round(t_host, 3),
                                 "host_extrapolated_to_N_s": round(t_host * N / sample, 1)}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
