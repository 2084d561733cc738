#!/usr/bin/env python
"""The grid shortest-path kernel (cave_hip_sp_grid_solve, cave_amd/csrc/sp_grid.h) timed against the host path it
replaces, in one process on one device -> profiles/sp_grid.json.

    python tools/diag/sp_grid.py [--quick] [--out profiles/sp_grid.json]

Setting: 30x30 grid (d = 1740), N = 10 000 instances, sp_gen_data costs; the "predictions" are a second sp_gen_data draw.

Device forms (one launch each, through the Python layer's tensors and the C ABI):
  solve        sol + obj + status
  solve_eval   sol + obj + eval + status, eval_costs given             (what sp_regret(device=) launches)
  solve_cones  sol + obj + status + key + val                          (what SPConeDataset(device=) launches)
Timing: HIP events around groups of `--group` launches; the figure of a repetition is the median group time per launch;
`--reps` repetitions per form, the forms alternating; reported: the median of the repetitions and their spread (max -
min).  Every form is warmed up, and its status examined, before it is timed.

Bytes the kernel must move (computed from the shapes): 4 N d per cost tensor read, 4 N d for sol, 8 * 5 d N for key +
val; over the kernel time that is the achieved rate, reported beside its share of the 8 TB/s HBM peak.

Host path, same run, same machine: tight.sp_regret on the same predictions (all N, wall clock), and the solve loop of
SPConeDataset on a 200-instance sample, EXTRAPOLATED to N (labelled so).  sp_regret(device=) on the full set is timed
end to end (wall clock around the call, which ends in the read-back of the scalar), inputs on the host and on the device.

The one condition: device regret evaluation of the full set is faster than the host evaluation of this run.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12  # bytes / s


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="N = 256 and a 16-instance host sample (a functional run of the driver)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--group", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sp_grid.json"))
    args = ap.parse_args(argv)

    import numpy as np
    import torch

    from cave_amd import _lib, tight

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = w = 30
    N, sample = (256, 16) if args.quick else (10000, 200)
    d = h * (w - 1) + (h - 1) * w
    feats, true = tight.sp_gen_data(N, 5, h, w, seed=135)
    pred = tight.sp_gen_data(N, 5, h, w, seed=77)[1]
    c_true, c_pred = torch.tensor(true, device=dev), torch.tensor(pred, device=dev)

    sol = torch.empty(N, d, device=dev)
    obj = torch.empty(N, dtype=torch.float64, device=dev)
    ev = torch.empty(N, dtype=torch.float64, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    key = torch.empty(N * 5 * d, dtype=torch.int32, device=dev)
    val = torch.empty(N * 5 * d, device=dev)
    stream = _lib.current_stream()
    p = _lib.ptr

    def launch(form):
        if form == "solve":
            rc = lib.cave_hip_sp_grid_solve(p(c_pred), None, N, h, w, p(sol), p(obj), None, p(status), None, None, stream)
        elif form == "solve_eval":
            rc = lib.cave_hip_sp_grid_solve(p(c_pred), p(c_true), N, h, w, p(sol), p(obj), p(ev), p(status), None, None, stream)
        else:
            rc = lib.cave_hip_sp_grid_solve(p(c_true), None, N, h, w, p(sol), p(obj), None, p(status), p(key), p(val), stream)
        _lib.check(rc, "cave_hip_sp_grid_solve")

    forms = {"solve": 4 * N * d + 4 * N * d, "solve_eval": 2 * 4 * N * d + 4 * N * d, "solve_cones": 4 * N * d + 4 * N * d + 8 * 5 * d * N}
    for f in forms:
        for _ in range(3):
            launch(f)
        torch.cuda.synchronize()
        assert bool((status == 0).all()), f

    def rep_us(form):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        launch(form)
        torch.cuda.synchronize()
        for a, b in evs:
            a.record()
            for _ in range(args.group):
                launch(form)
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / args.group for a, b in evs)
        return 1e3 * t[len(t) // 2]

    samples = {f: [] for f in forms}
    for _ in range(args.reps):
        for f in forms:
            samples[f].append(rep_us(f))
    kernel = {}
    for f, nbytes in forms.items():
        s = sorted(samples[f])
        med = s[len(s) // 2]
        rate = nbytes / (med * 1e-6)
        kernel[f] = {"us": round(med, 2), "spread_us": round(s[-1] - s[0], 2), "repetitions_us": [round(x, 2) for x in samples[f]],
                     "bytes_moved": nbytes, "achieved_TB_per_s": round(rate / 1e12, 3), "share_of_hbm_peak": round(rate / HBM_PEAK, 3)}

    # ---- regret evaluation end to end: the device route (wall clock, ends in the scalar's read-back) and the host route
    z = np.asarray([tight.sp_solve(c, h, w)[1] for c in true[:sample]], np.float64)  # host objectives of the sample
    sols_t, objs_t = tight.sp_solve_hip(c_true, h, w)
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
        return r, sorted(out)[len(out) // 2]

    tight.sp_regret(c_pred, c_true, z32, h, w, device=dev)  # warm-up
    r_dev, t_dev = wall(lambda: tight.sp_regret(c_pred, c_true, z32, h, w, device=dev), 9)
    r_dev_h, t_dev_h = wall(lambda: tight.sp_regret(pred, true, z32_host, h, w, device=dev), 9)
    r_host, t_host = wall(lambda: tight.sp_regret(pred, true, z32_host, h, w), 1)
    bound = (h + w) * 2.0 ** -23 * (1.0 + abs(r_host))   # positive costs: sum c . w(c_hat) / sum z = 1 + regret
    assert abs(r_dev - r_host) <= bound and abs(r_dev_h - r_host) <= bound, (r_dev, r_dev_h, r_host)

    # ---- the data set's solve loop: host on a sample (extrapolated), device on the full set
    _, t_ds_host = wall(lambda: tight.SPConeDataset(feats[:sample], true[:sample], h, w), 1)
    tight.SPConeDataset(feats, true, h, w, device=dev)
    _, t_ds_dev = wall(lambda: tight.SPConeDataset(feats, true, h, w, device=dev), 5)

    res = {"tool": "tools/diag/sp_grid.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "config": f"SP {h}x{w} (d = {d}), N = {N}, sp_gen_data costs",
           "timing": f"kernel: HIP events around groups of {args.group} launches, per repetition the median of {args.groups} groups, "
                     f"{args.reps} repetitions per form, forms alternating, spread = max - min; end to end: wall clock around "
                     "calls that end in a device synchronise, median of 9 (device) / one run (host)",
           "hbm_peak_TB_per_s": HBM_PEAK / 1e12, "kernel": kernel,
           "regret_evaluation": {"host_sp_regret_s": round(t_host, 3), "device_sp_regret_inputs_on_device_s": round(t_dev, 6),
                                 "device_sp_regret_inputs_on_host_s": round(t_dev_h, 6), "regret_host": r_host, "regret_device": r_dev,
                                 "difference": abs(r_dev - r_host), "bound": bound},
           "dataset_build": {"host_sample_instances": sample, "host_sample_s": round(t_ds_host, 3),
                             "host_extrapolated_to_N_s": round(t_ds_host * N / sample, 1),
                             "host_extrapolated_dense_ctrs_bytes": int((2 * h * w + d) * d * 4) * N,
                             "device_full_set_s": round(t_ds_dev, 6), "device_cones_bytes": 8 * 5 * d * N},
           "conditions": {"device_regret_faster_than_host": bool(t_dev_h < t_host)}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["conditions"]["device_regret_faster_than_host"] else 1


if __name__ == "__main__":
    sys.exit(main())
