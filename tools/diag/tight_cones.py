#!/usr/bin/env python
"""The tight-cone kernels (cave_hip_tight_cones_count / _fill, cave_amd/csrc/tight_cones.h) timed against the host route
they replace, in one process on one device -> profiles/tight_cones.json.

    python tools/diag/tight_cones.py [--quick] [--out profiles/tight_cones.json]

Cases (vertices on the device, systems moved there once):
  tsp20    TSP-20 (d = 190), N = 1024: random tours; per instance two lazy subtour rows, a segment of its tour (tight) and a
           random node set; system tight.tsp_system(20)
  sp30     SP 30x30 (d = 1740), N = 1024: the shortest paths of sp_gen_data costs (tight.sp_solve_hip); tight.sp_system(30, 30)
  tsp100   TSP-100 (d = 4950), N = 512: as tsp20 with segments of 30 nodes and sets of 50
Device figure: the count launch and the fill launch through the C ABI, the exclusive scan made beforehand (it is a
torch.cumsum in the package).  HIP events around groups of `--group` count + fill pairs; `--batches` input batches of the
case rotate from pair to pair, so no pair finds its own vertices in the caches; the figure of a repetition is the median
group time per pair; `--reps` repetitions per case, the cases alternating; reported: the median of the repetitions and
their spread (max - min).  Beside it `tight_cones_hip` end to end (wall clock: count, cumsum, the one host read,
allocation, fill), median of 9.  Every case is checked against the host route on the sample before it is timed.

Host route, same run, same machine: `tsp_tight_normals` / `sp_tight_normals` per instance + `SparseCones.from_ragged` +
upload, wall clock on a stated sample of the batch, EXTRAPOLATED to the batch (labelled so).
No condition is attached: the figures are reported as measured.
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
    ap.add_argument("--quick", action="store_true", help="N = 32 and small samples (a functional run of the driver)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--group", type=int, default=12)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tight_cones.json"))
    args = ap.parse_args(argv)

    import ctypes as C

    import numpy as np
    import torch

    from cave_amd import _lib, tight
    from cave_amd.sparse import SparseCones

    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    p, stream = _lib.ptr, _lib.current_stream()
    rng = np.random.RandomState(5)

    def tsp_batch(n, N, seg, loose):
        """random tours as edge indicators, and per instance a tight and a (most likely) slack subtour set"""
        eid = tight._edge_index(n)[1]
        sols, cuts = np.zeros((N, n * (n - 1) // 2), np.float32), []
        for b in range(N):
            tour = np.r_[0, 1 + rng.permutation(n - 1)]
            sols[b, eid[tour, np.roll(tour, -1)]] = 1.0
            at = int(rng.randint(0, n - seg))
            cuts.append([sorted(int(v) for v in tour[at:at + seg]), sorted(int(v) for v in rng.choice(n, loose, replace=False))])
        return sols, cuts

    def make_case(name, N, sample):
        batches = []
        for i in range(args.batches):
            if name == "sp30":
                costs = torch.tensor(tight.sp_gen_data(N, 5, 30, 30, seed=135 + i)[1], device=dev)
                sols, cuts = tight.sp_solve_hip(costs, 30, 30)[0], None
                lazy = None
            else:
                n, seg, loose = (20, 6, 8) if name == "tsp20" else (100, 30, 50)
                host_sols, cuts = tsp_batch(n, N, seg, loose)
                sols, lazy = torch.tensor(host_sols, device=dev), tight.cut_rows(n, cuts)
            batches.append((sols, cuts, lazy))
        system = tight.sp_system(30, 30) if name == "sp30" else tight.tsp_system(20 if name == "tsp20" else 100)
        return {"name": name, "N": N, "sample": min(sample, N), "system": system, "batches": batches}

    def host_route(case, sols, cuts, count):
        """the route the kernels replace, on the first `count` instances -> (SparseCones on the device, seconds)"""
        host = sols[:count].cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if case["name"] == "sp30":
            mats = [tight.sp_tight_normals(s, 30, 30) for s in host]
        else:
            n = 20 if case["name"] == "tsp20" else 100
            mats = [tight.tsp_tight_normals(s, n, k) for s, k in zip(host, cuts)]
        cones = SparseCones.from_ragged(mats).to(dev)
        torch.cuda.synchronize()
        return cones, time.perf_counter() - t0

    def prepare(case):
        """per batch: the C structs, the counted offsets and the output tensors; the sample checked against the host route"""
        sys_c, keep = case["system"].to(dev)
        runs = []
        for sols, cuts, lazy in case["batches"]:
            N = sols.shape[0]
            lazy_c, off = (None, None) if lazy is None else (lazy[0].to(dev)[0], torch.from_numpy(lazy[1]).to(dev))
            ref = lambda c: None if c is None else C.byref(c)  # noqa: E731
            n_rows = torch.empty(N, dtype=torch.int32, device=dev)
            n_ent = torch.empty(N, dtype=torch.int64, device=dev)
            status = torch.empty(N, dtype=torch.int32, device=dev)
            cones = tight.tight_cones_hip(case["system"], sols, lazy)
            key, val = torch.empty_like(cones.key), torch.empty_like(cones.val)

            def pair(sols=sols, lazy_c=lazy_c, off=off, N=N, n_rows=n_rows, n_ent=n_ent, status=status, cones=cones, key=key, val=val):
                _lib.check(lib.cave_hip_tight_cones_count(C.byref(sys_c), ref(lazy_c), p(off), p(sols), N, 1e-5, p(n_rows), p(n_ent),
                                                          p(status), stream), "cave_hip_tight_cones_count")
                _lib.check(lib.cave_hip_tight_cones_fill(C.byref(sys_c), ref(lazy_c), p(off), p(sols), N, 1e-5, p(cones.ent_off),
                                                         cones.nnz, p(key), p(val), p(status), stream), "cave_hip_tight_cones_fill")

            pair()
            torch.cuda.synchronize()
            assert bool((status == 0).all()) and torch.equal(key, cones.key) and torch.equal(val, cones.val), case["name"]
            runs.append((pair, cones, keep, lazy_c, off))
        sols, cuts, lazy = case["batches"][0]
        k = case["sample"]
        want, t_host = host_route(case, sols, cuts, k)
        got = runs[0][1][0:k]
        assert got.m_max >= want.m_max and all(torch.equal(getattr(got, a), getattr(want, a)) for a in ("ent_off", "key", "val")), case["name"]
        case["runs"], case["host_sample_s"] = runs, t_host
        case["entries_per_batch"] = int(runs[0][1].nnz)
        case["rows_max"] = int(runs[0][1].m_max)

    def rep_us(case):
        pairs = [r[0] for r in case["runs"]]
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.groups)]
        pairs[0]()
        torch.cuda.synchronize()
        i = 0
        for a, b in evs:
            a.record()
            for _ in range(args.group):
                pairs[i % len(pairs)]()
                i += 1
            b.record()
        torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) / args.group for a, b in evs)
        return 1e3 * t[len(t) // 2]

    def wall(fn, reps):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return sorted(out)[len(out) // 2]

    shapes = (("tsp20", 32, 8), ("sp30", 32, 4), ("tsp100", 32, 2)) if args.quick else (("tsp20", 1024, 64), ("sp30", 1024, 16), ("tsp100", 512, 4))
    cases = [make_case(*s) for s in shapes]
    for c in cases:
        prepare(c)
    samples = {c["name"]: [] for c in cases}
    for _ in range(args.reps):
        for c in cases:
            samples[c["name"]].append(rep_us(c))
    out = {}
    for c in cases:
        s = sorted(samples[c["name"]])
        sols, _, lazy = c["batches"][0]
        e2e = wall(lambda: tight.tight_cones_hip(c["system"], sols, lazy), 9)
        host_batch = c["host_sample_s"] * c["N"] / c["sample"]
        out[c["name"]] = {"N": c["N"], "d": c["system"].d, "system_rows": c["system"].R, "system_entries": c["system"].nnz,
                          "lazy_rows_per_instance": 0 if lazy is None else 2, "cone_entries_per_batch": c["entries_per_batch"],
                          "rows_max": c["rows_max"],
                          "count_plus_fill_us": round(s[len(s) // 2], 2), "spread_us": round(s[-1] - s[0], 2),
                          "repetitions_us": [round(x, 2) for x in samples[c["name"]]],
                          "tight_cones_hip_end_to_end_us": round(1e6 * e2e, 1),
                          "host_route_sample_instances": c["sample"], "host_route_sample_s": round(c["host_sample_s"], 4),
                          "host_route_extrapolated_to_batch_s": round(host_batch, 3),
                          "host_over_device_end_to_end": round(host_batch / e2e, 1)}
    res = {"tool": "tools/diag/tight_cones.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick),
           "timing": f"count + fill: HIP events around groups of {args.group} launch pairs, {args.batches} input batches rotating, per "
                     f"repetition the median of {args.groups} groups, {args.reps} repetitions per case, cases alternating, spread = max - "
                     "min; end to end: wall clock around tight_cones_hip with a device synchronise, median of 9; host route: "
                     "*_tight_normals + SparseCones.from_ragged + upload, wall clock on the sample, extrapolated to the batch",
           "cases": out}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
