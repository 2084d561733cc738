#!/usr/bin/env python
"""End-to-end CaVE training with `solver='hip'` — the loop of the reference's code_sample.py:23-60 (linear
predictor, Adam lr 1e-2, CaVE+ loss), no Gurobi / PyEPO needed.  Default: the grid shortest path at
BASELINE configs[0] sizes (5x5 grid, 100 instances, batch 32); `--problem tsp` is code_sample.py's own problem
(DFJ TSP) at a size the Held-Karp / HiGHS tight-cone builder of cave_amd/tight.py handles exactly; `--problem vrp` is the
reference's CVRP model (2-degree rows, rounded-capacity cuts), solved by the dynamic program of the same module.

    python examples/train_sp_cave.py [--grid 5 5] [--num-data 100] [--batch 32] [--epochs 10] [--packed]
    python examples/train_sp_cave.py --problem tsp --nodes 10 --packed --warm-start
    python examples/train_sp_cave.py --grid 30 30 --num-data 64 --batch 32 --epochs 3 --packed --inner ipm
    python examples/train_sp_cave.py --inner apgd [--sparse] [--apgd-iters 200]  # CaVE+ with the reference's APGD projector on the device
    python examples/train_sp_cave.py --packed --graph          # the whole step (predictor, loss, backward, Adam) as one HIP graph
    python examples/train_sp_cave.py --problem tsp --prefetch  # dense cones: the next batch's pack rides in this batch's loss call
    python examples/train_sp_cave.py --sparse [--packed]       # cones on the sparse wire format: no dense padding anywhere
    python examples/train_sp_cave.py --problem tsp --sparse --prefetch [--warm-start]  # the fused step packs the next SPARSE batch
    python examples/train_sp_cave.py --grid 30 30 --num-data 1000 --device-data --packed --inner ipm  # SP solved, cones built and regret evaluated on the device
    python examples/train_sp_cave.py --problem tsp --nodes 12 --packed --device-regret  # the regret's Held-Karp solves run on the device
    python examples/train_sp_cave.py --problem tsp --nodes 20 --num-data 64 --packed --device-regret  # TSP-20: above 14 nodes only the device solves exactly
    python examples/train_sp_cave.py --problem vrp --nodes 10 --capacity 30 --vehicles 3 --packed --device-regret --device-data  # CVRP: solved on the device
    python examples/train_sp_cave.py --problem tsp --nodes 10 --sparse --device-cones  # TSP: the tight cones are written on the device, no dense matrix
    python examples/train_sp_cave.py --problem vrp --nodes 16 --capacity 40 --vehicles 3 --num-data 32 --packed --device-regret --device-data  # CVRP-15: above 14 nodes only the device solves exactly
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch
from torch import nn
from torch.utils.data import DataLoader


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=[5, 5])
    ap.add_argument("--num-data", type=int, default=100)
    ap.add_argument("--num-feat", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--variant", default="inner", choices=["exact", "inner", "hybrid"])
    ap.add_argument("--packed", action="store_true", help="device-resident packed cones instead of dense padding")
    ap.add_argument("--problem", default="sp", choices=["sp", "tsp", "vrp"])
    ap.add_argument("--nodes", type=int, default=10, help="TSP / CVRP size, the depot included (Held-Karp: <= 14; the TSP up to 20 with --device-regret, "
                                                              "the device's wide Held-Karp tier; the CVRP up to 20 with --device-regret "
                                                              "AND --device-data, the device's wide CVRP tier: above 14 nodes no host "
                                                              "solver reaches the data set's optima or the regret's)")
    ap.add_argument("--capacity", type=float, default=30.0, help="CVRP: vehicle capacity (demands are uniform on [0, 10))")
    ap.add_argument("--vehicles", type=int, default=3, help="CVRP: number of vehicles")
    ap.add_argument("--inner", default="push", choices=["push", "ipm", "apgd"],
                    help="CaVE+ interior point: 'push' (nnls-style: exact projection pushed towards the average normal), "
                         "'ipm' (truncated interior-point iterate, as the reference's Clarabel max_iter=3: src/cave.py:213-214) or "
                         "'apgd' (the truncated iterate of the reference's APGD projector, src/qpsolver.py:11-110, --apgd-iters "
                         "iterations; dense or --sparse cones, not --packed: a store holds reduced cones)")
    ap.add_argument("--apgd-iters", type=int, default=200, help="iterations of --inner apgd (solver_kwargs['max_iters'])")
    ap.add_argument("--max-iter", type=int, default=3, help="interior-point steps of --inner ipm")
    ap.add_argument("--warm-start", action="store_true",
                    help="start each projection from the multipliers of the previous epoch (packed store, or dense / --sparse "
                         "cones through solver_kwargs={'warm_start': True})")
    ap.add_argument("--graph", action="store_true",
                    help="(with --packed, not hybrid) capture predictor + loss + backward + Adam of a full batch in ONE HIP "
                         "graph and replay it per step (the C-ABI launch path allocates nothing and never syncs when the "
                         "status check is off); a ragged last batch runs eagerly")
    ap.add_argument("--prefetch", action="store_true",
                    help="(dense or --sparse cones, not --packed) wrap the DataLoader in cave_amd.dataset.prefetch: the loop body "
                         "stays as it is and the pack stage of batch i+1 rides in the launch of batch i's loss")
    ap.add_argument("--sparse", action="store_true",
                    help="the dataset hands out cones on the sparse wire format (cave_amd.sparse.SparseCones) and the loader "
                         "collates them with collate_sparse; with --packed the store is built by ConeStore.from_sparse")
    ap.add_argument("--lazy-check", action="store_true", help="solver_kwargs check='lazy': no host sync per step")
    ap.add_argument("--device-data", action="store_true",
                    help="(shortest path, with --packed or --sparse) solve the instances, build their tight cones on the sparse "
                         "wire format and evaluate the regret on the device (SPConeDataset(..., device=), sp_regret(..., "
                         "device=)): no dense cone is ever made; (CVRP) solve the data set's instances on the device "
                         "(VRPConeDataset(..., device=)), the cut loop stays on the host")
    ap.add_argument("--device-regret", action="store_true",
                    help="evaluate the regret on the device (tsp_regret / vrp_regret / sp_regret(..., device=)): one launch "
                         "solves every prediction and prices it, only the scalar comes back; the dataset and the training "
                         "loop are untouched")
    ap.add_argument("--device-cones", action="store_true",
                    help="(TSP / CVRP, with --sparse or --packed) write the data set's tight cones on the device, on the sparse "
                         "wire format (TSPConeDataset(..., device=), VRPConeDataset(..., device=, cones='sparse'): "
                         "tight.tight_cones_hip): no dense cone is ever made; the cut loop stays on the host")
    args = ap.parse_args(argv)
    if args.device_cones and (args.problem == "sp" or not (args.packed or args.sparse)):
        ap.error("--device-cones is for --problem tsp and --problem vrp, where it needs --sparse or --packed (there are no dense "
                 "cones); the shortest path has --device-data")
    if args.device_data and (args.problem == "tsp" or (args.problem == "sp" and not (args.packed or args.sparse))):
        ap.error("--device-data is for the shortest-path problem, where it needs --packed or --sparse (there are no dense "
                 "cones), and for the CVRP")
    if args.problem == "tsp" and args.nodes > 14 and not (args.nodes <= 20 and args.device_regret):
        ap.error("--problem tsp takes --nodes up to 20, and above 14 nodes it needs --device-regret: the host's Held-Karp stops "
                 "at 14 nodes, the regret's exact tours then come from the device (tsp_regret(..., device=))")
    if args.problem == "vrp" and args.nodes > 14 and not (args.nodes <= 20 and args.device_regret and args.device_data):
        ap.error("--problem vrp takes --nodes up to 20, and above 14 nodes it needs --device-regret and --device-data: the host's "
                 "dynamic program stops at 14 nodes, the data set's optima and the regret's exact routes then come from the device "
                 "(VRPConeDataset(..., device=), vrp_regret(..., device=))")
    if args.inner == "apgd" and (args.packed or args.variant == "exact"):
        ap.error("--inner apgd is for the inner and hybrid variants on dense or --sparse cones: it iterates on the rows of the "
                 "wire format as they are, and a packed store holds reduced cones")
    sp_device = args.device_data and args.problem == "sp"
    if args.graph and (not args.packed or args.variant == "hybrid"):
        ap.error("--graph needs --packed and a variant without a per-call branch draw")

    from cave_amd.cave import EPO, exactConeAlignedCosine, innerConeAlignedCosine
    from cave_amd.dataset import ConeStore, PackedBatch, collate_sparse, prefetch
    from cave_amd.sparse import SparseCones
    from cave_amd.tight import (SPConeDataset, TSPConeDataset, VRPConeDataset, sp_gen_data, sp_regret, tsp_gen_data, tsp_regret,
                                vrp_gen_data, vrp_regret)
    from torch.nn.utils.rnn import pad_sequence

    h, w = args.grid
    if args.problem == "tsp":
        feats, costs = tsp_gen_data(args.num_data, args.num_feat, args.nodes, deg=4, noise_width=0.5, seed=42)
        dataset = TSPConeDataset(feats, costs, args.nodes, device="cuda" if args.device_cones else None)
        print(f"TSP-{args.nodes}: {len(dataset)} instances, {sum(dataset.tight_cuts)} tight subtour cuts in all")
    elif args.problem == "vrp":
        feats, costs, demands = vrp_gen_data(args.num_data, args.num_feat, args.nodes, deg=4, noise_width=0.5, seed=42)
        dataset = VRPConeDataset(feats, costs, args.nodes, demands, args.capacity, args.vehicles,
                                 device="cuda" if args.device_data or args.device_cones else None,
                                 cones="sparse" if args.device_cones else "dense")
        print(f"CVRP-{args.nodes - 1} (capacity {args.capacity:g}, {args.vehicles} vehicles): {len(dataset)} instances, "
              f"{sum(dataset.tight_cuts)} tight rounded-capacity cuts in all")
    else:
        feats, costs = sp_gen_data(args.num_data, args.num_feat, h, w, deg=4, noise_width=0.5, seed=135)
        dataset = SPConeDataset(feats, costs, h, w, device="cuda" if args.device_data else None)
    dev = torch.device("cuda")

    class _Model:  # what the loss modules read from a PyEPO optModel
        modelSense = EPO.MINIMIZE

    kw = {}
    if args.inner != "push":
        kw["inner"] = args.inner
    if args.inner == "apgd":
        kw["max_iters"] = args.apgd_iters
    if args.graph:
        kw["check"] = False   # (a captured step cannot read the status back; it is examined after each replay below)
    elif args.lazy_check:
        kw["check"] = "lazy"
    if args.warm_start and not args.packed:
        kw["warm_start"] = True   # dense or sparse batches: the loss module's multiplier cache, keyed by cone content
    if args.variant == "exact":
        cave = exactConeAlignedCosine(_Model(), solver="hip", solver_kwargs=kw or None)
    elif args.variant == "inner":
        cave = innerConeAlignedCosine(_Model(), solver="hip", seed=0, max_iter=args.max_iter, solver_kwargs=kw or None)
    else:
        cave = innerConeAlignedCosine(_Model(), solver="hip", solve_ratio=0.3, inner_ratio=0.2, seed=0, solver_kwargs=kw or None)

    # --sparse: what a dataset built from a solver's sparse constraint matrix would keep -- one SparseCones per instance
    dev_cones = sp_device or args.device_cones
    if dev_cones:
        sparse_ctrs = dataset.cones   # already on the device, straight from the solve kernel / the tight-cone kernels
    else:
        sparse_ctrs = SparseCones.from_ragged(dataset.ctrs) if args.sparse else None
    if args.packed:
        store = ConeStore.from_sparse(sparse_ctrs) if sparse_ctrs is not None else ConeStore.from_ragged(dataset.ctrs)
    else:
        store = None
    if store is not None and args.warm_start:
        store.enable_warm_start()

    def collate(batch):  # reference collate_fn (src/dataset.py:133-144) / its id-returning replacement
        idx = torch.as_tensor(batch, dtype=torch.int64)
        x, c = dataset.feats[idx.to(dataset.feats.device)], dataset.costs[idx.to(dataset.costs.device)]
        if args.packed:
            return x, c, idx
        if dev_cones:
            return x, c, sparse_ctrs[idx]   # one gather on the device
        if args.sparse:
            return collate_sparse([(x[j], c[j], sparse_ctrs[i]) for j, i in enumerate(batch)])
        return x, c, pad_sequence([dataset.ctrs[i] for i in batch], batch_first=True, padding_value=0.0)

    loader = DataLoader(list(range(len(dataset))), batch_size=args.batch, shuffle=True, collate_fn=collate,
                        generator=torch.Generator().manual_seed(0))
    d = dataset.costs.shape[1]
    torch.manual_seed(0)
    reg = nn.Linear(args.num_feat, d).to(dev)
    opt = torch.optim.Adam(reg.parameters(), lr=1e-2, capturable=args.graph)

    graph = None
    if args.graph:
        # static inputs of the captured step; three warm-up steps on a side stream (as torch.cuda.graph wants), the
        # capture, then parameters and Adam state back to their initial values IN PLACE (the graph holds their addresses)
        gx = torch.zeros(args.batch, args.num_feat, device=dev)
        gids = torch.zeros(args.batch, dtype=torch.int64, device=dev)
        gbatch = PackedBatch(store, gids)
        init = [p_.detach().clone() for p_ in reg.parameters()]

        def gstep():
            loss = cave(reg(gx), gbatch)
            opt.zero_grad(set_to_none=False)
            loss.backward()
            opt.step()
            return loss

        x0, _, i0 = next(iter(loader))
        if len(i0) == args.batch:
            gx.copy_(x0)
            gids.copy_(i0)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    gstep()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                gloss = gstep()
            with torch.no_grad():
                for p_, p0 in zip(reg.parameters(), init):
                    p_.copy_(p0)
                    if p_.grad is not None:
                        p_.grad.zero_()
                for st_ in opt.state.values():
                    for v_ in st_.values():
                        if torch.is_tensor(v_):
                            v_.zero_()
            if store is not None and args.warm_start:
                store.reset_warm_start()
            loader = DataLoader(list(range(len(dataset))), batch_size=args.batch, shuffle=True, collate_fn=collate,
                                generator=torch.Generator().manual_seed(0))  # the same batch order as an eager run

    def regret():
        if sp_device:  # predictions and true costs stay on the device, only the scalar comes back
            with torch.no_grad():
                return sp_regret(reg(dataset.feats), dataset.costs, dataset.objs[:, 0], h, w, device=dev)
        if args.device_regret:  # a host dataset: costs and objectives go to the device, the predictions are there already
            with torch.no_grad():
                cp = reg(dataset.feats.to(dev))
                if args.problem == "tsp":
                    return tsp_regret(cp, dataset.costs, dataset.objs[:, 0], args.nodes, device=dev)
                if args.problem == "vrp":
                    return vrp_regret(cp, dataset.costs, dataset.objs[:, 0], args.nodes, demands, args.capacity, args.vehicles,
                                      device=dev)
                return sp_regret(cp, dataset.costs, dataset.objs[:, 0], h, w, device=dev)
        with torch.no_grad():
            cp = reg(dataset.feats.to(dev)).cpu().numpy()
        if args.problem == "tsp":  # (.cpu(): with --device-cones the data set lives on the device)
            return tsp_regret(cp, dataset.costs.cpu().numpy(), dataset.objs.cpu().numpy()[:, 0], args.nodes)
        if args.problem == "vrp":
            return vrp_regret(cp, dataset.costs.cpu().numpy(), dataset.objs.cpu().numpy()[:, 0], args.nodes, demands, args.capacity,
                              args.vehicles)
        return sp_regret(cp, dataset.costs.numpy(), dataset.objs.numpy()[:, 0], h, w)

    hist = [(0, float("nan"), regret())]
    print(f"epoch 0: regret {hist[0][2] * 100:.2f}%")
    t0 = time.time()
    iters_log = []
    hit_log = []   # dense cones with --warm-start: share of the epoch's instances that started from cached multipliers
    for epoch in range(1, args.epochs + 1):
        tot = 0.0
        it_sum, it_max, it_n = 0.0, 0, 0
        hit_sum, hit_n = 0.0, 0
        for x, c, cones in (prefetch(loader) if args.prefetch and not args.packed else loader):
            if graph is not None and len(x) == args.batch:
                gx.copy_(x, non_blocking=True)
                gids.copy_(cones, non_blocking=True)
                graph.replay()
                loss = gloss
                if bool((store.last_status != 0).any()):
                    raise RuntimeError("solver='hip': a projection of the captured step failed")
            else:
                x = x.to(dev)
                cp = reg(x)
                loss = cave(cp, PackedBatch(store, cones) if args.packed else cones.to(dev))
                opt.zero_grad()
                loss.backward()
                opt.step()
            tot += float(loss.detach()) * len(x)
            src = store if store is not None else getattr(cave, "_warm", None)
            if store is None and src is not None and src.last_hit is not None:
                hit_sum, hit_n = hit_sum + float(src.last_hit.float().sum()), hit_n + src.last_hit.numel()
            if src is not None and getattr(src, "last_iters", None) is not None:
                li = src.last_iters
                it_sum, it_max, it_n = it_sum + float(li.sum()), max(it_max, int(li.max())), it_n + li.numel()
        hist.append((epoch, tot / len(dataset), regret()))
        extra = ""
        if it_n:
            iters_log.append((it_sum / it_n, it_max))
            extra = f"  Newton iterations mean {it_sum / it_n:.2f} max {it_max}"
        if hit_n:
            hit_log.append(hit_sum / hit_n)
            extra += f"  warm hits {100 * hit_sum / hit_n:.0f}%"
        print(f"epoch {epoch}: loss {hist[-1][1]:.4f}  regret {hist[-1][2] * 100:.2f}%{extra}")
    main.iters_log = iters_log
    main.hit_log = hit_log
    print(f"training time {time.time() - t0:.2f} s ({args.epochs} epochs, {len(dataset)} instances, batch {args.batch})")
    return hist


if __name__ == "__main__":
    main()
