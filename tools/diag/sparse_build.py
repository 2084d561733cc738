#!/usr/bin/env python
"""Sparse wire format against the dense route: store build time / peak device memory, and the pack kernel.

    python tools/diag/sparse_build.py [--quick]      -> one JSON line on stdout

store_build   ConeStore.from_sparse(SparseCones) against ConeStore.from_chunks_lazy(densify_on), for the batches of
              bench.py's other_configs (TSP-50 B = 512, TSP-100 B = 512, SP 30x30 B = 1024; the dense route at the chunk
              sizes bench.py uses).  Wall time host + device, synchronised; peak device memory above what was allocated
              before the build (torch.cuda.max_memory_allocated).  `host_prep_s` is SparseCones.from_coo (sorting on the
              host), paid once per dataset and not part of the sparse figure's `wall_s`; the coordinate lists themselves
              are an input of both routes.
pack_kernel   cave_hip_pack_fill_sparse against cave_hip_pack_fill, slot mode, four waves, TSP-20 B = 1024, launches
              rotating over 4 batches of distinct cones (4096 cones, 4 x 183 MB dense: more than the Infinity Cache),
              HIP events around each launch, median over `launches`.  And the two-launch step on top of them:
              cone_op_sparse against cone_op_dense (check=False, mode INNER), events around each call.
`sane` is the one condition the loader has to meet: the sparse fill's median is below the dense fill's.
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch


def _median_ms(fn, n, rotate):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i in range(8):
        fn(i % rotate)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(i % rotate)
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def store_build(dev, kind, size, B, chunk):
    from cave_amd import synth
    from cave_amd.dataset import ConeStore
    from cave_amd.sparse import SparseCones

    items, costs, _ = synth.coo_batch(kind, size, B, seed=0)
    d = int(costs.shape[1])
    m_max = max(it[3] for it in items)
    t0 = time.perf_counter()
    sc = SparseCones.from_coo(items, d)
    host_prep = time.perf_counter() - t0
    out = {"name": f"{kind}{size} B={B}", "d": d, "m_max": m_max, "nnz": sc.nnz, "sparse_input_bytes": sc.nbytes,
           "dense_input_bytes": 4 * B * m_max * d, "host_prep_s": round(host_prep, 4)}
    stores = {}
    for route in ("sparse", "dense"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        if route == "sparse":
            st = ConeStore.from_sparse(sc)
        else:
            st = ConeStore.from_chunks_lazy(lambda i: synth.densify_on(items[i:i + chunk], d, dev, m_max), list(range(0, B, chunk)))
        torch.cuda.synchronize()
        out[route] = {"wall_s": round(time.perf_counter() - t0, 4),
                      "peak_bytes": int(torch.cuda.max_memory_allocated() - base), "store_bytes": int(st.nbytes())}
        if route == "dense":
            out[route]["chunk"] = chunk
        stores[route] = st
    # (different chunkings may pack a chunk with a different kernel shape; the index arrays do not depend on it)
    out["same_structure"] = all(torch.equal(stores["sparse"].t[k], stores["dense"].t[k])
                                for k in ("row_off", "nnz_off", "ccol", "cvar", "cptr", "vkind", "usign"))
    out["wall_ratio_dense_over_sparse"] = round(out["dense"]["wall_s"] / out["sparse"]["wall_s"], 2)
    out["peak_ratio_dense_over_sparse"] = round(out["dense"]["peak_bytes"] / max(1, out["sparse"]["peak_bytes"]), 2)
    return out


def pack_kernel(dev, launches, rotate=4, B=1024):
    from cave_amd import _lib, synth
    from cave_amd.qpsolver import MODE_INNER, _SlotStore, cone_op_dense, cone_op_sparse
    from cave_amd.sparse import SparseCones

    lib = _lib.load()
    items, costs, _ = synth.coo_batch("tsp", 20, rotate * B, seed=0)
    d = int(costs.shape[1])
    m = max(it[3] for it in items)
    sparse = [SparseCones.from_coo(items[r * B:(r + 1) * B], d, m_max=m).cuda() for r in range(rotate)]
    dense = [s.densify() for s in sparse]
    preds = [torch.tensor(costs[r * B:(r + 1) * B], device=dev) for r in range(rotate)]
    refs = [s.c_ref() for s in sparse]
    ss = _SlotStore(dev, B, d)
    stream = _lib.current_stream()

    def fill_sparse(r):
        _lib.check(lib.cave_hip_pack_fill_sparse(refs[r], 0, 0, 4, ss.ref, 0, _lib.ptr(ss.pack_status), stream), "fill_sparse")

    def fill_dense(r):
        _lib.check(lib.cave_hip_pack_fill(_lib.ptr(dense[r]), B, m, d, 0, 0, 4, ss.ref, 0, _lib.ptr(ss.pack_status), stream), "fill")

    out = {"config": f"TSP-20 B={B}, {rotate} rotating batches of distinct cones", "launches": launches,
           "sparse_bytes_per_batch": sparse[0].nbytes, "dense_bytes_per_batch": 4 * B * m * d}
    ms, lo, hi = _median_ms(fill_sparse, launches, rotate)
    assert bool((ss.pack_status == 0).all())
    out["fill_sparse_us"] = {"median": round(1e3 * ms, 1), "min": round(1e3 * lo, 1), "max": round(1e3 * hi, 1)}
    md, lo, hi = _median_ms(fill_dense, launches, rotate)
    assert bool((ss.pack_status == 0).all())
    out["fill_dense_us"] = {"median": round(1e3 * md, 1), "min": round(1e3 * lo, 1), "max": round(1e3 * hi, 1)}
    out["fill_ratio_dense_over_sparse"] = round(md / ms, 2)
    # the two-launch step (one checked call each settles the shape first)
    o1 = cone_op_dense(dense[0], preds[0], MODE_INNER, -1.0, 0.2, outputs=("loss", "grad"))
    o2 = cone_op_sparse(sparse[0], preds[0], MODE_INNER, -1.0, 0.2, outputs=("loss", "grad"))
    out["step_outputs_bit_equal"] = bool(torch.equal(o1["loss"], o2["loss"]) and torch.equal(o1["grad"], o2["grad"]))
    ms2, lo, hi = _median_ms(lambda r: cone_op_sparse(sparse[r], preds[r], MODE_INNER, -1.0, 0.2, check=False, outputs=("loss", "grad")),
                             launches, rotate)
    out["step_sparse_us"] = {"median": round(1e3 * ms2, 1), "min": round(1e3 * lo, 1), "max": round(1e3 * hi, 1)}
    md2, lo, hi = _median_ms(lambda r: cone_op_dense(dense[r], preds[r], MODE_INNER, -1.0, 0.2, check=False, outputs=("loss", "grad")),
                             launches, rotate)
    out["step_dense_us"] = {"median": round(1e3 * md2, 1), "min": round(1e3 * lo, 1), "max": round(1e3 * hi, 1)}
    out["step_ratio_dense_over_sparse"] = round(md2 / ms2, 2)
    out["sane"] = bool(ms < md)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small batches (a functional run of the driver, not a measurement)")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--skip-build", action="store_true")
    args = ap.parse_args(argv)
    from cave_amd import _lib

    _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"tool": "tools/diag/sparse_build.py", "device": torch.cuda.get_device_name(dev), "quick": bool(args.quick)}
    res["pack_kernel"] = pack_kernel(dev, max(20, args.launches), B=128 if args.quick else 1024)
    if not args.skip_build:
        specs = [("tsp", 50, 512, 32), ("tsp", 100, 512, 4), ("sp", (30, 30), 1024, 32)]
        if args.quick:
            specs = [("tsp", 50, 32, 16), ("tsp", 100, 8, 4), ("sp", (30, 30), 16, 8)]
        store_build(dev, "tsp", 20, 64, 32)  # (runtime and allocator warm-up, not reported)
        res["store_build"] = [store_build(dev, *s) for s in specs]
    print(json.dumps(res))
    return 0 if res["pack_kernel"]["sane"] else 1


if __name__ == "__main__":
    sys.exit(main())
