#!/usr/bin/env python
"""Writes tests/golden/vrp_dp_wide.npz: for (n, K) = (18, 3), (20, 2), (20, 3) three instances (one `gen`, one `ties`, one
`signed`; tests/vrp_dp_cases.instance_of with seed 5) with the routes and objectives of the numpy restatement of the
CVRP dynamic program (tests/vrp_dp_wide_cases.solve_ref, which tests/test_vrp_dp_wide_emul.py checks against
tight.vrp_solve at n <= 12), and the objective tight.vrp_rcc_cuts finds for the `gen` instance of
vrp_dp_wide_cases.GOLDEN_RCC, which must equal the dynamic program's.  Every instance is feasible (solve_ref raises
otherwise) and every `ties` instance has a load equal to its capacity (asserted).

Runtime on one core: about 25 s -- 2.4 s and 1.4 s for n = 18 and n = 20 at K = 2, 19 s for n = 20 at K = 3 (one stored
layer, 3^19 / 2 pairs per instance), and 0.3 s for the cut loop (HiGHS) at n = 20.

    python tests/golden/make_vrp_dp_wide.py
"""

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import vrp_dp_cases as VC  # noqa: E402
import vrp_dp_wide_cases as WC  # noqa: E402
from cave_amd import tight  # noqa: E402


def main():
    out = {}
    for n, K in WC.GOLDEN_SHAPES:
        t0 = time.time()
        inst = WC.golden_instances(n, K)
        for kind, (_, q, cap) in zip(WC.KINDS, inst):
            WC.check_instance(kind, q, cap, n)
        res = [WC.solve_ref(c, n, q, cap, K) for c, q, cap in inst]
        t = f"{n}_{K}"
        out["costs" + t] = np.stack([c for c, _, _ in inst]).astype(np.float32)
        out["demands" + t] = np.stack([q for _, q, _ in inst]).astype(np.float32)
        out["caps" + t] = np.asarray([cap for _, _, cap in inst], np.float64)
        out["routes" + t] = np.stack([VC.pad_routes(r, n, K) for _, _, r in res])
        out["objs" + t] = np.asarray([o for _, o, _ in res], np.float64)
        assert np.isfinite(out["objs" + t]).all()
        print(n, K, out["objs" + t], f"{time.time() - t0:.1f} s", flush=True)
    n, K = WC.GOLDEN_RCC
    t0 = time.time()
    c, q, cap = WC.golden_instances(n, K)[0]
    _, rcc, _ = tight.vrp_rcc_cuts(c, n, q, cap, K)
    print("vrp_rcc_cuts", n, K, rcc, f"{time.time() - t0:.1f} s", flush=True)
    z = out[f"objs{n}_{K}"][0]  # another algorithm, the same optimum: the same n - 1 + k positive terms summed in another order
    assert abs(rcc - z) <= (n + K) * 2.0 ** -52 * abs(z), (rcc, z)
    out[f"rcc{n}_{K}"] = np.float64(rcc)
    np.savez_compressed(WC.GOLDEN, **out)
    print("wrote", WC.GOLDEN, os.path.getsize(WC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
