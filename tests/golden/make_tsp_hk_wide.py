#!/usr/bin/env python
"""Writes tests/golden/tsp_hk_wide.npz: for n = 18, 19, 20 three instances (one `gen`, one `ties`, one `signed`; costs from
tests/tsp_hk_cases.costs_of) with the tours and objectives of the numpy restatement of the Held-Karp recurrence
(tests/tsp_hk_wide_cases.solve_ref, which tests/test_tsp_hk_wide_emul.py checks against tight.tsp_solve at n <= 13), and
the objective tight.tsp_dfj_cuts finds for the `gen` instance.  About 15 s on one core.

    python tests/golden/make_tsp_hk_wide.py
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import tsp_hk_wide_cases as WC  # noqa: E402
from cave_amd import tight  # noqa: E402


def main():
    out = {}
    for n in WC.GOLDEN_NS:
        costs = WC.golden_costs(n)
        res = [WC.solve_ref(c, n) for c in costs]
        out[f"costs{n}"] = costs
        out[f"tours{n}"] = np.asarray([t for _, _, t in res], np.int32)
        out[f"objs{n}"] = np.asarray([o for _, o, _ in res], np.float64)
        _, dfj, _ = tight.tsp_dfj_cuts(costs[0], n)
        out[f"dfj{n}"] = np.float64(dfj)
        print(n, out[f"objs{n}"], dfj, flush=True)
    np.savez_compressed(WC.GOLDEN, **out)
    print("wrote", WC.GOLDEN, os.path.getsize(WC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
