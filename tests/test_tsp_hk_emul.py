"""CPU tier: the Held-Karp kernels (cave_amd/csrc/tsp_hk.h tsp_hk_block, 256-thread workgroups striding over the batch as
k_tsp_hk.hip launches them, both tiers) under the SIMT emulation (tests/emul/simt_tsp_hk.cpp): round robin, one shuffled
lane schedule, and once as a stand-alone program under AddressSanitizer + UBSan with exact-size buffers, LDS block and
workspace.

Oracle: tight.tsp_solve; cases and bounds: tests/tsp_hk_cases.py.  TEST INFRASTRUCTURE: nothing in cave_amd loads these
builds."""

import itertools

import numpy as np
import pytest

import tsp_hk_cases as TC
from emul_tsp_hk_lib import F_ALL, F_EVAL, F_OBJ, F_SOL, F_STATUS, F_TOUR, SimtTspHk, outputs, run_asan

SEEDS = (0, 17)  # round robin, one shuffled schedule


@pytest.fixture(scope="module")
def simt():
    return SimtTspHk()


def test_size_queries(simt):
    assert TC.LDS_MAX_N == 12 and TC.slot_bytes(13) == 196608 and TC.slot_bytes(14) == 425984
    for n in range(0, 17):
        assert simt.slot_bytes(n) == TC.slot_bytes(n), n
        for N in (0, 1, 5, 512, 513, 100000):
            assert simt.workspace_bytes(n, N) == TC.workspace_bytes(n, N), (n, N)
        if 3 <= n <= 14:
            assert simt.lds_bytes(n) == TC.lds_bytes(n) <= TC.MAX_LDS, n
    assert simt.workspace_bytes(13, -1) == TC.E_INVALID


def test_rejected_arguments(simt):
    for n in (2, 15):
        assert simt.solve(np.ones((1, TC.n_edges(n)), np.float32), n)[0] == TC.E_INVALID, n
    c = TC.host("gen", 4)[0]
    o = outputs(len(c), 4, F_EVAL)
    assert simt.solve(c, 4, into=o)[0] == TC.E_INVALID and (o["eval"] == 77.0).all()   # eval without eval_costs
    assert simt.solve(np.zeros((0, 6), np.float32), 4, flags=F_SOL)[0] == 0                          # N == 0
    assert simt.solve(np.zeros((0, TC.n_edges(13)), np.float32), 13, flags=F_SOL, workspace_bytes=0)[0] == 0
    for n in (TC.WS_MIN_N, 14):                                                         # the global tier needs one slot
        c = TC.host("ties", n)[0]
        o = outputs(len(c), n, F_ALL)
        for wsb in (0, 8, TC.slot_bytes(n) - 8):
            assert simt.solve(c, n, eval_costs=c, workspace_bytes=wsb, into=o)[0] == TC.E_INVALID, (n, wsb)
        assert simt.solve(c, n, eval_costs=c, workspace_bytes=TC.slot_bytes(n))[0] == 0   # one slot is enough
        assert all((a == (-7 if a.dtype == np.int32 else 77.0)).all() for a in o.values())
    assert simt.solve(TC.host("ties", 12)[0], 12, flags=F_SOL, workspace_bytes=0)[0] == 0           # the LDS tier needs none


@pytest.mark.parametrize("n", list(TC.SHAPES))
@pytest.mark.parametrize("kind", TC.KINDS)
def test_tours_objectives_and_evals_equal_the_host(simt, kind, n):
    costs, sols, objs, tours = TC.host(kind, n)
    ev = TC.costs_of("signed", len(costs), n, seed=3)
    first = None
    for seed in SEEDS:
        rc, o, grid = simt.solve(costs, n, eval_costs=ev, seed=seed)
        assert rc == 0 and grid == len(costs)
        TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=(kind, n, seed))
        if first is None:
            first = o
        else:  # the schedule does not show
            for k in o:
                assert np.array_equal(TC.bits(o[k]), TC.bits(first[k])), (kind, n, k)


@pytest.mark.parametrize("n", [TC.WS_MIN_N])
def test_two_slots_five_instances_and_a_batch_of_one(simt, n):
    """slot reuse and a tail: workgroup 0 takes instances 0, 2, 4 and workgroup 1 instances 1, 3; N = 1 in both tiers"""
    costs, sols, objs, tours = TC.host("ties", n, N=5, seed=1)
    rc, o, grid = simt.solve(costs, n, eval_costs=costs, workspace_bytes=2 * TC.slot_bytes(n), seed=5)
    assert rc == 0 and grid == 2
    TC.check_solve(o, sols, objs, tours, n, eval_costs=costs, what="two slots")
    rc, o1, grid = simt.solve(costs, n, eval_costs=costs, workspace_bytes=TC.slot_bytes(n) + 8)   # one slot and a remainder
    assert rc == 0 and grid == 1
    for k in o:
        assert np.array_equal(TC.bits(o[k]), TC.bits(o1[k])), k
    for m in (8, n):
        rc, o, grid = simt.solve(costs[:1, :TC.n_edges(m)], m, eval_costs=costs[:1, :TC.n_edges(m)], seed=9)
        s, z, t = TC.tight.tsp_solve(costs[0, :TC.n_edges(m)], m)
        assert rc == 0 and grid == 1
        TC.check_solve(o, s[None], np.asarray([z]), np.asarray([t], np.int32), m, eval_costs=costs[:1, :TC.n_edges(m)], what=("N=1", m))


@pytest.mark.parametrize("n", [8, TC.WS_MIN_N])
def test_a_non_finite_cost_fails_its_instance_alone(simt, n):
    bad, hit, ref = TC.bad_batch(n)
    for wsb in (None, 2 * TC.slot_bytes(n)) if TC.slot_bytes(n) else (None,):   # the bad instance's slot is reused
        rc, o, _ = simt.solve(bad, n, eval_costs=TC.host("gen", n, N=6, seed=3)[0], seed=7, workspace_bytes=wsb)
        assert rc == 0
        TC.check_bad(o, hit, ref, len(bad), what=(n, wsb))


@pytest.mark.parametrize("n", [4, TC.WS_MIN_N])
def test_every_null_output_combination_leaves_the_others_unchanged(simt, n):
    N = 3
    costs, sols, objs, tours = TC.host("ties", n, N=N, seed=2)
    ev = TC.costs_of("signed", N, n, seed=4)
    rc, full, _ = simt.solve(costs, n, eval_costs=ev)
    assert rc == 0
    TC.check_solve(full, sols, objs, tours, n, eval_costs=ev)
    each = (F_SOL, F_OBJ, F_EVAL, F_TOUR, F_STATUS)
    combos = list(itertools.product((0, 1), repeat=5)) if n == 4 else [(1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 0, 0, 0)]
    for keep in combos:
        flags = sum(f for f, k in zip(each, keep) if k)
        for with_ev in (True, False):
            if not with_ev and flags & F_EVAL:
                continue
            rc, o, _ = simt.solve(costs, n, eval_costs=ev if with_ev else None, flags=flags, seed=3)
            assert rc == 0, (keep, with_ev)
            for k, a in o.items():
                assert (a is None) == (not flags & dict(zip(("sol", "obj", "eval", "tour", "status"), each))[k])
                if a is not None:
                    assert np.array_equal(TC.bits(a), TC.bits(full[k])), (keep, with_ev, k)


def test_tsp_hk_kernels_are_asan_ubsan_clean(tmp_path):
    """a stand-alone sanitizer build of the emulation unit (its own main; no runtime preloaded): every input, every output,
    the LDS block and the workspace are heap blocks of their exact size.  One shuffled schedule; every shape of the
    table, both tiers, the two-slot workspace with its tail, a failed instance, absent outputs, the rejected calls."""
    cases, want = [], []
    for n, kind in ((3, "gen"), (4, "ties"), (7, "signed"), (8, "gen"), (TC.LDS_MAX_N, "ties"), (TC.WS_MIN_N, "gen"), (14, "ties")):
        costs, sols, objs, tours = TC.host(kind, n)
        cases.append((costs, n, costs, F_ALL, 11, TC.workspace_bytes(n, len(costs))))
        want.append((sols, objs, tours))
    n = TC.WS_MIN_N
    costs, sols, objs, tours = TC.host("ties", n, N=5, seed=1)
    cases.append((costs, n, None, F_SOL | F_OBJ | F_TOUR, 11, 2 * TC.slot_bytes(n)))
    want.append((sols, objs, tours))
    rejected = [(costs, n, None, F_SOL, 0, TC.slot_bytes(n) - 8), (costs, n, None, F_SOL, 0, 0), (costs[:, :1], 2, None, F_SOL, 0, 0)]
    res = run_asan(cases + rejected, str(tmp_path))
    assert [r[0] for r in res[len(cases):]] == [TC.E_INVALID] * 3
    for (costs, n, ev, flags, _, _), (sols, objs, tours), (rc, o) in zip(cases, want, res):
        assert rc == 0
        TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=("asan", n))
    for n in (8, TC.WS_MIN_N):   # a failed instance, in a reused slot too, and absent outputs
        bad, hit, ref = TC.bad_batch(n)
        (rc, o), (rc2, o2) = run_asan([(bad, n, bad, F_ALL, 3, 2 * TC.slot_bytes(n)), (bad, n, None, F_STATUS, 3, 2 * TC.slot_bytes(n))],
                                      str(tmp_path))
        assert rc == 0 and rc2 == 0
        TC.check_bad(o, hit, ref, len(bad), what=("asan", n))
        assert np.array_equal(o["status"], o2["status"])
