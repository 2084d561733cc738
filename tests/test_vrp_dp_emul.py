"""CPU tier: the CVRP dynamic-program kernels (cave_amd/csrc/vrp_dp.h vrp_dp_block, 256-thread workgroups striding over
the batch as k_vrp_dp.hip launches them, all tiers) under the SIMT emulation (tests/emul/simt_vrp_dp.cpp): round robin,
one shuffled lane schedule, and once as a stand-alone program under AddressSanitizer + UBSan with exact-size buffers,
LDS block and workspace.

Oracle: tight.vrp_solve; cases and bounds: tests/vrp_dp_cases.py.  TEST INFRASTRUCTURE: nothing in cave_amd loads these
builds."""

import itertools

import numpy as np
import pytest

import vrp_dp_cases as VC
from emul_vrp_dp_lib import F_ALL, F_EVAL, F_OBJ, F_ROUTES, F_SOL, F_STATUS, NAMES, SimtVrpDp, outputs, run_asan, untouched

SEEDS = (0, 17)  # round robin, one shuffled schedule
EACH = (F_SOL, F_OBJ, F_EVAL, F_ROUTES, F_STATUS)


@pytest.fixture(scope="module")
def simt():
    return SimtVrpDp()


def test_size_queries(simt):
    assert VC.LDS_MAX_N == 12 and VC.tier(12, 3) == 0 and VC.tier(13, 3) == 1 and VC.tier(14, 2) == 1 and VC.tier(13, 6) == 2
    assert VC.slot_bytes(13, 3) == 196608 and VC.slot_bytes(14, 2) == 425984 and VC.slot_bytes(13, 6) == 196608 + 5 * 32768
    for n in range(0, 17):
        for K in range(0, 10):
            assert simt.slot_bytes(n, K) == VC.slot_bytes(n, K), (n, K)
            for N in (0, 1, 5, 512, 513, 100000):
                assert simt.workspace_bytes(n, K, N) == VC.workspace_bytes(n, K, N), (n, K, N)
            if VC.valid(n, K):
                assert simt.tier(n, K) == VC.tier(n, K) and simt.lds_bytes(n, K) == VC.lds_bytes(n, K) <= VC.MAX_LDS, (n, K)
    assert simt.workspace_bytes(13, 3, -1) == VC.E_INVALID


def test_rejected_arguments_leave_the_outputs_untouched(simt):
    c, q, cap = VC.host("gen", 5, 2)[:3]
    o = outputs(len(c), 5, 2, F_ALL)
    for n, K in ((2, 1), (15, 1), (5, 0), (5, 9)):
        assert simt.solve(np.ones((1, VC.n_edges(n)), np.float32), n, np.ones(max(n - 1, 1)), 10.0, K, flags=F_SOL)[0] == VC.E_INVALID
    assert simt.solve(c, 5, q, cap, 2, into=outputs(len(c), 5, 2, F_EVAL))[0] == VC.E_INVALID      # eval without eval_costs
    for bad_cap in (0.0, -1.0, np.inf, np.nan):
        assert simt.solve(c, 5, q, bad_cap, 2, eval_costs=c, into=o)[0] == VC.E_INVALID, bad_cap
    assert simt.solve(c, 5, None, cap, 2, eval_costs=c, into=o)[0] == VC.E_INVALID                 # null demands
    assert simt.solve(c, 5, q, cap, 2, eval_costs=c, into=o, null_costs=True)[0] == VC.E_INVALID   # null costs
    assert untouched(o)
    assert simt.solve(np.zeros((0, 10), np.float32), 5, q, cap, 2, flags=F_SOL)[0] == 0             # N == 0
    assert simt.solve(np.zeros((0, VC.n_edges(13)), np.float32), 13, np.ones(12), 9.0, 3, flags=F_SOL, workspace_bytes=0)[0] == 0
    for n, K in ((VC.WS_MIN_N, 3), (13, 6)):                                          # a slot is needed
        c, q, cap = VC.host("ties", n, K)[:3]
        o = outputs(len(c), n, K, F_ALL)
        for wsb in (0, 8, VC.slot_bytes(n, K) - 8):
            assert simt.solve(c, n, q, cap, K, eval_costs=c, workspace_bytes=wsb, into=o)[0] == VC.E_INVALID, (n, K, wsb)
        assert untouched(o)
    c, q, cap = VC.host("ties", VC.LDS_MAX_N, 3)[:3]
    assert simt.solve(c, VC.LDS_MAX_N, q, cap, 3, flags=F_SOL, workspace_bytes=0)[0] == 0          # tier 0 needs none


@pytest.mark.parametrize("shape", list(VC.SHAPES), ids=lambda s: f"n{s[0]}-K{s[1]}")
@pytest.mark.parametrize("kind", VC.KINDS)
def test_routes_objectives_and_evals_equal_the_host(simt, kind, shape):
    n, K = shape
    costs, q, cap, sols, objs, routes = VC.host(kind, n, K)
    ev = VC.instance_of("signed", len(costs), n, K, seed=3)[0]
    first = None
    for seed in SEEDS:
        rc, o, grid = simt.solve(costs, n, q, cap, K, eval_costs=ev, seed=seed)
        assert rc == 0 and grid == len(costs)
        VC.check_solve(o, sols, objs, routes, n, eval_costs=ev, what=(kind, n, K, seed))
        if first is None:
            first = o
        else:  # the schedule does not show
            for k in o:
                assert np.array_equal(VC.bits(o[k]), VC.bits(first[k])), (kind, n, K, k)


def test_the_cases_use_every_route_count_and_bind_the_fleet():
    """the cases are not degenerate: over the shapes with K' >= 2 both a single route and the full fleet occur, and in
    the signed kind the optimum takes all K' routes somewhere (K binds)"""
    seen = set()
    for (n, K), _ in VC.SHAPES.items():
        for kind in VC.KINDS:
            routes = VC.host(kind, n, K)[5]
            for r in routes:
                seen.add((kind, VC.kmax(n, K), int((r == 0).sum()) - 1))
    assert any(k == "signed" and km >= 2 and used == km for k, km, used in seen)
    assert any(km >= 2 and used < km for _, km, used in seen) and any(km >= 3 and used >= 2 for _, km, used in seen)


def test_one_vehicle_and_a_loose_capacity_is_held_karp(simt):
    n = 8
    costs = VC.instance_of("ties", 4, n, 1)[0]
    ref = [VC.tight.tsp_solve(c, n) for c in costs]
    rc, o, _ = simt.solve(costs, n, np.ones(n - 1), 1e30, 1, eval_costs=costs, seed=3)
    assert rc == 0
    assert np.array_equal(o["sol"], np.stack([s for s, _, _ in ref])) and np.array_equal(VC.bits(o["obj"]), VC.bits(np.asarray([z for _, z, _ in ref])))
    assert np.array_equal(o["routes"][:, :n], np.asarray([t for _, _, t in ref], np.int32)) and (o["routes"][:, n] == 0).all()


@pytest.mark.parametrize("shape", [(VC.WS_MIN_N, 3), (13, 6)], ids=["tier1", "tier2"])
def test_two_slots_five_instances_and_a_batch_of_one(simt, shape):
    """slot reuse and a tail: workgroup 0 takes instances 0, 2, 4 and workgroup 1 instances 1, 3; N = 1"""
    n, K = shape
    costs, q, cap, sols, objs, routes = VC.host("ties", n, K, N=5, seed=1)
    rc, o, grid = simt.solve(costs, n, q, cap, K, eval_costs=costs, workspace_bytes=2 * VC.slot_bytes(n, K), seed=5)
    assert rc == 0 and grid == 2
    VC.check_solve(o, sols, objs, routes, n, eval_costs=costs, what="two slots")
    rc, o1, grid = simt.solve(costs, n, q, cap, K, eval_costs=costs, workspace_bytes=VC.slot_bytes(n, K) + 8)   # one slot and a remainder
    assert rc == 0 and grid == 1
    for k in o:
        assert np.array_equal(VC.bits(o[k]), VC.bits(o1[k])), k
    rc, o, grid = simt.solve(costs[:1], n, q, cap, K, eval_costs=costs[:1], seed=9)
    assert rc == 0 and grid == 1
    VC.check_solve(o, sols[:1], objs[:1], routes[:1], n, eval_costs=costs[:1], what="N=1")


def test_a_batch_of_one_in_lds(simt):
    costs, q, cap, sols, objs, routes = VC.host("gen", 8, 3)
    rc, o, grid = simt.solve(costs[:1], 8, q, cap, 3, eval_costs=costs[:1], seed=9)
    assert rc == 0 and grid == 1
    VC.check_solve(o, sols[:1], objs[:1], routes[:1], 8, eval_costs=costs[:1], what="N=1")


@pytest.mark.parametrize("shape", [(8, 3), (VC.WS_MIN_N, 3)], ids=["lds", "slot"])
def test_failed_instances(simt, shape):
    """a non-finite cost fails its instance alone (its slot is reused); a negative or non-finite demand fails them all"""
    n, K = shape
    bad, hit, case = VC.bad_batch(n, K)
    q, cap = case[1], case[2]
    for wsb in (None, 2 * VC.slot_bytes(n, K)) if VC.slot_bytes(n, K) else (None,):
        rc, o, _ = simt.solve(bad, n, q, cap, K, eval_costs=case[0], seed=7, workspace_bytes=wsb)
        assert rc == 0
        VC.check_bad(o, hit, case, what=(n, K, wsb))
    for v in (-1.0, np.nan, np.inf):
        qb = q.copy()
        qb[n - 2] = v
        rc, o, _ = simt.solve(case[0], n, qb, cap, K, eval_costs=case[0], seed=7)
        assert rc == 0
        VC.check_failed(o, VC.ST_BAD_INPUT, what=(n, K, v))


def test_infeasible_instances(simt):
    n = 8
    for costs, q, cap, K, want in VC.infeasible_calls(n):
        rc, o, _ = simt.solve(costs, n, q, cap, K, eval_costs=costs, seed=11)
        assert rc == 0
        if want is None:
            VC.check_failed(o, VC.ST_INFEASIBLE, what=(cap, K))
        else:
            VC.check_solve(o, *want, n, eval_costs=costs, what=(cap, K))


@pytest.mark.parametrize("shape", [(5, 2), (VC.WS_MIN_N, 3)], ids=["lds", "slot"])
def test_every_null_output_combination_leaves_the_others_unchanged(simt, shape):
    n, K = shape
    N = 3
    costs, q, cap, sols, objs, routes = VC.host("ties", n, K, N=N, seed=2)
    ev = VC.instance_of("signed", N, n, K, seed=4)[0]
    rc, full, _ = simt.solve(costs, n, q, cap, K, eval_costs=ev)
    assert rc == 0
    VC.check_solve(full, sols, objs, routes, n, eval_costs=ev)
    combos = list(itertools.product((0, 1), repeat=5)) if n == 5 else [(1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 0, 0, 0)]
    for keep in combos:
        flags = sum(f for f, k in zip(EACH, keep) if k)
        for with_ev in (True, False):
            if not with_ev and flags & F_EVAL:
                continue
            rc, o, _ = simt.solve(costs, n, q, cap, K, eval_costs=ev if with_ev else None, flags=flags, seed=3)
            assert rc == 0, (keep, with_ev)
            for k, a in o.items():
                assert (a is None) == (not flags & dict(zip(NAMES, EACH))[k])
                if a is not None:
                    assert np.array_equal(VC.bits(a), VC.bits(full[k])), (keep, with_ev, k)


def test_vrp_dp_kernels_are_asan_ubsan_clean(tmp_path):
    """a stand-alone sanitizer build of the emulation unit (its own main; no runtime preloaded): every input, every output,
    the LDS block and the workspace are heap blocks of their exact size.  One shuffled schedule; every shape, all tiers,
    the two-slot workspace with its tail, failed and infeasible instances, absent outputs, the rejected calls."""
    cases, want = [], []
    kinds = itertools.cycle(VC.KINDS)
    for (n, K) in VC.SHAPES:
        costs, q, cap, sols, objs, routes = VC.host(next(kinds), n, K)
        cases.append((costs, n, q, cap, K, costs, F_ALL, 11, VC.workspace_bytes(n, K, len(costs))))
        want.append((sols, objs, routes))
    n, K = VC.WS_MIN_N, 3
    costs, q, cap, sols, objs, routes = VC.host("ties", n, K, N=5, seed=1)
    cases.append((costs, n, q, cap, K, None, F_SOL | F_OBJ | F_ROUTES, 11, 2 * VC.slot_bytes(n, K)))
    want.append((sols, objs, routes))
    rejected = [(costs, n, q, cap, K, None, F_SOL, 0, VC.slot_bytes(n, K) - 8), (costs, n, q, cap, K, None, F_SOL, 0, 0),
                (costs[:, :1], 2, q[:1], cap, K, None, F_SOL, 0, 0), (costs, n, q, 0.0, K, None, F_SOL, 0, 2 * VC.slot_bytes(n, K)),
                (costs, n, q, cap, 9, None, F_SOL, 0, 2 * VC.slot_bytes(n, K)), (costs, n, q, cap, K, None, F_SOL | 64, 0, 2 * VC.slot_bytes(n, K))]
    res = run_asan(cases + rejected, str(tmp_path))
    assert [r[0] for r in res[len(cases):]] == [VC.E_INVALID] * len(rejected)
    for (costs, n, q, cap, K, ev, flags, _, _), (sols, objs, routes), (rc, o) in zip(cases, want, res):
        assert rc == 0
        VC.check_solve(o, sols, objs, routes, n, eval_costs=ev, what=("asan", n, K))
    for n, K in ((8, 3), (VC.WS_MIN_N, 3)):   # a failed instance, in a reused slot too, and absent outputs
        bad, hit, case = VC.bad_batch(n, K)
        q, cap = case[1], case[2]
        (rc, o), (rc2, o2) = run_asan([(bad, n, q, cap, K, bad, F_ALL, 3, 2 * VC.slot_bytes(n, K)),
                                       (bad, n, q, cap, K, None, F_STATUS, 3, 2 * VC.slot_bytes(n, K))], str(tmp_path))
        assert rc == 0 and rc2 == 0
        VC.check_bad(o, hit, case, what=("asan", n, K))
        assert np.array_equal(o["status"], o2["status"])
    calls = VC.infeasible_calls(8)
    res = run_asan([(c, 8, q, cap, K, c, F_ALL, 5, 0) for c, q, cap, K, _ in calls], str(tmp_path))
    for (c, q, cap, K, expect), (rc, o) in zip(calls, res):
        assert rc == 0
        if expect is None:
            VC.check_failed(o, VC.ST_INFEASIBLE, what=("asan", cap, K))
        else:
            VC.check_solve(o, *expect, 8, eval_costs=c, what=("asan", cap, K))
