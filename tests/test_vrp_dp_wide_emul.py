"""CPU tier: the wide CVRP tier (cave_amd/csrc/vrp_dp_wide.h: the list kernel, then vrp_dp_wide_block<M>, 512-thread
workgroups striding over the batch as k_vrp_dp_wide.hip launches them, behind vrp_dp_wide_plan) under the SIMT emulation
(tests/emul/simt_vrp_dp_wide.cpp): round robin, one shuffled lane schedule, and once as a stand-alone program under
AddressSanitizer + UBSan with exact-size buffers, LDS blocks and workspace.

Oracles: tight.vrp_solve up to n = 14 and the first tier's emulation there, the numpy restatement beyond; cases and
bounds: tests/vrp_dp_wide_cases.py.  TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest

import vrp_dp_cases as VC
import vrp_dp_wide_cases as WC
from emul_vrp_dp_lib import SimtVrpDp
from emul_vrp_dp_wide_lib import F_ALL, F_EVAL, F_OBJ, F_ROUTES, F_SOL, F_STATUS, NAMES, SimtVrpDpWide, outputs, run_asan, untouched

SEEDS = (0, 17)  # round robin, one shuffled schedule
EACH = (F_SOL, F_OBJ, F_EVAL, F_ROUTES, F_STATUS)
EMUL_SHAPES = [(n, K) for n in (13, 14, 15) for K in (1, 2, 3)]


@pytest.fixture(scope="module")
def simt():
    return SimtVrpDpWide()


@pytest.fixture(scope="module")
def first_tier():
    return SimtVrpDp()


@pytest.mark.parametrize("shape", [(5, 2), (6, 3), (9, 3), (10, 3), (11, 4), (12, 3), (12, 6)], ids=lambda s: f"n{s[0]}-K{s[1]}")
def test_the_restatement_equals_the_host_solver(shape):
    n, K = shape
    for kind in WC.KINDS:
        costs, q, cap, sols, objs, routes = VC.host(kind, n, K, N=2)
        for i in range(2):
            s, o, r = WC.solve_ref(costs[i], n, q, cap, K)
            assert np.array_equal(s, sols[i]) and np.float64(o).tobytes() == objs[i].tobytes(), (kind, n, K, i)
            assert np.array_equal(VC.pad_routes(r, n, K), routes[i]), (kind, n, K, i)


def test_the_restatement_raises_where_the_host_does():
    for costs, q, cap, K, want in VC.infeasible_calls(8):
        if want is None:
            for c in costs:
                with pytest.raises(ValueError):
                    WC.solve_ref(c, 8, q, cap, K)


def test_the_fixture_is_of_the_instances_and_agrees_with_the_cut_loop():
    for n, K in WC.GOLDEN_SHAPES:
        costs, q, caps, sols, objs, routes = WC.golden(n, K)   # (asserts that the rows are golden_instances(n, K))
        assert np.isfinite(objs).all()
        for i, kind in enumerate(WC.KINDS):
            WC.check_instance(kind, q[i], caps[i], n)
            r = routes[i][routes[i] >= 0]
            k = int((r == 0).sum()) - 1
            assert 1 <= k <= K and sols[i].sum() == n - 1 + k and sorted(r[r > 0]) == list(range(1, n)), (n, K, kind)
            # every route of at least two customers and within the capacity: loads summed as the model sums them
            cut = np.flatnonzero(r == 0)
            for a, b in zip(cut, cut[1:]):
                assert b - a - 1 >= 2 and sum(np.float64(q[i][v - 1]) for v in sorted(r[a + 1:b])) <= caps[i], (n, K, kind)
            # the routes' cost summed in another order: the same n - 1 + k terms, that many roundings on either side
            bound = (n + K) * 2.0 ** -52 * float(np.abs(costs[i].astype(np.float64)) @ sols[i])
            assert abs(float(costs[i].astype(np.float64) @ sols[i]) - objs[i]) <= bound, (n, K, kind)
        assert objs[1] == np.round(objs[1])   # integer costs from {1, 2, 3}
    n, K = WC.GOLDEN_RCC
    z = WC.golden(n, K)[4][0]
    assert (n, K) == WC.GOLDEN_SHAPES[-1] and abs(WC.golden_rcc() - z) <= (n + K) * 2.0 ** -52 * abs(z), (WC.golden_rcc(), z)


def test_size_queries(simt):
    assert WC.slot_bytes(13, 3) == 196608 + 2 * 32768 and WC.slot_bytes(20, 2) == 39845888 + 4194304
    assert WC.slot_bytes(20, 8) == 39845888 + 7 * 4194304 and WC.slot_bytes(15, 1) == 917504
    assert WC.default_slots(20, 2) == 195 and WC.default_slots(20, 8) == 124 and WC.default_slots(18, 8) == 512
    for n in range(0, 23):
        for K in range(0, 10):
            assert simt.slot_bytes(n, K) == WC.slot_bytes(n, K), (n, K)
            for N in (0, 1, 5, 124, 125, 195, 196, 512, 513, 100000):
                assert simt.workspace_bytes(n, K, N) == WC.workspace_bytes(n, K, N), (n, K, N)
            assert simt.workspace_bytes(n, K, -1) == WC.E_INVALID
            if WC.valid(n, K):
                assert simt.header_bytes(n, K) == WC.header_bytes(n) and simt.lds_bytes(n, K) == WC.lds_bytes(n) <= 24 * 1024, (n, K)


def test_rejected_arguments_leave_the_outputs_untouched(simt):
    n, K = 13, 3
    c, q, cap = WC.ref("gen", n, K)[:3]
    enough = WC.workspace_bytes(n, K, len(c))
    for nn, kk in ((12, 3), (21, 3), (13, 0), (13, 9)):
        assert simt.solve(np.ones((1, VC.n_edges(nn)), np.float32), nn, np.ones(nn - 1), 1e3, kk, flags=F_SOL, workspace_bytes=1 << 20)[0] == WC.E_INVALID
    o = outputs(len(c), n, K, F_ALL)
    assert simt.solve(c, n, q, cap, K, into=outputs(len(c), n, K, F_EVAL), workspace_bytes=enough)[0] == WC.E_INVALID   # eval without eval_costs
    for bad_cap in (0.0, -1.0, np.inf, np.nan):
        assert simt.solve(c, n, q, bad_cap, K, eval_costs=c, into=o, workspace_bytes=enough)[0] == WC.E_INVALID, bad_cap
    assert simt.solve(c, n, None, cap, K, eval_costs=c, into=o, workspace_bytes=enough)[0] == WC.E_INVALID                 # null demands
    assert simt.solve(c, n, q, cap, K, eval_costs=c, into=o, workspace_bytes=enough, null_costs=True)[0] == WC.E_INVALID   # null costs
    for wsb in (0, 8, WC.slot_bytes(n, K), WC.header_bytes(n) + WC.slot_bytes(n, K) - 8):   # the header region and one slot are needed
        assert simt.solve(c, n, q, cap, K, eval_costs=c, workspace_bytes=wsb, into=o)[0] == WC.E_INVALID, wsb
    assert untouched(o)
    assert simt.solve(np.zeros((0, VC.n_edges(n)), np.float32), n, q, cap, K, flags=F_SOL, workspace_bytes=0)[0] == 0   # N == 0
    assert simt.solve(c, n, q, cap, K, eval_costs=c, workspace_bytes=WC.header_bytes(n) + WC.slot_bytes(n, K))[0] == 0   # enough


@pytest.mark.parametrize("shape", EMUL_SHAPES, ids=lambda s: f"n{s[0]}-K{s[1]}")
@pytest.mark.parametrize("kind", WC.KINDS)
def test_routes_objectives_and_evals_equal_the_oracle_and_the_first_tier(simt, first_tier, kind, shape):
    n, K = shape
    costs, q, cap, sols, objs, routes = WC.ref(kind, n, K, N=2)
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
    if n <= 14:  # the same bytes as the first entry's kernels
        rc, o1, _ = first_tier.solve(costs, n, q, cap, K, eval_costs=ev)
        assert rc == 0
        for k in first:
            assert np.array_equal(VC.bits(first[k]), VC.bits(o1[k])), (kind, n, K, k)


def test_the_lower_edge_with_every_layer_stored_equals_the_first_tier(simt, first_tier):
    """n = 13 at K = 6: K' = 6, four stored layers behind r (the first entry's tier 2)"""
    n, K = 13, 6
    costs, q, cap, sols, objs, routes = WC.ref("signed", n, K, N=2)
    rc, o, _ = simt.solve(costs, n, q, cap, K, eval_costs=costs, seed=5)
    assert rc == 0
    VC.check_solve(o, sols, objs, routes, n, eval_costs=costs, what=(n, K))
    rc, o1, _ = first_tier.solve(costs, n, q, cap, K, eval_costs=costs)
    assert rc == 0 and all(np.array_equal(VC.bits(o[k]), VC.bits(o1[k])) for k in o)


def test_the_cases_use_several_route_counts():
    """the cases are not degenerate: a single route and the full fleet both occur among the optima with K' >= 2"""
    used = set()
    for n, K in EMUL_SHAPES:
        for kind in WC.KINDS:
            for r in WC.ref(kind, n, K, N=2)[5]:
                used.add((K, int((r == 0).sum()) - 1))
    assert any(K >= 2 and k == K for K, k in used) and any(K >= 2 and k < K for K, k in used)


def test_two_slots_five_instances_and_one_slot_with_a_remainder(simt):
    """slot reuse and a tail: workgroup 0 takes instances 0, 2, 4 and workgroup 1 instances 1, 3"""
    n, K = 15, 3
    costs, q, cap, sols, objs, routes = WC.ref("ties", n, K, N=5, seed=1)
    two = WC.header_bytes(n) + 2 * WC.slot_bytes(n, K)
    rc, o, grid = simt.solve(costs, n, q, cap, K, eval_costs=costs, workspace_bytes=two, seed=5)
    assert rc == 0 and grid == 2
    VC.check_solve(o, sols, objs, routes, n, eval_costs=costs, what="two slots")
    rc, o1, grid = simt.solve(costs, n, q, cap, K, eval_costs=costs, workspace_bytes=WC.header_bytes(n) + WC.slot_bytes(n, K) + 8)
    assert rc == 0 and grid == 1
    for k in o:
        assert np.array_equal(VC.bits(o[k]), VC.bits(o1[k])), k


def test_failed_instances(simt):
    """a non-finite cost fails its instance alone (its slot is reused); a negative or non-finite demand fails them all"""
    n, K = 13, 3
    bad, hit, case = WC.bad_batch(n, K)
    q, cap = case[1], case[2]
    for wsb in (None, WC.header_bytes(n) + 2 * WC.slot_bytes(n, K)):
        rc, o, _ = simt.solve(bad, n, q, cap, K, eval_costs=case[0], seed=7, workspace_bytes=wsb)
        assert rc == 0
        VC.check_bad(o, hit, case, what=(n, K, wsb))
    for v in (-1.0, np.nan, np.inf):
        qb = q.copy()
        qb[n - 2] = v
        rc, o, _ = simt.solve(case[0][:2], n, qb, cap, K, eval_costs=case[0][:2], seed=7)
        assert rc == 0
        VC.check_failed(o, VC.ST_BAD_INPUT, what=(n, K, v))


def test_infeasible_instances(simt):
    n = 15
    for costs, q, cap, K, want in WC.infeasible_calls(n):
        rc, o, _ = simt.solve(costs, n, q, cap, K, eval_costs=costs, seed=11)
        assert rc == 0
        if want is None:
            VC.check_failed(o, VC.ST_INFEASIBLE, what=(cap, K))
        else:
            VC.check_solve(o, *want, n, eval_costs=costs, what=(cap, K))


def test_null_output_combinations_leave_the_others_unchanged(simt):
    n, K, N = 13, 3, 3
    costs, q, cap, sols, objs, routes = WC.ref("ties", n, K, N=N, seed=2)
    ev = VC.instance_of("signed", N, n, K, seed=4)[0]
    rc, full, _ = simt.solve(costs, n, q, cap, K, eval_costs=ev)
    assert rc == 0
    VC.check_solve(full, sols, objs, routes, n, eval_costs=ev)
    for keep in [(1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 0, 0, 0)]:
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


def test_vrp_dp_wide_kernels_are_asan_ubsan_clean(tmp_path):
    """a stand-alone sanitizer build of the emulation unit (its own main; no runtime preloaded): every input, every output,
    the LDS blocks and the workspace (header region + slots) are heap blocks of their exact size.  One shuffled schedule;
    n = 13 and 15 at K = 1, 3 (and 13 at K = 6), the two-slot workspace with its tail, a failed instance in a reused slot,
    an infeasible call, absent outputs, the rejected calls."""
    cases, want = [], []
    for kind, (n, K) in zip(("gen", "ties", "signed", "gen", "signed"), ((13, 3), (15, 3), (13, 1), (15, 1), (13, 6))):
        costs, q, cap, sols, objs, routes = WC.ref(kind, n, K, N=2)
        cases.append((costs, n, q, cap, K, costs, F_ALL, 11, WC.workspace_bytes(n, K, 2)))
        want.append((sols, objs, routes))
    n, K = 15, 3
    costs, q, cap, sols, objs, routes = WC.ref("ties", n, K, N=5, seed=1)
    two = WC.header_bytes(n) + 2 * WC.slot_bytes(n, K)
    cases.append((costs, n, q, cap, K, None, F_SOL | F_OBJ | F_ROUTES, 11, two))
    want.append((sols, objs, routes))
    rejected = [(costs, n, q, cap, K, None, F_SOL, 0, two - WC.slot_bytes(n, K) - 8), (costs, n, q, cap, K, None, F_SOL, 0, 0),
                (costs[:, :66], 12, q[:11], cap, K, None, F_SOL, 0, 1 << 20), (costs, n, q, 0.0, K, None, F_SOL, 0, two),
                (costs, n, q, cap, 9, None, F_SOL, 0, two), (costs, n, q, cap, K, None, F_SOL | 64, 0, two)]
    bad, hit, case = WC.bad_batch(13, 3)
    two13 = WC.header_bytes(13) + 2 * WC.slot_bytes(13, 3)
    failed = [(bad, 13, case[1], case[2], 3, bad, F_ALL, 3, two13), (bad, 13, case[1], case[2], 3, None, F_STATUS, 3, two13)]
    c, q2, cap2, K2, _ = WC.infeasible_calls(15)[1]
    res = run_asan(cases + rejected + failed + [(c, 15, q2, cap2, K2, c, F_ALL, 5, WC.workspace_bytes(15, K2, 1))], str(tmp_path))
    a, b = len(cases), len(cases) + len(rejected)
    assert [r[0] for r in res[a:b]] == [WC.E_INVALID] * len(rejected)
    for (costs, n, q, cap, K, ev, _, _, _), (sols, objs, routes), (rc, o) in zip(cases, want, res):
        assert rc == 0
        VC.check_solve(o, sols, objs, routes, n, eval_costs=ev, what=("asan", n, K))
    (rc, o), (rc2, o2), (rc3, o3) = res[b:]
    assert rc == 0 and rc2 == 0 and rc3 == 0
    VC.check_bad(o, hit, case, what="asan")
    assert np.array_equal(o["status"], o2["status"])
    VC.check_failed(o3, VC.ST_INFEASIBLE, what="asan")
