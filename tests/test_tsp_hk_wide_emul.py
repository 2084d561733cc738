"""CPU tier: the wide Held-Karp tier (cave_amd/csrc/tsp_hk_wide.h: the list kernel, then tsp_hk_wide_block, 512-thread
workgroups striding over the batch as k_tsp_hk_wide.hip launches them) under the SIMT emulation
(tests/emul/simt_tsp_hk_wide.cpp): round robin, one shuffled lane schedule, and once as a stand-alone program under
AddressSanitizer + UBSan with exact-size buffers, LDS blocks and workspace.

Oracles: tight.tsp_solve at n = 13; beyond it the numpy restatement of tests/tsp_hk_wide_cases.py, which is itself
asserted against tight.tsp_solve here; at n = 18 the committed fixture.  Everything is asserted EQUAL.
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest

import tsp_hk_cases as TC
import tsp_hk_wide_cases as WC
from emul_tsp_hk_wide_lib import F_ALL, F_EVAL, F_OBJ, F_SOL, F_STATUS, F_TOUR, SimtTspHkWide, outputs, run_asan

SEEDS = (0, 17)  # round robin, one shuffled schedule


@pytest.fixture(scope="module")
def simt():
    return SimtTspHkWide()


@pytest.mark.parametrize("n", [5, 9, 12, 13])
def test_the_restatement_equals_the_host_solver(n):
    for kind in TC.KINDS:
        costs, sols, objs, tours = TC.host(kind, n, N=3)
        for i in range(3):
            s, o, t = WC.solve_ref(costs[i], n)
            assert np.array_equal(s, sols[i]) and np.float64(o).tobytes() == objs[i].tobytes() and t == list(tours[i]), (kind, n, i)


def test_the_fixture_is_what_its_script_writes_and_agrees_with_the_cut_loop():
    for n in WC.GOLDEN_NS:
        costs, sols, objs, tours, dfj = WC.golden(n)
        assert np.array_equal(TC.bits(costs), TC.bits(WC.golden_costs(n))), n
        assert (sols.sum(1) == n).all() and (np.sort(tours, axis=1) == np.arange(n)).all() and (tours[:, 0] == 0).all()
        # a tour's length summed in another order, and another algorithm's optimum: fp64 sums of the same n positive
        # terms, n - 1 roundings of at most 2^-53 of the objective on either side
        assert abs(float(costs[0].astype(np.float64) @ sols[0]) - objs[0]) <= n * 2.0 ** -52 * abs(objs[0])
        assert abs(dfj - objs[0]) <= n * 2.0 ** -52 * abs(objs[0]), (n, dfj, objs[0])
        assert objs[1] == np.round(objs[1]) and n <= objs[1] <= 3 * n   # integer costs from {1, 2, 3}


def test_size_queries(simt):
    table = {13: 196608, 14: 425984, 15: 917504, 17: 4194304, 18: 8912896, 19: 18874368, 20: 39845888}
    slots = {18: 512, 19: 455, 20: 215}
    for n in range(0, 23):
        ok = 13 <= n <= 20
        assert simt.slot_bytes(n) == WC.slot_bytes(n) == (8 * (n - 1) * 2 ** (n - 2) if ok else -1), n
        if n in table:
            assert simt.slot_bytes(n) == table[n]
        if ok:
            assert WC.default_slots(n) == slots.get(n, 512), n
            assert simt.header_bytes(n) == WC.header_bytes(n) and simt.lds_bytes(n) == WC.lds_bytes(n) <= 16 * 1024, n
        for N in (0, 1, 5, 215, 216, 455, 456, 512, 513, 100000):
            want = WC.header_bytes(n) + WC.slot_bytes(n) * min(N, WC.default_slots(n)) if ok else -1
            assert simt.workspace_bytes(n, N) == WC.workspace_bytes(n, N) == want, (n, N)
        assert simt.workspace_bytes(n, -1) == TC.E_INVALID


def test_rejected_arguments(simt):
    for n in (12, 21):
        assert simt.solve(np.ones((1, TC.n_edges(n)), np.float32), n, workspace_bytes=1 << 20)[0] == TC.E_INVALID, n
    c = TC.host("gen", 13)[0]
    o = outputs(len(c), 13, F_EVAL)
    assert simt.solve(c, 13, into=o)[0] == TC.E_INVALID and (o["eval"] == 77.0).all()   # eval without eval_costs
    assert simt.solve(np.zeros((0, TC.n_edges(13)), np.float32), 13, flags=F_SOL, workspace_bytes=0)[0] == 0   # N == 0
    for n in (13, 15):   # the header region and one slot are needed
        c = TC.costs_of("ties", 2, n)
        o = outputs(len(c), n, F_ALL)
        for wsb in (0, 8, WC.slot_bytes(n) - 8, WC.slot_bytes(n), WC.header_bytes(n) + WC.slot_bytes(n) - 8):
            assert simt.solve(c, n, eval_costs=c, workspace_bytes=wsb, into=o)[0] == TC.E_INVALID, (n, wsb)
        assert all((a == (-7 if a.dtype == np.int32 else 77.0)).all() for a in o.values())
    c = TC.host("ties", 13)[0]
    assert simt.solve(c, 13, eval_costs=c, workspace_bytes=WC.header_bytes(13) + WC.slot_bytes(13))[0] == 0   # enough


def _both_schedules(simt, costs, n, ev, want, what, **kw):
    sols, objs, tours = want
    first = None
    for seed in SEEDS:
        rc, o, grid = simt.solve(costs, n, eval_costs=ev, seed=seed, **kw)
        assert rc == 0
        TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=(what, seed))
        if first is None:
            first = o
        else:  # the schedule does not show
            for k in o:
                assert np.array_equal(TC.bits(o[k]), TC.bits(first[k])), (what, k)
    return grid


@pytest.mark.parametrize("kind", TC.KINDS)
def test_n13_equals_the_host(simt, kind):
    costs, sols, objs, tours = TC.host(kind, 13, N=3)
    ev = TC.costs_of("signed", 3, 13, seed=3)
    assert _both_schedules(simt, costs, 13, ev, (sols, objs, tours), (kind, 13)) == 3


def test_n15_equals_the_restatement(simt):
    costs, sols, objs, tours = WC.ref("gen", 15, N=2)
    ev = TC.costs_of("signed", 2, 15, seed=3)
    assert _both_schedules(simt, costs, 15, ev, (sols, objs, tours), ("gen", 15)) == 2


@pytest.mark.parametrize("n", [17, 18])
def test_the_16_bit_boundaries(simt, n):
    """n = 17: class offsets over the m-bit sets reach 2^16; n = 18: T has 17 bits, offsets over m-1 bits reach 2^16"""
    if n == 18:
        costs, sols, objs, tours = (a[1:2] for a in WC.golden(18)[:4])   # the fixture's `ties` row
    else:
        costs, sols, objs, tours = WC.ref("ties", n, N=1)
    assert _both_schedules(simt, costs, n, costs, (sols, objs, tours), ("ties", n)) == 1


def test_two_slots_five_instances_and_one_slot_with_a_remainder(simt):
    """slot reuse and a tail: workgroup 0 takes instances 0, 2, 4 and workgroup 1 instances 1, 3"""
    n = 15
    costs, sols, objs, tours = WC.ref("ties", n, N=5, seed=1)
    rc, o, grid = simt.solve(costs, n, eval_costs=costs, workspace_bytes=WC.header_bytes(n) + 2 * WC.slot_bytes(n), seed=5)
    assert rc == 0 and grid == 2
    TC.check_solve(o, sols, objs, tours, n, eval_costs=costs, what="two slots")
    rc, o1, grid = simt.solve(costs, n, eval_costs=costs, workspace_bytes=WC.header_bytes(n) + WC.slot_bytes(n) + 8)
    assert rc == 0 and grid == 1
    for k in o:
        assert np.array_equal(TC.bits(o[k]), TC.bits(o1[k])), k


def test_a_non_finite_cost_fails_its_instance_alone(simt):
    n = 13
    bad, hit, ref = WC.bad_batch(n)
    ev = TC.host("gen", n, N=6, seed=3)[0]
    for wsb in (None, WC.header_bytes(n) + 2 * WC.slot_bytes(n)):   # the bad instance's slot is reused
        rc, o, _ = simt.solve(bad, n, eval_costs=ev, seed=7, workspace_bytes=wsb)
        assert rc == 0
        TC.check_bad(o, hit, ref, len(bad), what=(n, wsb))


def test_null_output_combinations_leave_the_others_unchanged(simt):
    n, N = 13, 3
    costs, sols, objs, tours = TC.host("ties", n, N=N, seed=2)
    ev = TC.costs_of("signed", N, n, seed=4)
    rc, full, _ = simt.solve(costs, n, eval_costs=ev)
    assert rc == 0
    TC.check_solve(full, sols, objs, tours, n, eval_costs=ev)
    each = (F_SOL, F_OBJ, F_EVAL, F_TOUR, F_STATUS)
    for keep in [(1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 0, 0, 0)]:
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


def test_tsp_hk_wide_kernels_are_asan_ubsan_clean(tmp_path):
    """a stand-alone sanitizer build of the emulation unit (its own main; no runtime preloaded): every input, every output,
    the LDS blocks and the workspace (header region + slots) are heap blocks of their exact size.  One shuffled schedule;
    n = 13 and 15, the two-slot workspace with its tail, a failed instance in a reused slot, absent outputs, the rejected
    calls."""
    c13, s13, o13, t13 = TC.host("gen", 13, N=3)
    c15, s15, o15, t15 = WC.ref("gen", 15, N=2)
    t5, ts5, to5, tt5 = WC.ref("ties", 15, N=5, seed=1)
    cases = [(c13, 13, c13, F_ALL, 11, WC.workspace_bytes(13, 3)), (c15, 15, c15, F_ALL, 11, WC.workspace_bytes(15, 2)),
             (t5, 15, None, F_SOL | F_OBJ | F_TOUR, 11, WC.header_bytes(15) + 2 * WC.slot_bytes(15))]
    want = [(s13, o13, t13), (s15, o15, t15), (ts5, to5, tt5)]
    rejected = [(c13, 13, None, F_SOL, 0, WC.header_bytes(13) + WC.slot_bytes(13) - 8), (c13, 13, None, F_SOL, 0, 0),
                (c13[:, :66], 12, None, F_SOL, 0, 1 << 20)]
    bad, hit, ref = WC.bad_batch(13)
    two = WC.header_bytes(13) + 2 * WC.slot_bytes(13)
    res = run_asan(cases + rejected + [(bad, 13, bad, F_ALL, 3, two), (bad, 13, None, F_STATUS, 3, two)], str(tmp_path))
    assert [r[0] for r in res[3:6]] == [TC.E_INVALID] * 3
    for (costs, n, ev, _, _, _), (sols, objs, tours), (rc, o) in zip(cases, want, res):
        assert rc == 0
        TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=("asan", n))
    (rc, o), (rc2, o2) = res[6:]
    assert rc == 0 and rc2 == 0
    TC.check_bad(o, hit, ref, len(bad), what="asan")
    assert np.array_equal(o["status"], o2["status"])
