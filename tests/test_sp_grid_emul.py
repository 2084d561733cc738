"""CPU tier: the grid shortest-path kernel (cave_amd/csrc/sp_grid.h sp_grid_instance, one 64-lane wave per instance, the
workgroups of k_sp_grid.hip) under the SIMT emulation (tests/emul/simt_sp_grid.cpp): round robin, one shuffled lane
schedule, and once as a stand-alone program under AddressSanitizer + UBSan with exact-size buffers and LDS block.

Oracle: tight.sp_solve, tight.sp_tight_normals and SparseCones.from_ragged; cases and bounds: tests/sp_grid_cases.py.
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest

import sp_grid_cases as SC
from cave_amd import tight
from cave_amd.sparse import SparseCones
from emul_sp_grid_lib import F_ALL, F_CONES, F_EVAL, F_OBJ, F_SOL, F_STATUS, SimtSpGrid, run_asan

SEEDS = (0, 17)  # round robin, one shuffled schedule


@pytest.fixture(scope="module")
def simt():
    return SimtSpGrid()


def test_lds_query_and_rejected_shapes(simt):
    for (h, w) in list(SC.SHAPES) + [(1, 1), (128, 128), (134, 134), (135, 135), (1, 70000), (0, 5), (5, -1)]:
        assert simt.lds_bytes(h, w) == SC.lds_bytes(h, w), (h, w)
    at, above = SC.lds_limit_shapes()
    assert 0 < simt.lds_bytes(*at) <= SC.MAX_LDS and simt.lds_bytes(*above) == SC.E_INVALID
    one = np.ones((1, 1), np.float32)
    assert simt.solve(np.ones((1, 0), np.float32), 1, 1)[0] == SC.E_INVALID
    assert simt.solve(np.ones((1, SC.n_arcs(*above)), np.float32), *above, flags=F_SOL)[0] == SC.E_INVALID
    assert simt.solve(one, 1, 2, flags=F_EVAL)[0] == SC.E_INVALID          # eval without eval_costs
    assert simt.solve(np.zeros((0, 1), np.float32), 1, 2, flags=F_SOL)[0] == 0   # N == 0
    # cone output: rows and columns are 16-bit
    d = SC.n_arcs(128, 129)
    assert 2 * 128 * 129 + d > 65535 >= 2 * 128 * 128 + SC.n_arcs(128, 128)
    c = np.ones((1, d), np.float32)
    assert simt.solve(c, 128, 129, flags=F_CONES)[0] == SC.E_INVALID
    assert simt.solve(c, 128, 129, flags=F_SOL)[0] == 0


@pytest.mark.parametrize("shape", list(SC.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", SC.KINDS)
def test_solve_eval_and_cones_equal_the_host(simt, kind, shape):
    h, w = shape
    costs, sols, objs = SC.host(kind, h, w)
    ev = SC.costs_of("signed", len(costs), h, w, seed=3)
    ref = SC.host_cones(kind, h, w)
    first = None
    for seed in SEEDS:
        rc, o, waves = simt.solve(costs, h, w, eval_costs=ev, seed=seed)
        assert rc == 0 and waves == 4
        SC.check_solve(o, costs, sols, objs, h, w, eval_costs=ev, what=(kind, shape, seed))
        SC.check_cones(o["key"], o["val"], ref, len(costs), h, w, what=(kind, shape, seed))
        if first is None:
            first = o
        else:  # condition 7: the schedule does not show
            for k in o:
                assert np.array_equal(o[k].view(np.uint8), first[k].view(np.uint8)), (kind, shape, k)


def test_cone_coo_builder_is_from_ragged():
    """the dense-free oracle of the 128x128 case, against the dense one"""
    for (h, w) in ((1, 2), (2, 2), (1, 7), (7, 1), (5, 5), (3, 70)):
        sols = SC.host("gen", h, w)[1][:3]
        a = SparseCones.from_coo([SC.cone_coo(s, h, w) for s in sols], SC.n_arcs(h, w))
        b = SparseCones.from_ragged([tight.sp_tight_normals(s, h, w) for s in sols])
        assert a.m_max == b.m_max and all(np.array_equal(getattr(a, k).numpy(), getattr(b, k).numpy()) for k in ("ent_off", "key", "val"))


def test_limit_shapes(simt):
    """the shape at the LDS limit (one wave per workgroup, three strips; solve only: beyond the key's 16 bits) and the
    largest square grid whose cone fits the key (128x128, two strips)"""
    (h, w), _ = SC.lds_limit_shapes()
    costs, sols, objs = SC.host("ties", h, w, N=2)
    rc, o, waves = simt.solve(costs, h, w, eval_costs=costs, flags=F_ALL & ~F_CONES, seed=5)
    assert rc == 0 and waves == 1
    SC.check_solve(o, costs, sols, objs, h, w, eval_costs=costs, what="lds limit")
    assert simt.solve(costs, h, w, flags=F_ALL)[0] == SC.E_INVALID
    h = w = 128
    costs, sols, objs = SC.host("gen", h, w, N=1)
    rc, o, waves = simt.solve(costs, h, w, eval_costs=None, flags=F_ALL & ~F_EVAL)
    assert rc == 0 and waves == 1
    SC.check_solve(o, costs, sols, objs, h, w, what="cone limit")
    ref = SparseCones.from_coo([SC.cone_coo(sols[0], h, w)], SC.n_arcs(h, w))
    SC.check_cones(o["key"], o["val"], ref, 1, h, w, what="cone limit")
    assert ref.m_max == 65280


def test_batch_variants(simt):
    h, w = 5, 5
    d = SC.n_arcs(h, w)
    # a batch of one; a batch of 1000 (250 workgroups)
    for N in (1, 1000):
        costs, sols, objs = SC.host("gen", h, w, N=N)
        rc, o, _ = simt.solve(costs, h, w, eval_costs=costs, flags=F_ALL & ~F_CONES, seed=N)
        assert rc == 0
        SC.check_solve(o, costs, sols, objs, h, w, eval_costs=costs, what=N)
        assert np.abs(o["eval"] - objs).max() <= SC.eval_bound(costs, sols, h, w).max()  # priced under its own costs: the objective
    # each output pointer null in turn; eval_costs present and absent
    costs, sols, objs = SC.host("ties", h, w)
    ref = SC.host_cones("ties", h, w)
    for drop in (F_SOL, F_OBJ, F_EVAL, F_STATUS, F_CONES):
        for ev in (costs, None):
            flags = F_ALL & ~drop & ~(0 if ev is not None else F_EVAL)
            rc, o, _ = simt.solve(costs, h, w, eval_costs=ev, flags=flags, seed=3)
            assert rc == 0
            SC.check_solve(o, costs, sols, objs, h, w, eval_costs=ev, what=(drop, ev is None))
            if o["key"] is not None:
                SC.check_cones(o["key"], o["val"], ref, len(costs), h, w)


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("shape", [(5, 5), (3, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_non_finite_cost_fails_its_instance_alone(simt, shape, poison):
    h, w = shape
    costs, sols, objs = SC.host("gen", h, w)
    d = SC.n_arcs(h, w)
    bad = costs.copy()
    hit = (0, 9, len(costs) - 1)
    for n, b in enumerate(hit):
        bad[b, (d - 1, 0, d // 2)[n]] = poison
    rc, o, _ = simt.solve(bad, h, w, eval_costs=costs, seed=7)
    assert rc == 0
    ok = np.ones(len(costs), bool)
    ok[list(hit)] = False
    assert (o["status"][~ok] == SC.ST_BAD_INPUT).all() and (o["status"][ok] == SC.ST_OK).all()
    assert (o["sol"][~ok] == 0).all() and np.isnan(o["obj"][~ok]).all() and np.isnan(o["eval"][~ok]).all()
    assert np.array_equal(o["sol"][ok], sols[ok]) and np.array_equal(o["obj"][ok], objs[ok])
    # the cones: the neighbours' are the host's, a failed instance gets the cone of the zero vector (all arcs at 0)
    ref = SC.host_cones("gen", h, w)
    zero = SparseCones.from_ragged([tight.sp_tight_normals(np.zeros(d, np.float32), h, w)])
    key, val = o["key"].reshape(len(costs), 5 * d), o["val"].reshape(len(costs), 5 * d)
    rk, rv = ref.key.numpy().reshape(len(costs), 5 * d), ref.val.numpy().reshape(len(costs), 5 * d)
    assert np.array_equal(key[ok], rk[ok]) and np.array_equal(val[ok], rv[ok])
    for b in hit:
        assert np.array_equal(key[b], zero.key.numpy()) and np.array_equal(val[b], zero.val.numpy())


def test_sp_grid_kernel_is_asan_ubsan_clean(tmp_path):
    """a stand-alone sanitizer build of the emulation unit (its own main; no runtime preloaded): every input, every
    output and the LDS block are heap blocks of their exact size.  One shuffled schedule; the wave-width edges, several
    strips, the LDS limit, a failed instance, absent outputs."""
    cases, want = [], []
    for (h, w), kind, N in (((1, 2), "gen", 5), ((7, 1), "signed", 3), ((5, 5), "ties", 9), ((2, 65), "gen", 6), ((65, 2), "spread", 5),
                            ((3, 70), "ties", 7), ((70, 3), "gen", 4), ((30, 30), "gen", 5)):
        costs, sols, objs = SC.host(kind, h, w)
        cases.append((costs[:N], h, w, costs[:N], F_ALL, 11))
        want.append((sols[:N], objs[:N]))
    (lh, lw), above = SC.lds_limit_shapes()
    costs, sols, objs = SC.host("ties", lh, lw, N=2)
    cases.append((costs, lh, lw, None, F_SOL | F_OBJ | F_STATUS, 11))
    want.append((sols, objs))
    res = run_asan(cases + [(np.ones((1, SC.n_arcs(*above)), np.float32), *above, None, F_SOL, 0)], str(tmp_path))
    assert res[-1][0] == SC.E_INVALID
    for (costs, h, w, ev, flags, _), (sols, objs), (rc, o) in zip(cases, want, res):
        assert rc == 0
        SC.check_solve(o, costs, sols, objs, h, w, eval_costs=ev, what=("asan", h, w))
        if o["key"] is not None:
            ref = SparseCones.from_ragged(tight.sp_tight_normals(s, h, w) for s in sols)
            SC.check_cones(o["key"], o["val"], ref, len(costs), h, w, what=("asan", h, w))
    # a failed instance and absent outputs under the sanitizers
    costs = SC.host("gen", 5, 5)[0][:6].copy()
    costs[2, 3] = np.nan
    (rc, o), (rc2, o2) = run_asan([(costs, 5, 5, costs, F_ALL, 3), (costs, 5, 5, None, F_CONES, 3)], str(tmp_path))
    assert rc == 0 and rc2 == 0 and o["status"][2] == SC.ST_BAD_INPUT and (np.delete(o["status"], 2) == 0).all()
    assert np.array_equal(o["key"], o2["key"]) and np.array_equal(o["val"], o2["val"])
