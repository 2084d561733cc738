"""CPU tier: the tight-cone kernels (cave_amd/csrc/tight_cones.h: tight_cones_count_instance, tight_cones_fill_instance, one
64-lane wave per instance, the workgroups of k_tight_cones.hip) under the SIMT emulation (tests/emul/simt_tight_cones.cpp)
behind the shared plan function: round robin, one shuffled lane schedule, and once as a stand-alone program under
AddressSanitizer + UBSan with exact-size buffers.  And, host only, the Python layer in front of them (cave_amd/tight.py:
LinSystem, tsp_system, vrp_system, sp_system, cut_rows).

Oracle: sp_tight_normals, tsp_tight_normals, vrp_tight_normals, tests/tight_ref.py, each through SparseCones.from_ragged;
cases: tests/tight_cones_cases.py.  TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest
import scipy.sparse as sp

import tight_cones_cases as TC
from cave_amd import tight
from cave_amd.synth import sp_arcs, tsp_edges
from emul_tight_cones_lib import SimtTightCones, run_asan

SEEDS = (0, 17)  # round robin, one shuffled schedule


@pytest.fixture(scope="module")
def simt():
    return SimtTightCones()


# ------------------------------------------------------------------ the cases themselves (host only)

def test_the_cases_hold_what_they_are_there_for():
    _, _, sols, cuts = TC.tsp_data(8)
    assert sum(1 for k in cuts if k) == 7 and len(cuts[7]) == 2  # 7 of the 12 instances carry a cut, instance 7 two
    c7 = TC.tsp_case(8)
    lz = TC.dense(c7.lazy)[c7.lazy_off[7]:c7.lazy_off[8]]
    assert sorted(np.abs(c7.lazy.rhs[c7.lazy_off[7]:c7.lazy_off[8]] - lz @ sols[7].astype(np.float64)) < 1e-5) == [False, True]
    _, _, _, _, vs, vcuts = TC.vrp_data()
    assert len(vcuts[3]) == 4 and all(s[:TC.VRP_N - 1].sum() == 2 * TC.VRP_K for s in vs)  # the depot row is tight in all eight
    sys, lazy, off, sol = TC.synth_parts()
    assert sys.R == 70 and sys.d == 67 and set(sys.sense) == {0, 1, 2} and off[3] == off[2] and off[4] - off[3] > 64
    tight_at = np.abs(sys.rhs[None, :] - sol.astype(np.float64) @ TC.dense(sys).T) < 1e-5
    assert not tight_at[4].any() and all(tight_at[b].sum() >= 10 for b in range(4))
    for b in range(4):  # every sense occurs among each instance's tight rows
        assert set(sys.sense[tight_at[b]]) == {0, 1, 2}
    assert TC.synth_case().rows[4] == 0 and (np.diff(TC.long_row_case().sys.row_off) == [130, 0, 3]).all()


@pytest.mark.parametrize("case", [TC.sp_case(3, 3), TC.sp_case(5, 5), TC.tsp_case(8), TC.tsp_case(6), TC.vrp_case()], ids=lambda c: c.name)
def test_the_model_functions_and_the_restatement_agree(case):
    """sp_/tsp_/vrp_tight_normals (through the case's expectation) against tests/tight_ref.py on the LinSystem forms"""
    mats = TC.ref_matrices(case.sys, case.lazy, case.lazy_off, case.sol, case.tol)
    e = TC.SparseCones.from_ragged(mats)
    assert e.m_max == case.expect.m_max
    for k in ("ent_off", "key", "val"):
        assert np.array_equal(getattr(e, k).numpy(), getattr(case.expect, k).numpy()), (case.name, k)


# ------------------------------------------------------------------ the kernels

@pytest.mark.parametrize("case", TC.good_cases(), ids=lambda c: c.name)
def test_cones_equal_the_host(simt, case):
    first = None
    for seed in SEEDS:
        rc, o = simt.run(case, seed=seed)
        TC.check(case, rc, o, seed)
        if first is None:
            first = o
        else:  # the schedule does not show
            for k in o:
                assert np.array_equal(o[k].view(np.uint8), first[k].view(np.uint8)), (case.name, k)


@pytest.mark.parametrize("case", TC.bad_cases(), ids=lambda c: c.name)
def test_a_failed_instance_counts_nothing_and_writes_nothing(simt, case):
    rc, o = simt.run(case, seed=5)
    TC.check(case, rc, o)
    assert (o["n_rows"][:len(case.sol)][case.status != 0] == 0).all() and (o["n_ent"][:len(case.sol)][case.status != 0] == 0).all()


def test_the_fill_pass_refuses_a_window_that_is_not_the_counted_one(simt):
    case = TC.synth_case()
    N = len(case.sol)
    want = case.expect.ent_off.numpy()
    off = want.copy()
    off[2:] += 1  # instance 1 gets one entry too many, the others keep their sizes
    cap = int(off[-1])
    key, val, st = np.full(cap + 8, -7, np.int32), np.full(cap + 8, 77.0, np.float32), np.full(N, -7, np.int32)
    assert simt.fill(case.sys, case.lazy, case.lazy_off, case.sol, N, case.tol, off, cap, key, val, st, seed=3) == 0
    assert list(st) == [0, TC.ST_BAD_INPUT, 0, 0, 0]
    assert (key[off[1]:off[2]] == -7).all() and (key[cap:] == -7).all() and (val[cap:] == 77.0).all()
    for b in (0, 2, 3):
        assert np.array_equal(key[off[b]:off[b + 1]], case.expect.key.numpy()[want[b]:want[b + 1]])
    # a window beyond ent_cap: refused as well, nothing written
    key[:] = -7
    assert simt.fill(case.sys, case.lazy, case.lazy_off, case.sol, N, case.tol, want, int(want[3]), key, val, st, seed=3) == 0
    # (instance 4 is empty, but its window lies beyond ent_cap as well)
    assert list(st) == [0, 0, 0, TC.ST_BAD_INPUT, TC.ST_BAD_INPUT] and (key[want[3]:] == -7).all()


def test_invalid_arguments_are_refused_before_any_launch(simt):
    case = TC.d1_case()
    s, sol, N = case.sys, case.sol, len(case.sol)
    n_rows, n_ent, st = np.full(N, -7, np.int32), np.full(N, -7, np.int64), np.full(N, -7, np.int32)

    def count(sys=s, lazy=None, lazy_off=None, sol=sol, N=N, tol=1e-5, n_rows=n_rows, n_ent=n_ent, st=st):
        return simt.count(sys, lazy, lazy_off, sol, N, tol, n_rows, n_ent, st)

    assert count() == 0
    n_rows[:], n_ent[:], st[:] = -7, -7, -7
    odd = np.zeros(4 * N + 4, np.uint8)[1:1 + 4 * N].view(np.float32)  # misaligned
    lz = TC.tsp_case(6).lazy
    for kw in (dict(sol=None), dict(sol=odd), dict(n_rows=None), dict(n_ent=None), dict(sys=s._replace(d=0)), dict(sys=s._replace(d=65536)),
               dict(sys=s._replace(R=-1)), dict(sys=s._replace(Z=-1)), dict(N=-1), dict(tol=-1e-9), dict(tol=np.nan), dict(tol=np.inf),
               dict(sys=s._replace(row_off=None)), dict(sys=s._replace(col=None)), dict(sys=s._replace(coef=None)),
               dict(sys=s._replace(sense=None)), dict(sys=s._replace(rhs=None)),
               dict(lazy=s, lazy_off=None),               # lazy rows without lazy_off
               dict(lazy=lz, lazy_off=np.zeros(N + 1, np.int64))):  # lazy rows over another d
        assert count(**kw) == TC.E_INVALID, kw
    assert (n_rows == -7).all() and (n_ent == -7).all() and (st == -7).all()
    assert simt.count(None, None, None, sol, N, 1e-5, n_rows, n_ent, st) == TC.E_INVALID
    # N == 0: nothing to do, whatever the arrays; status may be absent; d = 65535 is in range
    assert count(N=0, sol=None, n_rows=None, n_ent=None, st=None) == 0
    assert count(st=None) == 0 and (n_rows >= 0).all()
    wide = TC.RawSys(0, 0, 65535, None, None, None, None, None)
    assert simt.count(wide, None, None, np.full((1, 65535), 0.5, np.float32), 1, 1e-5, n_rows, n_ent, st) == 0 and n_rows[0] == 0
    # the fill pass
    off, key, val = np.zeros(N + 1, np.int64), np.zeros(8, np.int32), np.zeros(8, np.float32)
    assert simt.fill(s, None, None, sol, N, 1e-5, None, 8, key, val, st) == TC.E_INVALID
    assert simt.fill(s, None, None, sol, N, 1e-5, off, -1, key, val, st) == TC.E_INVALID
    assert simt.fill(s, None, None, sol, N, 1e-5, off, 8, None, val, st) == TC.E_INVALID
    assert simt.fill(s, None, None, sol, N, 1e-5, off, 8, key, None, st) == TC.E_INVALID
    assert simt.fill(s, None, None, sol, 0, 1e-5, None, 0, None, None, None) == 0


def test_tight_cone_kernels_are_asan_ubsan_clean(tmp_path):
    """a stand-alone sanitizer build of the emulation unit (its own main; no runtime preloaded): every input and every
    output is a heap block of its exact size, key / val exactly the counted entries.  One shuffled schedule, every case."""
    cases = TC.good_cases() + TC.bad_cases()
    res = run_asan([(c, int(c.expect.ent_off[-1])) for c in cases], str(tmp_path))
    for c, (rc, o) in zip(cases, res):
        o["ent_off"] = np.r_[0, np.cumsum(o["n_ent"])].astype(np.int64)
        pad = {k: np.r_[o[k], np.full(TC.GUARD, TC.FILL_I, o[k].dtype)] for k in ("n_rows", "n_ent", "status", "fill_status")}
        TC.check(c, rc, dict(o, **pad), "asan")


# ------------------------------------------------------------------ the Python layer (host only)

def test_lin_system_canonicalises():
    A = np.array([[0, 2, 0, -1], [0, 0, 0, 0], [1e-60, 1, 0, 0]])
    a = tight.LinSystem(A, ["<", ">", "="], [1, 2, 3])
    assert (a.R, a.d, a.nnz) == (3, 4, 3) and a.row_off.tolist() == [0, 2, 2, 3] and a.col.tolist() == [1, 3, 1]
    assert a.coef.tolist() == [2.0, -1.0, 1.0] and a.sense.tolist() == [0, 1, 2] and a.rhs.tolist() == [1.0, 2.0, 3.0]
    assert [t.dtype for t in (a.row_off, a.col, a.coef, a.sense, a.rhs)] == [np.int64, np.int32, np.float32, np.int8, np.float64]
    # a scipy matrix with unsorted columns, a repeated entry and an explicit zero; one sense and one rhs for all rows
    M = sp.coo_matrix(([1.0, 2.0, 3.0, 0.0, 4.0], ([0, 0, 0, 1, 1], [3, 1, 3, 0, 2])), shape=(2, 4))
    b = tight.LinSystem(M, "=", 2.0)
    assert b.row_off.tolist() == [0, 2, 3] and b.col.tolist() == [1, 3, 2] and b.coef.tolist() == [2.0, 4.0, 4.0]
    assert b.sense.tolist() == [2, 2] and b.rhs.tolist() == [2.0, 2.0]
    assert np.array_equal(b.dense(), np.array([[0, 2, 0, 4], [0, 0, 4, 0]], np.float32))
    for same in (M.tocsr(), M.tocsc(), M.toarray()):
        c = tight.LinSystem(same, ["E", b"="], np.array([2, 2]))
        assert all(np.array_equal(getattr(b, k), getattr(c, k)) for k in ("row_off", "col", "coef", "sense", "rhs"))
    assert tight.LinSystem(np.zeros((0, 3)), [], []).R == 0


def test_lin_system_errors():
    A = np.eye(2)
    with pytest.raises(ValueError, match="Invalid constraint sense"):
        tight.LinSystem(A, ["<", "!"], [0, 0])
    with pytest.raises(ValueError, match="senses"):
        tight.LinSystem(A, ["<"], [0, 0])
    with pytest.raises(ValueError, match="right-hand sides"):
        tight.LinSystem(A, "<", [0, 0, 0])
    with pytest.raises(ValueError, match="not finite"):
        tight.LinSystem(A, "<", [0, np.inf])
    with pytest.raises(ValueError, match="not finite"):
        tight.LinSystem(np.array([[np.nan, 1.0]]), "<", 0)
    with pytest.raises(ValueError, match="columns"):
        tight.LinSystem(sp.csr_matrix((1, 65536)), "<", 0)
    with pytest.raises(ValueError, match="columns"):
        tight.LinSystem(np.zeros((2, 0)), "<", 0)
    with pytest.raises(ValueError, match="dense"):
        tight.LinSystem(np.zeros(3), "<", 0)


def test_the_model_systems_are_the_matrices_the_host_functions_build():
    for n in (3, 6, 8):
        edges = tsp_edges(n)
        d = len(edges)
        deg = np.zeros((n, d), np.float32)
        deg[edges[:, 0], np.arange(d)] = 1.0
        deg[edges[:, 1], np.arange(d)] = 1.0
        t = tight.tsp_system(n)
        assert np.array_equal(t.dense(), deg) and (t.sense == 2).all() and (t.rhs == 2).all()
        v = tight.vrp_system(n, 3)
        assert np.array_equal(v.dense(), deg) and v.sense.tolist() == [0] + [2] * (n - 1) and v.rhs.tolist() == [6.0] + [2.0] * (n - 1)
    for h, w in ((1, 2), (3, 3), (2, 5)):
        arcs = sp_arcs(h, w)
        d = len(arcs)
        Nm = np.zeros((h * w, d), np.float32)
        Nm[arcs[:, 1], np.arange(d)] = 1.0
        Nm[arcs[:, 0], np.arange(d)] = -1.0
        s = tight.sp_system(h, w)
        assert np.array_equal(s.dense(), Nm) and (s.sense == 2).all()
        path = tight.sp_solve(np.ones(d, np.float32), h, w)[0]
        assert np.array_equal(Nm.astype(np.float64) @ path, s.rhs)  # a path satisfies the rows


def test_cut_rows_are_the_dense_cut_rows():
    n = 7
    eid = tight._edge_index(n)[1]
    d = n * (n - 1) // 2
    per = [[[1, 2, 3], [4, 6, 5, 0]], [], [([2, 5], 0.0), ([1, 3, 4, 6], 2.0)]]
    lazy, off = tight.cut_rows(n, per)
    assert off.tolist() == [0, 2, 2, 4] and lazy.d == d and (lazy.sense == 0).all() and lazy.rhs.tolist() == [2.0, 3.0, 0.0, 2.0]
    want = np.stack([tight._cut_row(sorted(c[0] if isinstance(c, tuple) else c), eid, d) for cuts in per for c in cuts])
    assert np.array_equal(lazy.dense(), want.astype(np.float32))
    empty, off0 = tight.cut_rows(n, [[], []])
    assert empty.R == 0 and off0.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        tight.cut_rows(n, [[[1, 7]]])
