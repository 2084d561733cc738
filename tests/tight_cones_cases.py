"""Cases of the tight-cone kernels (cave_amd/csrc/tight_cones.h), shared by the CPU tier (tests/test_tight_cones_emul.py:
the kernels under the SIMT emulation) and the GPU tier (tests/test_gpu_tight_cones.py).

Every expected value comes from host code: `sp_tight_normals`, `tsp_tight_normals`, `vrp_tight_normals` for the three
models, the numpy restatement of the reference's rule (tests/tight_ref.py) for the rest, each through
`SparseCones.from_ragged`.  No expected value comes from the kernels.  All comparisons are exact: every value used is a
small dyadic number, so that the fp64 row sums are the same in every order of the additions.
"""

from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import tight_ref
from cave_amd import tight
from cave_amd.sparse import SparseCones

E_INVALID = -1
ST_OK, ST_TOO_LARGE, ST_BAD_INPUT = 0, 2, 3
GUARD = 8  # sentinel elements behind every output
FILL_I, FILL_F = -7, 77.0

# a cave_lin_system as numpy arrays (which may break the contract on purpose)
RawSys = namedtuple("RawSys", "R Z d row_off col coef sense rhs")
# sys / lazy: RawSys (lazy or lazy_off may be None); sol (N, d) float32; rows: expected n_rows (N,); expect: the
# SparseCones of the batch (a failed instance holds no entries); status: expected (N,)
Case = namedtuple("Case", "name sys lazy lazy_off sol tol rows expect status")


def raw(ls) -> RawSys:
    """the arrays of a cave_amd.tight.LinSystem"""
    return RawSys(ls.R, ls.nnz, ls.d, ls.row_off.copy(), ls.col.copy(), ls.coef.copy(), ls.sense.copy(), ls.rhs.copy())


def dense(s: RawSys) -> np.ndarray:
    a = np.zeros((s.R, s.d))
    a[np.repeat(np.arange(s.R), np.diff(s.row_off)), s.col] = s.coef
    return a


def ref_matrices(sys: RawSys, lazy, lazy_off, sol, tol):
    """tests/tight_ref.py per instance -> a list of (m_i, d) float32 matrices"""
    A = dense(sys)
    L = dense(lazy) if lazy is not None else None
    out = []
    for b, x in enumerate(sol):
        rows = []
        if lazy is not None and lazy_off is not None:
            rows = [(L[i], int(lazy.sense[i]), lazy.rhs[i]) for i in range(int(lazy_off[b]), int(lazy_off[b + 1]))]
        out.append(tight_ref.tight_normals(A, sys.sense, sys.rhs, rows, x, tol))
    return out


def make(name, sys, lazy, lazy_off, sol, tol, mats, status=None) -> Case:
    """`mats`: the expected matrix per instance; an instance with a status other than OK expects nothing"""
    sol = np.ascontiguousarray(sol, dtype=np.float32)
    status = np.zeros(len(sol), np.int32) if status is None else np.asarray(status, np.int32)
    mats = [m if st == ST_OK else np.zeros((0, sys.d), np.float32) for m, st in zip(mats, status)]
    return Case(name, sys, lazy, None if lazy_off is None else np.ascontiguousarray(lazy_off, dtype=np.int64), sol, float(tol),
                np.array([len(m) for m in mats], np.int32), SparseCones.from_ragged(mats), status)


# ------------------------------------------------------------------ the three models

@functools.lru_cache(maxsize=None)
def sp_case(h: int, w: int, N: int = 4) -> Case:
    costs = tight.sp_gen_data(N, 5, h, w, seed=135)[1]
    sols = np.stack([tight.sp_solve(c, h, w)[0] for c in costs])
    return make(f"sp{h}x{w}", raw(tight.sp_system(h, w)), None, None, sols, 1e-5, [tight.sp_tight_normals(s, h, w) for s in sols])


@functools.lru_cache(maxsize=None)
def tsp_data(n: int, N: int = 12):
    """-> (feats, costs, sols, cuts per instance) of tsp_gen_data(N, 5, n, seed=42) under tsp_dfj_cuts"""
    feats, costs = tight.tsp_gen_data(N, 5, n, seed=42)
    res = [tight.tsp_dfj_cuts(c, n) for c in costs]
    return feats, costs, np.stack([r[0] for r in res]), [r[2] for r in res]


@functools.lru_cache(maxsize=None)
def tsp_case(n: int) -> Case:
    _, _, sols, cuts = tsp_data(n)
    lazy, off = tight.cut_rows(n, cuts)
    return make(f"tsp{n}", raw(tight.tsp_system(n)), raw(lazy), off, sols, 1e-5,
                [tight.tsp_tight_normals(s, n, k) for s, k in zip(sols, cuts)])


VRP_N, VRP_K = 7, 2


@functools.lru_cache(maxsize=None)
def vrp_data():
    """-> (feats, costs, demands, capacity, sols, cuts per instance) of vrp_gen_data(8, 5, 7, seed=42), K = 2"""
    feats, costs, demands = tight.vrp_gen_data(8, 5, VRP_N, seed=42)
    capacity = float(np.ceil(1.3 * float(demands.sum()) / 2 + 5))
    sols = np.stack([tight.vrp_solve(c, VRP_N, demands, capacity, VRP_K)[0] for c in costs])
    cuts = [tight.vrp_rcc_cuts(c, VRP_N, demands, capacity, VRP_K)[2] for c in costs]
    return feats, costs, demands, capacity, sols, cuts


@functools.lru_cache(maxsize=None)
def vrp_case() -> Case:
    _, _, _, _, sols, cuts = vrp_data()
    lazy, off = tight.cut_rows(VRP_N, cuts)
    return make("vrp7", raw(tight.vrp_system(VRP_N, VRP_K)), raw(lazy), off, sols, 1e-5,
                [tight.vrp_tight_normals(s, VRP_N, k, VRP_K) for s, k in zip(sols, cuts)])


# ------------------------------------------------------------------ a synthetic system: all three senses, interleaved

_VALS = np.array([1.0, -1.0, 2.0, -2.0, 0.5])
_SOLV = np.array([0.0, 1.0, 0.0, 1.0, 0.5, 0.25])


def _rows(rng, R, d, lo=1, hi=6):
    """R random rows over d columns -> (row_off, col, coef)"""
    off, col, coef = [0], [], []
    for _ in range(R):
        k = int(rng.randint(lo, hi + 1))
        c = np.sort(rng.choice(d, size=min(k, d), replace=False))
        col.append(c)
        coef.append(_VALS[rng.randint(0, len(_VALS), size=len(c))])
        off.append(off[-1] + len(c))
    return np.asarray(off, np.int64), np.concatenate(col).astype(np.int32), np.concatenate(coef).astype(np.float32)


def _dots(off, col, coef, x):
    return np.array([float(coef[off[r]:off[r + 1]].astype(np.float64) @ x[col[off[r]:off[r + 1]]].astype(np.float64))
                     for r in range(len(off) - 1)])


@functools.lru_cache(maxsize=None)
def synth_parts(R: int = 70, d: int = 67):
    """-> (sys, lazy, lazy_off, sol): R rows (a ballot chunk is crossed), d columns (the bound rows cross a chunk), sense of
    row r = r % 3; row r is tight at instance r % 4 unless r % 5 == 0; no row is tight at instance 4.  Lazy rows: instance 0
    `<=` tight, `<=` slack, `>=` tight, `==` tight (the adjacent row, -row pair); instance 1 one `==` tight; instance 2
    none; instance 3 seventy (a chunk is crossed), every third slack; instance 4 two, both slack."""
    rng = np.random.RandomState(7)
    sol = _SOLV[rng.randint(0, len(_SOLV), size=(5, d))].astype(np.float32)
    sol[4] = 0.375  # strictly inside the box
    off, col, coef = _rows(rng, R, d)
    rhs = np.array([_dots(off[r:r + 2] - off[r], col[off[r]:off[r + 1]], coef[off[r]:off[r + 1]], sol[r % 4])[0] + (r % 5 == 0)
                    for r in range(R)])
    rhs[np.abs(rhs - _dots(off, col, coef, sol[4])) < 0.01] += 16.0  # nothing tight at the interior instance
    sys = RawSys(R, int(off[-1]), d, off, col, coef, (np.arange(R) % 3).astype(np.int8), rhs)
    per = [[(0, 0.0), (0, 1.0), (1, 0.0), (2, 0.0)], [(2, 0.0)], [], [(i % 3, float(i % 3 == 2)) for i in range(70)], [(0, 16.0), (2, 16.0)]]
    L = sum(len(p) for p in per)
    loff, lcol, lcoef = _rows(rng, L, d, 1, 8)
    lrhs, lsense, lazy_off, i = [], [], [0], 0
    for b, p in enumerate(per):
        for s, slack in p:
            lrhs.append(_dots(loff[i:i + 2] - loff[i], lcol[loff[i]:loff[i + 1]], lcoef[loff[i]:loff[i + 1]], sol[b])[0] + slack)
            lsense.append(s)
            i += 1
        lazy_off.append(i)
    lazy = RawSys(L, int(loff[-1]), d, loff, lcol, lcoef, np.asarray(lsense, np.int8), np.asarray(lrhs))
    return sys, lazy, np.asarray(lazy_off, np.int64), sol


def synth_case() -> Case:
    sys, lazy, off, sol = synth_parts()
    return make("synth", sys, lazy, off, sol, 1e-5, ref_matrices(sys, lazy, off, sol, 1e-5))


def single_case() -> Case:
    """N = 1: instance 0 of the synthetic batch"""
    sys, lazy, off, sol = synth_parts()
    return make("single", sys, lazy, off[:2], sol[:1], 1e-5, ref_matrices(sys, lazy, off[:2], sol[:1], 1e-5))


def long_row_case() -> Case:
    """d = 200: a row of 130 entries (the wave strides over it), an empty `==` row that is tight (two row numbers, no
    entry) and a short row; a long lazy `==` row"""
    d = 200
    rng = np.random.RandomState(3)
    sol = (rng.rand(3, d) < 0.5).astype(np.float32)
    sol[2, ::7] = 0.5
    c0 = np.sort(rng.choice(d, 130, replace=False)).astype(np.int32)
    c2 = np.array([3, 77, 199], np.int32)
    off = np.array([0, 130, 130, 133], np.int64)
    col, coef = np.r_[c0, c2].astype(np.int32), np.r_[_VALS[rng.randint(0, 4, 130)], [1.0, 2.0, -1.0]].astype(np.float32)
    rhs = np.array([_dots(off[:2], col, coef, sol[0])[0], 0.0, _dots(np.array([0, 3]), c2, coef[130:], sol[1])[0]])
    sys = RawSys(3, 133, d, off, col, coef, np.array([1, 2, 0], np.int8), rhs)
    lc = np.sort(rng.choice(d, 90, replace=False)).astype(np.int32)
    lv = _VALS[rng.randint(0, 4, 90)].astype(np.float32)
    lazy = RawSys(1, 90, d, np.array([0, 90], np.int64), lc, lv, np.array([2], np.int8), np.array([_dots(np.array([0, 90]), lc, lv, sol[2])[0]]))
    loff = np.array([0, 0, 0, 1], np.int64)
    return make("long_row", sys, lazy, loff, sol, 1e-5, ref_matrices(sys, lazy, loff, sol, 1e-5))


@functools.lru_cache(maxsize=None)
def many_long_parts():
    """d = 200: seven long rows (33 ... 200 entries: the kernel takes four at a time, sixteen lanes each, so two rounds and
    every group of lanes) around a short one, all senses; six long lazy rows for instance 0, one for instance 2"""
    d = 200
    rng = np.random.RandomState(11)
    sol = _SOLV[rng.randint(0, len(_SOLV), size=(3, d))].astype(np.float32)
    lens = [33, 40, 3, 64, 65, 100, 129, 200]
    off, col, coef = [0], [], []
    for n in lens:
        col.append(np.sort(rng.choice(d, n, replace=False)))
        coef.append(_VALS[rng.randint(0, len(_VALS), n)])
        off.append(off[-1] + n)
    off, col, coef = np.asarray(off, np.int64), np.concatenate(col).astype(np.int32), np.concatenate(coef).astype(np.float32)
    R = len(lens)
    rhs = np.array([_dots(off[r:r + 2] - off[r], col[off[r]:off[r + 1]], coef[off[r]:off[r + 1]], sol[r % 2])[0] + (r == 4) for r in range(R)])
    sys = RawSys(R, int(off[-1]), d, off, col, coef, (np.arange(R) % 3).astype(np.int8), rhs)
    llens = [50, 34, 128, 70, 199, 45, 90]
    loff, lcol, lcoef = [0], [], []
    for n in llens:
        lcol.append(np.sort(rng.choice(d, n, replace=False)))
        lcoef.append(_VALS[rng.randint(0, len(_VALS), n)])
        loff.append(loff[-1] + n)
    loff, lcol, lcoef = np.asarray(loff, np.int64), np.concatenate(lcol).astype(np.int32), np.concatenate(lcoef).astype(np.float32)
    owner = [0, 0, 0, 0, 0, 0, 2]
    lrhs = np.array([_dots(loff[i:i + 2] - loff[i], lcol[loff[i]:loff[i + 1]], lcoef[loff[i]:loff[i + 1]], sol[owner[i]])[0] + (i == 3)
                     for i in range(len(llens))])
    lazy = RawSys(len(llens), int(loff[-1]), d, loff, lcol, lcoef, np.array([2, 1, 0, 0, 2, 1, 2], np.int8), lrhs)
    return sys, lazy, np.array([0, 6, 6, 7], np.int64), sol


def many_long_case() -> Case:
    sys, lazy, off, sol = many_long_parts()
    return make("many_long", sys, lazy, off, sol, 1e-5, ref_matrices(sys, lazy, off, sol, 1e-5))


def d1_case() -> Case:
    """d = 1: x <= 1, x >= 0, 2 x == 1 at x = 0, 1, 0.5"""
    sys = RawSys(3, 3, 1, np.array([0, 1, 2, 3], np.int64), np.zeros(3, np.int32), np.array([1, 1, 2], np.float32),
                 np.array([0, 1, 2], np.int8), np.array([1.0, 0.0, 1.0]))
    sol = np.array([[0.0], [1.0], [0.5]], np.float32)
    return make("d1", sys, None, None, sol, 1e-5, ref_matrices(sys, None, None, sol, 1e-5))


def tol_edge_case() -> Case:
    """tol = 1e-5 lies between 2^-17 and 2^-16: a slack of 2^-17 is tight, one of 2^-16 is not (either sign); 2^-17 is low,
    1 - 2^-17 high; 0.5, 2^-16 and 1 - 2^-16 are neither"""
    e17, e16 = 2.0 ** -17, 2.0 ** -16
    sol = np.array([[0.5, 0.5, e17, 1 - e17, 0.5, e16, 1 - e16, 0.5]], np.float32)
    assert sol[0, 3] == 1 - e17 and sol[0, 6] == 1 - e16  # representable
    R = 4
    sys = RawSys(R, R, 8, np.arange(R + 1, dtype=np.int64), np.array([0, 1, 4, 7], np.int32), np.ones(R, np.float32),
                 np.array([0, 0, 1, 2], np.int8), np.array([0.5 + e17, 0.5 + e16, 0.5 - e17, 0.5 - e16]))
    mats = ref_matrices(sys, None, None, sol, 1e-5)
    assert len(mats[0]) == 2 + 2  # rows 0 and 2 are tight, columns 2 and 3 are at a bound
    return make("tol_edges", sys, None, None, sol, 1e-5, mats)


def tol_zero_case() -> Case:
    """tol = 0 is accepted; at a strictly interior point (some rows with slack 0 exactly) the cone is empty"""
    sys, _, _, sol = synth_parts()
    sys = sys._replace(rhs=_dots(sys.row_off, sys.col, sys.coef, sol[4]))  # every row's slack is 0 exactly
    mats = ref_matrices(sys, None, None, sol[4:], 0.0)
    assert len(mats[0]) == 0
    return make("tol_zero", sys, None, None, sol[4:], 0.0, mats)


def good_cases():
    return [sp_case(3, 3), sp_case(5, 5), tsp_case(8), tsp_case(6), vrp_case(), synth_case(), single_case(), long_row_case(),
            many_long_case(), d1_case(), tol_edge_case(), tol_zero_case()]


# ------------------------------------------------------------------ failures

def nan_case() -> Case:
    """NaN in one instance's sol: the neighbours are unaffected"""
    sys, lazy, off, sol = synth_parts()
    bad = sol.copy()
    bad[2, 5] = np.nan
    return make("nan_sol", sys, lazy, off, bad, 1e-5, ref_matrices(sys, lazy, off, sol, 1e-5), [0, 0, ST_BAD_INPUT, 0, 0])


def lazy_col_case() -> Case:
    """a lazy row of instance 1 with a column >= d"""
    sys, lazy, off, sol = synth_parts()
    col = lazy.col.copy()
    col[lazy.row_off[off[1] + 1] - 1] = sys.d  # the last entry of instance 1's row: still increasing, out of range
    return make("lazy_col", sys, lazy._replace(col=col), off, sol, 1e-5, ref_matrices(sys, lazy, off, sol, 1e-5), [0, ST_BAD_INPUT, 0, 0, 0])


def unsorted_case() -> Case:
    """a shared system with unsorted columns: every instance fails"""
    sys, lazy, off, sol = synth_parts()
    r = int(np.flatnonzero(np.diff(sys.row_off) >= 2)[-1])
    col = sys.col.copy()
    a = sys.row_off[r]
    col[a], col[a + 1] = col[a + 1], col[a]
    return make("unsorted", sys._replace(col=col), lazy, off, sol, 1e-5, ref_matrices(sys, lazy, off, sol, 1e-5), [ST_BAD_INPUT] * 5)


def long_bad_case(which: str) -> Case:
    """the long rows: `shared` -- a zero coefficient in the sixth long row of the shared system (second round, second group
    of lanes): every instance fails; `lazy` -- two columns swapped in the fifth long lazy row of instance 0: it alone fails"""
    sys, lazy, off, sol = many_long_parts()
    mats = ref_matrices(sys, lazy, off, sol, 1e-5)
    if which == "shared":
        coef = sys.coef.copy()
        coef[sys.row_off[6] + 77] = 0.0
        return make("long_bad_shared", sys._replace(coef=coef), lazy, off, sol, 1e-5, mats, [ST_BAD_INPUT] * 3)
    col = lazy.col.copy()
    a = lazy.row_off[4] + 150
    col[a], col[a + 1] = col[a + 1], col[a]
    return make("long_bad_lazy", sys, lazy._replace(col=col), off, sol, 1e-5, mats, [ST_BAD_INPUT, 0, 0])


def too_large_case() -> Case:
    """d = 40000, R = 30000 unit rows, all tight at sol = 0: 70000 rows.  A second instance at 0.5 is unaffected (no row)"""
    d, R = 40000, 30000
    sys = RawSys(R, R, d, np.arange(R + 1, dtype=np.int64), np.arange(R, dtype=np.int32), np.ones(R, np.float32), np.zeros(R, np.int8),
                 np.zeros(R))
    sol = np.zeros((2, d), np.float32)
    sol[1] = 0.5
    return make("too_large", sys, None, None, sol, 1e-5, [np.zeros((0, d), np.float32)] * 2, [ST_TOO_LARGE, 0])


def bad_cases():
    return [nan_case(), lazy_col_case(), unsorted_case(), long_bad_case("shared"), long_bad_case("lazy"), too_large_case()]


# ------------------------------------------------------------------ running and checking, for both tiers

def two_passes(case: Case, count, fill, up, down, slack: int = 0):
    """Both passes on sentinel-filled outputs with GUARD elements behind each.  count(sys, lazy, lazy_off, sol, N, tol,
    n_rows, n_ent, status) and fill(sys, lazy, lazy_off, sol, N, tol, ent_off, ent_cap, key, val, status) are the tier's
    entry points on the tier's arrays; up / down move a numpy array to the tier and back.  -> (rc, outputs dict of numpy
    arrays, guards included)."""
    def sys_up(s):
        return None if s is None else s._replace(**{k: up(getattr(s, k)) for k in ("row_off", "col", "coef", "sense", "rhs")})

    N = case.sol.shape[0]
    sys, lazy = sys_up(case.sys), sys_up(case.lazy)
    lazy_off = None if case.lazy_off is None else up(case.lazy_off)
    sol = up(case.sol)
    t = {"n_rows": up(np.full(N + GUARD, FILL_I, np.int32)), "n_ent": up(np.full(N + GUARD, FILL_I, np.int64)),
         "status": up(np.full(N + GUARD, FILL_I, np.int32)), "fill_status": up(np.full(N + GUARD, FILL_I, np.int32))}
    rc = count(sys, lazy, lazy_off, sol, N, case.tol, t["n_rows"], t["n_ent"], t["status"])
    if rc != 0:
        return rc, {k: down(v) for k, v in t.items()}
    ent_off = np.zeros(N + 1, np.int64)
    np.cumsum(down(t["n_ent"])[:N], out=ent_off[1:])
    cap = int(ent_off[-1])
    t["key"], t["val"] = up(np.full(cap + slack + GUARD, FILL_I, np.int32)), up(np.full(cap + slack + GUARD, FILL_F, np.float32))
    rc = fill(sys, lazy, lazy_off, sol, N, case.tol, up(ent_off), cap + slack, t["key"], t["val"], t["fill_status"])
    out = {k: down(v) for k, v in t.items()}
    out["ent_off"] = ent_off
    return rc, out


def check(case: Case, rc: int, o, what=None):
    """the outputs of two_passes against the case's expectation, exactly; the guards (and the slack) untouched"""
    what = (case.name, what)
    N = len(case.sol)
    assert rc == 0, what
    for k in ("n_rows", "n_ent", "status", "fill_status"):
        assert (o[k][N:] == FILL_I).all(), (what, k, "written beyond its end")
    assert np.array_equal(o["status"][:N], case.status), (what, o["status"][:N])
    assert np.array_equal(o["fill_status"][:N], case.status), (what, o["fill_status"][:N])
    assert np.array_equal(o["n_rows"][:N], case.rows), (what, o["n_rows"][:N], case.rows)
    e = case.expect
    assert int(o["n_rows"][:N].max()) == e.m_max, what
    assert np.array_equal(o["ent_off"], e.ent_off.numpy()), (what, o["ent_off"], e.ent_off)
    Z = int(e.ent_off[-1])
    assert np.array_equal(o["key"][:Z], e.key.numpy()), (what, "key")
    assert np.array_equal(o["val"][:Z].view(np.int32), e.val.numpy().view(np.int32)), (what, "val")
    assert (o["key"][Z:] == FILL_I).all() and (o["val"][Z:] == FILL_F).all(), (what, "written beyond the counted entries")
