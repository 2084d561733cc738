"""The operators of the Newton loop alone: cases and checks shared by the two tiers (TEST INFRASTRUCTURE).

tests/test_ops_emul.py (CPU tier, SIMT emulation) and tests/test_gpu_ops.py (the MI355X) differ only in the `run`
function they pass in and in the cap on band_weight: run(op, ctx, pm1, cases, seed=0) -> per case {"out", "outf", "outi"} (emul_lib.op_run_host).
Everything else -- how a reduced cone is drawn (directly as the arrays of a SolveView, rows exactly on the dispatch
thresholds; nothing goes through build_cone), the restatement (ops_ref.py), the bound, the margins that are recorded -- is
here.  Cases are seeded and generated when a test runs; nothing is stored.
"""

from __future__ import annotations

import json
import os

import numpy as np

import limit_cones as LCN
import ops_ref as R

NW = {"w1": 1, "b2": 2, "b4": 4, "l2": 2, "l4": 4, "solo": 1}
NT = {k: 64 * v for k, v in NW.items()}
SMALL_CTX, LARGE_CTX = ("w1", "b2", "b4"), ("w1", "l2", "l4")

# ---- margins: worst error / bound per entry; the GPU tier writes profiles/ops_margins.json, the CPU tier only where
# the environment variable CAVE_OPS_MARGINS names a JSON file (it also redirects the GPU tier)
MARGINS: dict = {}


def record(entry, ratio):
    MARGINS[entry] = max(MARGINS.get(entry, 0.0), float(ratio))


def dump_margins(tier, default=None):
    path = os.environ.get("CAVE_OPS_MARGINS", default)
    if not path or not MARGINS:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[tier] = {k: float("%.3g" % v) for k, v in sorted(MARGINS.items())}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the agreement must be exact; an unwritten element (NaN) is inf"""
    got = np.asarray(got, np.float64).ravel()
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    err = R._f64(np.abs(R._num(got) - np.asarray(ref).ravel())) if np.asarray(ref).dtype != object else \
        np.array([abs(float(a - b)) for a, b in zip(R._num(got), np.asarray(ref).ravel())])
    bound = np.broadcast_to(np.asarray(bound, np.float64).ravel() if np.ndim(bound) else float(bound), err.shape)
    out = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(out.max())


# ------------------------------------------------------------------------------------------------------------- cones
def make_cone(M, pm1, usign=None, vkind=None, rng=None):
    """the SolveView arrays of the reduced rows M [p, d] (float32-exact entries; pm1: all +-1, sign in bit 15)"""
    M = np.asarray(M, np.float32).astype(np.float64)
    p, d = M.shape
    rng = rng or np.random.default_rng(p * 1000 + d)
    nzr, nzc = np.nonzero(M)            # row-major: CSR order, columns ascending within a row
    mptr = np.concatenate([[0], np.cumsum(np.bincount(nzr, minlength=p))]).astype(np.uint32)
    vals = M[nzr, nzc]
    o = np.lexsort((nzr, nzc))          # CSC order, rows ascending within a column
    cptr = np.concatenate([[0], np.cumsum(np.bincount(nzc, minlength=d))]).astype(np.uint32)
    if pm1:
        assert (np.abs(vals) == 1).all()
    sgn = lambda v: np.where(v < 0, 0x8000, 0) if pm1 else 0
    lens = np.diff(mptr.astype(np.int64))
    c = {"d": d, "p": p, "pm1": bool(pm1), "M": M, "mptr": mptr, "cptr": cptr,
         "mcol": (nzc | sgn(vals)).astype(np.uint16), "cvar": (nzr[o] | sgn(vals[o])).astype(np.uint16),
         "mval": None if pm1 else vals.astype(np.float32), "cvalc": None if pm1 else vals[o].astype(np.float32),
         "usign": (rng.integers(0, 4, d) if usign is None else np.asarray(usign)).astype(np.uint8),
         "vkind": (rng.integers(0, 2, p) if vkind is None else np.asarray(vkind)).astype(np.uint8),
         "longrow": np.flatnonzero(lens > R.K_LONG_ROW).astype(np.uint32),
         "teamrow": np.flatnonzero(lens > R.K_TEAM_ROW).astype(np.uint32)}
    return c


def case(c, ins=(), s=(0, 0, 0, 0), n_out=0, fin=None, **kw):
    k = dict(c)
    k.update(ins=[np.asarray(a, np.float64) for a in ins], s=tuple(s) + (0,) * (4 - len(s)), n_out=n_out,
             fin=np.zeros(2 * c["d"], np.float32) if fin is None else np.asarray(fin, np.float32), **kw)
    return k


def _vals(rng, n, pm1):
    return rng.choice([-1.0, 1.0], n) if pm1 else (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)).astype(np.float32)


def rows_by_len(rng, d, lens, pm1):
    M = np.zeros((len(lens), d), np.float32)
    for i, n in enumerate(lens):
        cols = rng.choice(d, n, replace=False)
        M[i, cols] = _vals(rng, n, pm1)
    return M


def rows_by_colcount(rng, p, counts, pm1):
    M = np.zeros((p, len(counts)), np.float32)
    for k, n in enumerate(counts):
        rows = rng.choice(p, n, replace=False)
        M[rows, k] = _vals(rng, n, pm1)
    return M


def row_cones(pm1, ctx, streamed):
    """rows of 1-5 entries (the four partial sums), 63 / 64 / 65 (kLongRow), 255 / 256 / 257 (one U x WL chunk),
    1024 / 1025 (kTeamRow), one of 4 700, an empty row between long rows, nlong of 1, NW, NW + 1, 2 NW + 1, p of 1,
    15 / 16 / 17, 63 / 64 / 65; streamed: more rows than R x NT"""
    rng = np.random.default_rng([11, int(pm1), NW[ctx], int(streamed)])
    nw = NW[ctx]
    out = [make_cone(rows_by_len(rng, 130, [1, 2, 3, 4, 5, 63, 64, 65, 7, 64, 65, 1], pm1), pm1),
           make_cone(rows_by_len(rng, 5, [3], pm1), pm1),
           make_cone(rows_by_len(rng, 300, [255, 256, 257], pm1), pm1),
           make_cone(rows_by_len(rng, 1100, [1024, 1025, 3, 1025], pm1), pm1),
           make_cone(rows_by_len(rng, 4800, [70, 0, 4700, 0, 66, 2], pm1), pm1)]
    for p in (15, 16, 17, 63, 64, 65):
        out.append(make_cone(rows_by_len(rng, 40, list(rng.integers(1, 10, p)), pm1), pm1))
    for nl in sorted({1, nw, nw + 1, 2 * nw + 1}):
        out.append(make_cone(rows_by_len(rng, 140, [65 + 7 * i for i in range(nl)] + [3], pm1), pm1))
    if streamed:
        p = 8 * NT[ctx] + 6
        out.append(make_cone(rows_by_len(rng, 64, list(rng.integers(0, 6, p)), pm1), pm1))
    return out


COL_COUNTS = (0, 1, 2, 3, 4, 8, 9, 12)


def col_cones(pm1, seed, sizes=(1, 63, 64, 65, 255, 256, 257, 1025), p=16):
    """column counts 0 .. 4 (E = 3 of the gather, E = 4 of dense_gradient), 8, 9, 12 (E = 8 of dense_hessian and its
    tail loop); d of 1, 63 / 64 / 65, 255 / 256 / 257 and 1025 (G x NT)"""
    rng = np.random.default_rng([12, int(pm1), seed])
    out = []
    for d in sizes:
        counts = [COL_COUNTS[(k + d) % len(COL_COUNTS)] for k in range(d)]
        out.append(make_cone(rows_by_colcount(rng, p, counts, pm1), pm1, rng=rng))
    out.append(make_cone(rows_by_colcount(rng, 1, [1, 0, 1, 1, 0], pm1), pm1, rng=rng))
    return out


def residual(rng, d, scale=1.0):
    """negative, exactly 0 and positive next to every usign"""
    r = rng.standard_normal(d) * scale
    r[rng.random(d) < 0.25] = 0.0
    return r


# ------------------------------------------------------------------------------------------------------------ gathers
def check_gather(run, op, ctx, pm1, tag):
    rng = np.random.default_rng([21, int(pm1), NW[ctx]])
    cones = col_cones(pm1, 1)
    cases, refs = [], []
    for i, c in enumerate(cones):
        th = rng.standard_normal(c["p"])
        y = rng.standard_normal(c["d"]).astype(np.float32)
        sgn, nobase = (-1.0, 0) if i % 3 else (1.0, 1)
        cases.append(case(c, [th], (sgn,), c["d"], fin=np.concatenate([y, y * 0]), flags=nobase))
        refs.append(R.gather(c, th, sgn, None if nobase else y))
    worst = 0.0
    for k, o, (ref, bound) in zip(cases, run(op, ctx, pm1, cases), refs):
        rt = ratio(o["out"], ref, bound)
        assert rt <= 1.0, (tag, ctx, pm1, k["d"], rt)
        worst = max(worst, rt)
    record(tag, worst)


# ---------------------------------------------------------------------------------------------- clip and line search
def _line_cone(rng, d, p=3):
    return make_cone(rows_by_colcount(rng, p, [1] * d, True), True, usign=np.arange(d) % 4, rng=rng)


def check_refresh(run, ctx, rb):
    rng = np.random.default_rng([31, NW[ctx], rb])
    op = "refresh_rb" if rb else "refresh"
    cases, refs = [], []
    for d in (1, 63, 64, 65, 257, 8 * NT[ctx] + 3):
        c = _line_cone(rng, d)
        r = residual(rng, d)
        cases.append(case(c, [r], n_out=d + 1))
        refs.append(R.refresh(c, r, NT[ctx]))
    worst = 0.0
    for k, o, (rc, f, bf) in zip(cases, run(op, ctx, True, cases), refs):
        assert np.array_equal(o["out"][:-1], R._f64(rc)), (ctx, k["d"])   # the clip returns r or 0
        rt = ratio(o["out"][-1:], [f], bf)
        assert rt <= 1.0, (ctx, k["d"], rt)
        worst = max(worst, rt)
    record(op, worst)


def check_dphi(run, ctx, rb):
    """dyadic r, q, alpha: r - alpha q, its clip and every sum are exact, and r - alpha q == 0 occurs next to every
    usign -> the outputs are the reference's to the bit.  Gaussian r, q: the bound."""
    rng = np.random.default_rng([32, NW[ctx], rb])
    op = "dphi_rb" if rb else "dphi"
    cases, refs = [], []
    for d in (1, 63, 65, 257, 8 * NT[ctx] + 3):
        for alpha in (0.0, 0.25, 1.0, 1.5):
            c = _line_cone(rng, d)
            q = rng.integers(-1024, 1025, d) / 256.0
            r = rng.integers(-1024, 1025, d) / 256.0
            hit = rng.random(d) < 0.3
            r[hit] = alpha * q[hit]
            cases.append(case(c, [r, q], (alpha,), 2))
            refs.append(("exact",) + R.dphi(c, r, q, alpha, NT[ctx]))
        c = _line_cone(rng, d)
        r, q = rng.standard_normal(d), rng.standard_normal(d)
        cases.append(case(c, [r, q], (0.7,), 2))
        refs.append(("bound",) + R.dphi(c, r, q, 0.7, NT[ctx]))
    worst = 0.0
    for k, o, (how, d1, d2, b1, b2, gap) in zip(cases, run(op, ctx, True, cases), refs):
        if how == "exact":
            assert o["out"][0] == float(d1) and o["out"][1] == float(d2), (ctx, k["d"], k["s"], o["out"], float(d1), float(d2))
        else:
            assert gap > 1e-9
            rt = max(ratio(o["out"][:1], [d1], b1), ratio(o["out"][1:], [d2], b2))
            assert rt <= 1.0, (ctx, k["d"], rt)
            worst = max(worst, rt)
    record(op, worst)


def check_update_theta(run, ctx, rb):
    rng = np.random.default_rng([33, NW[ctx], rb])
    op = "update_rb" if rb else "update"
    cases, refs = [], []
    for p in (1, 63, 65, 8 * NT[ctx] + 3):
        for alpha, amax in ((1.0, 1.0), (1.0, 2.5), (0.5, 2.5), (2.5, 2.5), (0.3, 0.3)):
            M = rows_by_len(rng, 4, [1] * p, True)
            c = make_cone(M, True, rng=rng)
            dv = rng.integers(-64, 65, p) / 16.0
            theta = np.where(c["vkind"] == 0, rng.integers(0, 65, p) / 16.0, rng.integers(-64, 65, p) / 16.0)
            blocked = rng.random(p) < 0.3
            theta[blocked & (dv < 0)] = (-amax * dv)[blocked & (dv < 0)]  # exactly at the bound at alpha = amax
            tc = np.where(rng.random(p) < 0.3, 0.0, rng.random(p))
            cases.append(case(c, [theta, tc, dv], (alpha, amax), p))
            refs.append(R.update_theta(c, theta, tc, dv, alpha, amax))
    for k, o, (t, tol, zero) in zip(cases, run(op, ctx, True, cases), refs):
        got = o["out"]
        assert np.isfinite(got).all()
        assert (np.abs(got - R._f64(t)) <= tol).all(), (ctx, k["p"], k["s"])
        assert (got[zero] == 0.0).all() and not np.signbit(got[zero]).any(), (ctx, k["p"], k["s"])
        assert zero.any() or k["p"] < 8
        # ... and what the function is FOR, stated without its expressions: multipliers with a bound stay feasible, and
        # at the end of the feasible segment (alpha = amax) a row whose exact theta + amax dv is not positive sits at 0
        th, dv, (alpha, amax) = k["ins"][0], k["ins"][2], k["s"][:2]
        bnd = np.asarray(k["vkind"]) == 0
        assert (got[bnd] >= 0.0).all(), (ctx, k["p"], k["s"])
        if alpha == amax:
            hit = bnd & (R._f64(R._num(th) + amax * R._num(dv)) <= 0.0)
            assert (got[hit] == 0.0).all(), (ctx, k["p"], k["s"])
        free = ~bnd
        assert (np.abs(got[free] - R._f64(R._num(th) + alpha * R._num(dv))[free]) <= tol[free]).all()
    record(op, 0.0)


def exact_step_cases():
    """(x, y, psi0, amax, what)"""
    return [
        ([0.0, 2.0], [-1.0, 1.0], -1.0, 1.0, "root exactly at the full step, amax = 1"),
        ([0.0, 0.5, 2.0], [-1.0, -0.2, 3.0], -1.0, 1.0, "root below 1"),
        ([0.0, 1.0, 3.0, 8.0], [-1.0, -0.6, -0.1, 2.0], -1.0, 1e300, "root above 1, open segment (the hi < 1e299 branch)"),
        ([0.0, 1.0, 3.0, 8.0], [-1.0, -0.6, -0.1, 2.0], -1.0, 1.0, "a bound blocks at amax = 1"),
        ([0.0, 4.0, 5.0, 9.0], [-1.0, -1.0, -0.5, 3.0], -1.0, 1e300, "zero curvature at the start: doubling"),
        ([0.0, 4.0, 5.0, 9.0], [-1.0, -1.0, -0.5, 3.0], -1.0, 6.0, "zero curvature at the start, bracketed"),
        ([0.0, 0.25, 0.5, 4.0], [-1e-300, -0.5e-300, 1e-300, 9e-300], -1e-300, 1.0, "psi0 of 1e-300"),
        ([0.0, 1e-3, 2e-3, 1.0], [-1.0, -0.9, 5.0, 6.0], -1.0, 1.0, "kink far below the start"),
        ([0.0, 3.0, 3.0 + 1e-13, 10.0], [-1.0, -0.9, 50.0, 60.0], -1.0, 10.0, "a jump: the bracket collapses"),
    ]


def check_exact_step(simt):
    psitol = simt.psitol()
    for x, y, psi0, amax, what in exact_step_cases():
        alpha, evals = simt.exact_step(x, y, psi0, amax)
        assert 0.0 < alpha <= amax and 1 <= evals <= 60, (what, alpha, evals)
        d1 = R.phi_pl(R._num(x), R._num(y), R._num([alpha])[0])
        ok_slope = abs(float(d1)) <= psitol * abs(psi0)
        ok_end = alpha == amax and d1 < 0
        # a collapsed bracket: phi' changes sign within 1e-15 alpha of the returned point
        lo, hi = alpha * (1 - 4e-15), alpha * (1 + 4e-15)
        ok_collapse = float(R.phi_pl(R._num(x), R._num(y), R._num([lo])[0])) < 0 < float(R.phi_pl(R._num(x), R._num(y), R._num([hi])[0]))
        assert ok_slope or ok_end or ok_collapse, (what, alpha, float(d1), evals)


# ----------------------------------------------------------------------------------------------------------- gradient
def check_gradient(run, op, ctx, pm1, tag):
    rng = np.random.default_rng([41, int(pm1), NW[ctx]])
    cones = row_cones(pm1, ctx, op == "grad_st")
    cases, refs = [], []
    for c in cones:
        rc = residual(rng, c["d"])
        cases.append(case(c, [rc], n_out=c["p"]))
        refs.append(R.gradient(c, rc))
    worst = 0.0
    for k, o, (g, bound, _) in zip(cases, run(op, ctx, pm1, cases), refs):
        rt = ratio(o["out"], g, bound)
        assert rt <= 1.0, (tag, ctx, pm1, k["p"], k["d"], rt)
        worst = max(worst, rt)
    record(tag, worst)


def dense_gradient_cases(pm1):
    """the column-count cones at p <= 128, a row whose products all have one sign at rmax (the sum meets fixed_scale's
    bound), rc all zero, |rc| around 1e-300 and 1e300, general entries with cancelling signs"""
    rng = np.random.default_rng([42, int(pm1)])
    cases, refs = [], []
    for i, c in enumerate(col_cones(pm1, 2) + col_cones(pm1, 3, sizes=(200, 257), p=128)):
        vm, ml = R.cone_scales(c)
        # (1e300, or as close to it as keeps rmax x gcol_bound a finite double: the product's residuals come from float32 y)
        rc = residual(rng, c["d"], scale=(1.0, 1e-300, min(1e300, 1e305 / (vm * ml)), 1e-3)[i % 4])
        if i == 4:
            rc[:] = 0.0
        cases.append(case(c, [rc], (vm * ml,), c["p"]))
        refs.append((R.gradient(c, rc), R.dense_gradient_bound(c, rc, vm * ml)))
    # one sign at rmax: every product of row 0 equals +vm * rmax, the row is the longest one
    M = np.zeros((4, 300), np.float32)
    M[0, :] = -1.0 if pm1 else np.float32(-3.5)
    M[1, ::3] = 1.0
    M[2, 5] = 1.0
    c = make_cone(M, pm1)
    vm, ml = R.cone_scales(c)
    rc = np.full(300, 2.75)
    cases.append(case(c, [rc], (vm * ml,), 4))
    refs.append((R.gradient(c, rc), R.dense_gradient_bound(c, rc, vm * ml)))
    return cases, refs


def check_dense_gradient(run, ctx, pm1, seeds=(0,)):
    cases, refs = dense_gradient_cases(pm1)
    outs = [run("grad_dense", ctx, pm1, cases, seed=s) for s in seeds]
    worst = 0.0
    for i, (k, ((g, _, _), (bound, sc))) in enumerate(zip(cases, refs)):
        rt = ratio(outs[0][i]["out"], g, bound)
        assert rt <= 1.0, (ctx, pm1, i, k["p"], k["d"], rt, sc)
        worst = max(worst, rt)
        for o in outs[1:]:  # integer adds: the same bits in any order
            assert np.array_equal(o[i]["out"], outs[0][i]["out"]), (ctx, pm1, i)
    record("dense_gradient", worst)


# ------------------------------------------------------------------------------------------------------------ weights
def weight_cases():
    rng = np.random.default_rng(51)
    out = []
    for inv_mu in (0.0, 1.0, 37.5, 1e6, 1e-6):
        d = 260
        r = residual(rng, d) * 10.0 ** rng.uniform(-3, 3, d)
        r[:8] = [0.0, 1e-15, 1e-14, 1.0, -1.0, 4.0, -4.0, 1e-300]
        out.append((np.arange(d) % 4, r, inv_mu))
    return out


def check_band_weight(run, cap):
    cases = [case(make_cone(np.zeros((0, len(r))), True, usign=u, vkind=[]), [r], (im,), len(r)) for u, r, im in weight_cases()]
    worst = 0.0
    for (u, r, im), o in zip(weight_cases(), run("weight", "w1", True, cases)):
        ref = R.band_weight(u, r, im)
        rf = R._f64(ref)
        exact = (rf == 0.0) | (rf == 1.0) | (rf == 0.5)
        assert np.array_equal(o["out"][exact & (u % 3 == 0)], rf[exact & (u % 3 == 0)])
        rt = ratio(o["out"], ref, R.band_weight_scale(u, ref, im) * R.U)
        assert rt <= cap, (im, rt)
        worst = max(worst, rt / cap)
    record("band_weight", worst)
    return worst * cap


WEIGHT_EXTREMES = ((2, 1e155, 1.0), (2, 1e300, 1.0), (1, -1e155, 1.0), (2, -1e155, 1.0), (2, 0.0, float("inf")), (1, 0.0, float("inf")))


def band_weight_extremes(run):
    """t / mu of 1e155 and 1e300 (z^2 overflows) and 1 / mu = inf with t = 0 -> what band_weight returns"""
    cases = [case(make_cone(np.zeros((0, 1)), True, usign=[u], vkind=[]), [[r]], (im,), 1) for u, r, im in WEIGHT_EXTREMES]
    return [float(o["out"][0]) for o in run("weight", "w1", True, cases)]


# ------------------------------------------------------------------------------------------------------------ Hessian
def sixteenths(rng, d):
    w = rng.integers(0, 17, d) / 16.0
    w[:3] = [0.0, 1.0, 0.5]
    return w


def band_cone(rng, p, bw, d, pm1):
    """columns inside a window of bw + 1 rows; every fifth column spans exactly bw"""
    M = np.zeros((p, d), np.float32)
    for k in range(d):
        j = int(rng.integers(0, p - bw)) if p > bw else 0
        span = min(bw, p - 1 - j)
        if k % 5 == 0 and span >= 1:
            rows = np.unique(np.concatenate([[j, j + span], j + rng.integers(0, span + 1, int(rng.integers(0, 4)))]))
        else:
            rows = j + rng.choice(span + 1, int(rng.integers(0, min(4, span + 1) + 1)), replace=False)
        M[rows, k] = _vals(rng, len(rows), pm1)
    return M


def one_sign_cone(pm1, vkind=(1, 0, 1)):
    """the longest row carries the largest |entry| on EVERY column with one sign: with weights 1 its diagonal entry of H
    is vm x vm x ml, the very bound fixed_scale is given (a scale that overflows only when a whole row has one sign)"""
    M = np.zeros((3, 40), np.float32)
    M[0, :] = -1.0 if pm1 else np.float32(-3.5)
    M[1, ::3] = 1.0
    M[2, 1::4] = -1.0 if pm1 else np.float32(0.75)
    return make_cone(M, pm1, vkind=vkind)


def hessian_weights(rng, c, how, wcap=4):
    """-> (in0, inv_mu, flags bit 1, the weights in working precision, absolute error of each weight as computed: wcap u
    (w + |q| / 2) for band_weight, the cap test_band_weight holds the tier to)"""
    d = c["d"]
    if how == "ones":
        return np.ones(d), 0.0, 2, np.ones(d), np.zeros(d)
    if how == "usign0":  # band_weight returns exactly 1 for a coordinate without unit rows, whatever r and mu
        assert not c["usign"].any()
        return residual(rng, d), 4.0, 0, np.ones(d), np.zeros(d)
    if how == "grid":
        w = sixteenths(rng, d)
        return w, 0.0, 2, w, np.zeros(d)
    if how == "array":
        w = rng.random(d)
        w[:4] = [0.0, 1e-15, 1e-14, 1.0]
        return w, 0.0, 2, w, np.zeros(d)
    r = residual(rng, d)
    inv_mu = 0.0 if how == "binary" else 4.0
    wl = R.band_weight(c["usign"], r, inv_mu)
    return r, inv_mu, 0, R._f64(wl), wcap * R.U * R.band_weight_scale(c["usign"], wl, inv_mu)


def _hess_bound(c, w, werr, hscale):
    """werr: absolute error of each weight as the product computes it (band_weight; 0 for weights read from an array)"""
    H, n, mx = R.hessian(c, w)
    A = np.abs(c["M"])
    return H, n * (0.5 / hscale + R.U * mx) + (A * werr[None, :]) @ A.T


def check_band_hessian(run, ctx, pm1, seeds=(0,), wcap=4):
    rng = np.random.default_rng([61, NW[ctx], int(pm1)])
    cases, metas = [], []
    shapes = [(2, 1, 9, 1), (5, 4, 40, 1), (34, 33, 70, 1), (12, 1, 30, 0), (130, 4, 300, 0), (130, 33, 260, 0), (40, 33, 1025, 0)]
    for i, (p, bw, d, in_lds) in enumerate(shapes):
        for how in ("grid", "array", "weight", "binary"):
            c = make_cone(band_cone(rng, p, bw, d, pm1), pm1, rng=rng)
            x, inv_mu, fl, w, wrel = hessian_weights(rng, c, how, wcap)
            cases.append(case(c, [x], (inv_mu,), p * (bw + 1) + 2, ldh=bw + 1, flags=fl | in_lds))
            metas.append((c, w, wrel, how, bw + 1))
    for in_lds in (1, 0):
        for how in ("ones", "usign0"):
            c = one_sign_cone(pm1)
            if how == "usign0":
                c["usign"][:] = 0
            x, inv_mu, fl, w, wrel = hessian_weights(rng, c, how, wcap)
            cases.append(case(c, [x], (inv_mu,), 3 * 3 + 2, ldh=3, flags=fl | in_lds))
            metas.append((c, w, wrel, how, 3))
    outs = [run("band_h", ctx, pm1, cases, seed=s) for s in seeds]
    worst = 0.0
    for i, (c, w, wrel, how, ldh) in enumerate(metas):
        o = outs[0][i]["out"]
        vm, ml = R.cone_scales(c)
        hs = R.fixed_scale(vm, vm * ml)
        assert o[-2] == hs and o[-1] == vm * ml, (ctx, i, o[-2:], hs)          # the product's scale is the reference's
        H, bound = _hess_bound(c, w, wrel, hs)
        ref, bl = R.band_layout(H, ldh), R.band_layout(bound, ldh)
        if how in ("ones", "usign0"):
            vm, ml = R.cone_scales(c)
            assert float(H[0, 0]) == vm * vm * ml and o[0] == vm * vm * ml, (ctx, i, how, o[0])  # the bound itself, exactly
        if pm1 and how in ("grid", "binary", "ones", "usign0"):
            assert np.array_equal(o[:-2], R._f64(ref)), (ctx, i, how)          # multiples of 1/16 below 2^12: exact
        rt = ratio(o[:-2], ref, bl)
        assert rt <= 1.0, (ctx, pm1, i, how, rt)
        worst = max(worst, rt)
        for oo in outs[1:]:
            assert np.array_equal(oo[i]["out"], o), (ctx, pm1, i)
    record("band_hessian", worst)


def dense_order_cases(pm1):
    """free / bound mixes with nF of 0, 1, p - 1 and p; p of 1, 2, 127 and 128 (the folded-triangle index)"""
    rng = np.random.default_rng([62, int(pm1)])
    out = []
    for p in (1, 2, 16, 127, 128):
        for nF in sorted({0, 1, p - 1, p}):
            if nF < 0 or nF > p:
                continue
            vk = np.zeros(p, np.uint8)
            vk[rng.choice(p, nF, replace=False)] = 1
            d = 70 if p > 16 else 33
            counts = [min(COL_COUNTS[(k + p) % len(COL_COUNTS)], p) for k in range(d)]
            out.append(make_cone(rows_by_colcount(rng, p, counts, pm1), pm1, vkind=vk, rng=rng))
    return out


def check_dense_hessian(run, ctx, pm1, seeds=(0,), wcap=4):
    rng = np.random.default_rng([63, NW[ctx], int(pm1)])
    cases, metas = [], []
    for i, c in enumerate(dense_order_cases(pm1)):
        how = ("grid", "array", "weight", "binary")[i % 4]
        x, inv_mu, fl, w, wrel = hessian_weights(rng, c, how, wcap)
        cases.append(case(c, [x], (inv_mu,), R.fold_entries(c["p"]) + 2 * c["p"] + 3, flags=fl))
        metas.append((c, w, wrel, how))
    for how, vk in (("ones", (1, 0, 1)), ("usign0", (0, 1, 0)), ("ones", (0, 0, 0))):
        c = one_sign_cone(pm1, vk)
        if how == "usign0":
            c["usign"][:] = 0
        x, inv_mu, fl, w, wrel = hessian_weights(rng, c, how, wcap)
        cases.append(case(c, [x], (inv_mu,), R.fold_entries(3) + 2 * 3 + 3, flags=fl))
        metas.append((c, w, wrel, how))
    outs = [run("dense_h", ctx, pm1, cases, seed=s) for s in seeds]
    worst = 0.0
    for i, (c, w, wrel, how) in enumerate(metas):
        o, p = outs[0][i]["out"], c["p"]
        ne = R.fold_entries(p)
        pos, ordr, nF = R.dense_order(c["vkind"])
        assert np.array_equal(o[ne:ne + p], pos) and np.array_equal(o[ne + p:ne + 2 * p], ordr) and o[ne + 2 * p] == nF, (ctx, i)
        vm, ml = R.cone_scales(c)
        hs = R.fixed_scale(vm, vm * ml)
        assert o[ne + 2 * p + 1] == hs and o[ne + 2 * p + 2] == vm * ml
        H, bound = _hess_bound(c, w, wrel, hs)
        ref, bl = R.fold_layout(H, pos), R.fold_layout(bound, pos)
        if how in ("ones", "usign0"):
            vm, ml = R.cone_scales(c)
            at = R.fold_base(p, int(pos[0]))
            assert float(H[0, 0]) == vm * vm * ml and o[at] == vm * vm * ml, (ctx, i, how, o[at])  # the bound itself
        if pm1 and how in ("grid", "binary", "ones", "usign0"):
            assert np.array_equal(o[:ne], R._f64(ref)), (ctx, i, how)
        rt = ratio(o[:ne], ref, bl)
        assert rt <= 1.0, (ctx, pm1, i, how, p, rt)
        worst = max(worst, rt)
        for oo in outs[1:]:
            assert np.array_equal(oo[i]["out"], o), (ctx, pm1, i)
    record("dense_hessian", worst)


# ----------------------------------------------------------------------------------------------------------- epilogue
EP_FLAGS = {"proj": 1, "rnorm": 2, "target": 4, "loss": 8, "grad": 16}


def epilogue_cases():
    rng = np.random.default_rng(71)
    out = []
    for d in (1, 63, 65, 257):
        for mode in range(6):
            for j, (sign, what) in enumerate(((1.0, "plain"), (-1.0, "plain"), (1.0, "empty"), (-1.0, "inside"), (1.0, "zero"), (-1.0, "tiny"))):
                y = rng.standard_normal(d).astype(np.float32)
                if what == "zero":
                    y[:] = 0
                if what == "tiny":
                    y *= np.float32(1e-9 / max(np.linalg.norm(y.astype(np.float64)), 1e-30))
                res = rng.standard_normal(d) * 0.3 * float(np.abs(y).max())
                f = 1e-16 if what == "inside" else 0.5 * float(res @ res) + 1e-12
                avg = rng.standard_normal(d).astype(np.float32)
                avg /= np.float32(max(np.linalg.norm(avg), 1e-6))
                out.append(dict(d=d, mode=mode, sign=sign, ratio=0.2 + 0.1 * j, empty=int(what == "empty"), y=y, res=res, f=f,
                                avg=avg, flags=0, what=what))
    base = dict(out[2 * 36 + 2 * 6])  # d = 65, INNER, plain: every combination of null outputs
    for fl in range(1, 32):
        out.append(dict(base, flags=fl))
    return out


def _ep_case(e):
    d = e["d"]
    c = make_cone(np.zeros((0, d)), True, usign=np.zeros(d), vkind=[])
    return case(c, [e["res"]], (e["f"], e["sign"], e["ratio"]), 0, fin=np.concatenate([e["y"], e["avg"]]), mode=e["mode"],
                flags=e["flags"], empty=e["empty"], n_outf=3 * d + 2)


def check_epilogue(run, ctx):
    eps = epilogue_cases()
    outs = run("epilogue", ctx, True, [_ep_case(e) for e in eps])
    worst = 0.0
    full = None
    for e, o in zip(eps, outs):
        d, of = e["d"], o["outf"]
        got = {"proj": of[:d], "target": of[d:2 * d], "grad": of[2 * d:3 * d], "rnorm": of[3 * d:3 * d + 1], "loss": of[3 * d + 1:]}
        ref, scale = R.epilogue(e["mode"], e["sign"], e["ratio"], e["empty"], e["y"], e["res"], e["f"], e["avg"])
        if e["flags"] == 0 and e["mode"] == R.MODE_INNER and e["d"] == 65 and e["what"] == "plain" and e["sign"] == 1.0:
            full = got
        for name, g in got.items():
            if name not in ref or (e["flags"] & EP_FLAGS[name]):
                assert np.isnan(g).all(), (ctx, e["mode"], name, "written although null / not an output of the mode")
                continue
            if e["flags"]:
                assert np.array_equal(g, full[name]), (ctx, e["flags"], name)  # the others unchanged
                continue
            rv = np.atleast_1d(ref[name])
            if e["mode"] == R.MODE_AVG:
                assert np.array_equal(g, e["avg"])
                continue
            bound = 2.0 ** -24 * np.abs(R._f64(rv)) + d * R.U * scale[name]
            rt = ratio(g, rv, bound)
            assert rt <= 1.0, (ctx, d, e["mode"], e["what"], name, rt)
            worst = max(worst, rt)
    record("epilogue", worst)


# ---------------------------------------------------------------------------------------------------------- lite form
def lite_cones(seed=5):
    """the cones of limit_cones.IN_CASES: reduced rows of +-1, [free | bound]"""
    out = []
    for i, lc in enumerate(LCN.IN_CASES):
        rng = np.random.default_rng([seed, i])
        M = LCN.draw_rows(rng, lc.d, lc.p, lc.nnz, lc.col_cap)
        vk = np.concatenate([np.ones(lc.n_free, np.uint8), np.zeros(lc.n_bound, np.uint8)])
        c = make_cone(M, True, vkind=vk, rng=rng)
        c["chn8"] = lc.chn8
        out.append(c)
    return out


def check_lite_gather_gradient(run):
    rng = np.random.default_rng(81)
    cones = lite_cones()
    gc, gr, rc_cases, rr = [], [], [], []
    for c in cones:
        d, p = c["d"], c["p"]
        x = rng.standard_normal(p)
        y = rng.standard_normal(d).astype(np.float32)
        gc.append(case(c, [np.concatenate([x, np.zeros(33 - p)])], (-1.0,), d, fin=np.concatenate([y, y * 0]), ldh=p | 1))
        gr.append(R.gather(c, x, -1.0, y))
        rc = residual(rng, d)
        rc_cases.append(case(c, [np.concatenate([rc, [0.0]])], n_out=p, ldh=p | 1))
        rr.append((R.gradient(c, rc), R.lite_gradient_bound(c, rc, c["chn8"])))
    worst = 0.0
    for c, o, (ref, bound) in zip(cones, run("lite_gather", "solo", True, gc), gr):
        assert o["outi"][0] == 1, "lite_build refused the cone"
        # (all eight slots of a column are added, dummies included: 9 adds, within n + c for every column count)
        rt = ratio(o["out"], ref, bound)
        assert rt <= 1.0, (c["d"], c["p"], rt)
        worst = max(worst, rt)
    record("lite_gather", worst)
    worst = vs_row = 0.0
    for c, o, ((g, rowb, _), bound) in zip(cones, run("lite_grad", "solo", True, rc_cases), rr):
        assert o["outi"][0] == 1, "lite_build refused the cone"
        rt = ratio(o["out"], g, bound)
        assert rt <= 1.0, (c["d"], c["p"], rt)
        worst = max(worst, rt)
        err = np.abs(o["out"] - R._f64(g))
        vs_row = max(vs_row, float((err[rowb > 0] / rowb[rowb > 0]).max(initial=0.0)))
    record("lite_gradient", worst)
    record("lite_gradient_vs_rowwise_bound", vs_row)


def check_lite_hessian(run):
    """a sequence of calls with changing r and mu on the same H / wold: after every call wold is the reference's
    quantised weight (where 8 (1 + z / sqrt(1 + z^2)) + 1/2 lies within 2^-14 of an integer the adjacent level is
    accepted too; at most 1 % of the coordinates may), H the exact M diag(wold) M^T on the lower triangle, the strict
    upper triangle untouched"""
    rng = np.random.default_rng(82)
    cones = lite_cones(6)
    mus = (0.5, 0.11, 0.0, 0.3, 1e-3)
    cases, rs = [], []
    for c in cones:
        d, p = c["d"], c["p"]
        r = np.stack([rng.uniform(-4, 4, d) * (mu if mu > 0 else 1.0) for mu in mus])
        r[:, 0], r[0, 1], r[0, 2] = 0.0, 4.0 * mus[0], -4.0 * mus[0]   # z = 0, |z| = 4 exactly
        c = dict(c, usign=np.where(np.arange(d) < 3, 2, c["usign"]).astype(np.uint8))
        cases.append(case(c, [r.ravel(), mus], n_out=len(mus) * (p * (p | 1) + d), ldh=p | 1, n_seq=len(mus)))
        rs.append((c, r))
    window = total = 0
    for (c, r), o in zip(rs, run("lite_hess", "solo", True, cases)):
        assert o["outi"][0] == 1, "lite_build refused the cone"
        d, p, ldh = c["d"], c["p"], c["p"] | 1
        blk = o["out"].reshape(len(mus), p * ldh + d)
        for s, mu in enumerate(mus):
            lev, dist = R.lite_weight(c["usign"], r[s], mu)
            w16 = blk[s, p * ldh:] * 16.0
            near = dist < 2.0 ** -14
            assert np.array_equal(w16[~near], lev[~near]), (c["d"], s, mu)
            assert (np.abs(w16[near] - lev[near]) <= 1.0).all()
            if s == 0:
                assert w16[0] == 8.0  # z = 0: exactly 1/2
            window += int(near.sum())
            total += d
            H = blk[s, :p * ldh].reshape(p, ldh)[:, :p]
            ref = R._f64(R.hessian(c, np.where(w16 > 0, w16 / 16.0, 0.0))[0])
            low = np.tril(np.ones((p, p), bool))
            assert np.array_equal(H[low], ref[low]), (c["d"], s, mu)
            assert np.isnan(blk[s, :p * ldh].reshape(p, ldh)[np.triu(np.ones((p, ldh), bool), 1)]).all(), "upper triangle written"
    assert window <= 0.01 * total, (window, total)
    record("lite_weight_window_share", window / total / 0.01)


def check_lite_hessian_ipm(run):
    rng = np.random.default_rng(83)
    cones = lite_cones(7)
    cases, ws = [], []
    for i, c in enumerate(cones):
        d, p = c["d"], c["p"]
        w = sixteenths(rng, d).astype(np.float32) if i % 2 == 0 else rng.random(d).astype(np.float32)
        cases.append(case(c, n_out=p * (p | 1), ldh=p | 1, fin=np.concatenate([w, w * 0])))
        ws.append(w)
    worst = 0.0
    for i, (c, w, o) in enumerate(zip(cones, ws, run("lite_hess_ipm", "solo", True, cases))):
        assert o["outi"][0] == 1
        p, ldh = c["p"], c["p"] | 1
        H = o["out"].reshape(p, ldh)
        wd = np.where(w > 0, w.astype(np.float64), 0.0)
        Hr, n, mx = R.hessian(c, wd)
        low = np.tril(np.ones((p, p), bool))
        if i % 2 == 0:
            assert np.array_equal(H[:, :p][low], R._f64(Hr)[low])
        rt = ratio(H[:, :p][low], Hr[low], (n * R.U * n * mx)[low])  # n adds of terms <= mx, each relative to a sum <= n mx
        assert rt <= 1.0, (c["d"], rt)
        assert (H[np.triu(np.ones((p, ldh), bool), 1)] == 0.0).all()  # zeroed, never added to
        worst = max(worst, rt)
    record("lite_hessian_ipm", worst)
