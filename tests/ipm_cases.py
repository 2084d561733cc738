"""Inputs of the interior-point iterate's tests, and the bound they assert (TEST INFRASTRUCTURE; numpy only, seeded).

Both tiers -- tests/test_ipm_iterate_emul.py and tests/test_gpu_ipm_iterate.py -- run the entry points of
CAVE_MODE_INNER_IPM on the families below and hold every float output to the extended-precision restatement of
tests/ipm_ref.py.  Nothing is compared with another kernel.

A family is a batch [B, m, d]: each of its cones appears five times in a row, with the predictions
    Gaussian g,  a point inside the cone,  exactly zero,  g * 2^-20,  g * 2^10
(rows 5 i .. 5 i + 4 belong to cone i; the kernels get pred = -y and sign = -1, as the fixtures are used everywhere).

  tsp20 / sp5        structured.npz [:4]: 2 - 5 bound rows (the 0.995 branch) / no bound row (the 0.2 tau branch)
  generic / setup    generic.npz [:4]: Gaussian rows (PM1 = false); only the general kernels take them
  limit cones        limit_cones.IN_CASES named in step_ipm_cases.LIMIT_NAMES: d = 256 / 255 / 193, 32 rows, 8 bound rows
  built              constructed cones, d = 40: see _built
  sp12 / tsp30 / band4   the large path, B = 2 with Gaussian predictions: 144 free rows in a band, dense LDL^T with bound
                     rows, 70 bound rows of half bandwidth 4 (the other four kinds of prediction reach that path
                     through the small families, which the tests force onto it)

The bound (E): for step count k and quantity q,  E_k = 8 S_k + F_k, S_k the spread of eight double twins of the
reference on that very input, F_k the fixed-point Hessian's bound pushed through the reference's steps (multi-wave
general kernels only).  A float output is held to 2^-24 |ref| + E_k (+ the epilogue's own bound, ipm_ref.output_bounds).
A case whose E_k exceeds TOL * sc / 4 (sc = max(1, |y|_inf), TOL = 2e-6 of golden_cases) is ill conditioned and is left
out; the cap on how many may be is asserted from the reference alone (test_ipm_iterate_emul.py).
"""

import functools
import os

import numpy as np

import ipm_ref as I
import limit_cones as LC
from golden_cases import TOL
from step_ipm_cases import LIMIT_NAMES

SIGN = -1.0
MODE_IPM = 5
K_STEPS = (1, 2, 3, 6)
K_MAX = 6
K_FLOOR = 24
# (c): the Gaussian predictions of tsp20[:2] and generic[:2], and two predictions inside their cones (rows 5 i + 1), on
# which a wrong floor shows: every coordinate with a unit row has s = 0 there and rho = -+sqrt(tau)
FLOOR_ROWS = {"tsp20": (0, 5, 1), "generic": (0, 5), "sp5": (1,)}
KINDS = ("gauss", "inside", "zero", "small", "big")
FIELDS = ("proj", "rnorm", "target", "loss", "grad")
COMPARED = ("proj", "rnorm", "theta_b", "z_b", "mtheta")   # the quantities of ipm_ref.QUANT that a test compares (f: via rnorm)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def five(A, g, seed):
    """the five predictions y of one cone A [m, d] from its Gaussian one g -> [5, d] float32 (y, i.e. sign * pred)"""
    rng = np.random.default_rng([seed, 5])
    g = np.asarray(g, np.float32)
    m = A.shape[0]
    lam = (rng.random(m) * (rng.random(m) < 0.5)).astype(np.float32)
    return np.stack([g, (lam @ A).astype(np.float32), np.zeros_like(g), g * np.float32(2.0 ** -20), g * np.float32(2.0 ** 10)])


def _family(cones, gauss, seed):
    """cones [n, m, d], gauss [n, d] (y) -> dict(ctrs [5 n, m, d], y [5 n, d], pred = SIGN * y, cone_of [5 n], kind [5 n])"""
    ctrs = np.repeat(np.asarray(cones, np.float32), 5, axis=0)
    y = np.concatenate([five(A, g, seed + i) for i, (A, g) in enumerate(zip(cones, gauss))]).astype(np.float32)
    return {"ctrs": np.ascontiguousarray(ctrs), "y": y, "pred": (np.float32(SIGN) * y).astype(np.float32),
            "cone_of": np.repeat(np.arange(len(cones)), 5), "kind": np.tile(np.arange(5), len(cones))}


# ------------------------------------------------------------------------------------------------- constructed cones
D_BUILT, M_BUILT = 40, 48


def _rows(seed, n, nnz):
    return LC.draw_rows(np.random.default_rng([seed, 40]), D_BUILT, n, nnz, 8)


def _units(signs):
    """signs: {k: '+', '-' or '+-'} -> unit rows"""
    out = []
    for k, s in sorted(signs.items()):
        for ch in s:
            e = np.zeros(D_BUILT, np.float32)
            e[k] = 1.0 if ch == "+" else -1.0
            out.append(e)
    return np.stack(out) if out else np.zeros((0, D_BUILT), np.float32)


def _block(*parts):
    blk = np.concatenate([np.asarray(p, np.float32).reshape(-1, D_BUILT) for p in parts], axis=0)
    A = np.zeros((M_BUILT, D_BUILT), np.float32)
    assert len(blk) <= M_BUILT
    A[:len(blk)] = blk
    return A


def _built():
    """name -> cone [48, 40]; the reduced rows stand [free | bound], at most 8 bound rows, +-1 entries: every form takes
    them.  What each is for stands beside it."""
    every_other = {k: ("+" if k % 4 == 0 else "-") for k in range(0, D_BUILT, 2)}
    r = _rows(1, 6, 60)
    out = {
        # p = 0: no step, the result is the smoothing of y at tau0
        "unit_only": _block(_units(every_other)),
        # usign = 3 on coordinates 3 and 8 (rho = rho' = 0 there), beside bound rows
        "both_signs": _block(r[:4], _units({3: "+-", 8: "+-", 11: "+", 20: "-", 33: "+"})),
        # unit rows of one sign only (the u = 1 branch alone)
        "one_sign": _block(r[:3], _units({k: "+" for k in range(0, D_BUILT, 2)})),
        # a +a / -a pair (one free row) beside inequality rows
        "pair_and_ineq": _block(r[4:6], -r[4:6], r[:3], _units(every_other)),
        # a duplicated inequality row: two multipliers share one column of M^T, only the barrier terms separate them
        "dup_row": _block(r[0], r[0], r[1], r[2], _units(every_other)),
        # one bound row and nothing else (p = 1)
        "one_bound": _block(r[0]),
        # no unit row at all: rho = s and rho' = 1 on every coordinate
        "no_units": _block(r[3:5], -r[3:5], r[:3]),
    }
    # step lengths at step 1, found by a seeded search and asserted from the reference's own alpha (test_..._emul.py):
    # the primal step length binds (alpha_p < 1) / does not (alpha_p = 1)
    for name, seed in ALPHA_SEEDS.items():
        rr = _rows(seed, 5, 40)
        out[name] = _block(rr[3:5], -rr[3:5], rr[:3], _alpha_units(seed))
    # the dual step length binds and the primal does not: three bound rows and a prediction far along their sum, so
    # every multiplier has to grow by more than its own size (dz = -dtheta at step 1)
    out["alpha_d_binds"] = _block(_rows(3, 5, 40)[:3], _alpha_units(3))
    return out


def _alpha_units(seed):
    return _units({k: ("+" if (k + seed) % 3 else "-") for k in range(1, D_BUILT, 3)})


ALPHA_SEEDS = {"alpha_p_binds": 2, "alpha_p_free": 4}
ALPHA_WANT = {"alpha_p_binds": lambda ap, ad: ap < 1, "alpha_p_free": lambda ap, ad: ap == 1,
              "alpha_d_binds": lambda ap, ad: ad < 1 and ap == 1}


def _built_gauss(i, name):
    """the Gaussian prediction of a constructed cone"""
    if name in ALPHA_SEEDS:
        return np.random.default_rng([14, ALPHA_SEEDS[name]]).standard_normal(D_BUILT)
    if name == "alpha_d_binds":
        return 4 * _rows(3, 5, 40)[:3].sum(0) + 0.1 * np.random.default_rng([14, 3]).standard_normal(D_BUILT)
    return np.random.default_rng([14, 100 + i]).standard_normal(D_BUILT)


def band_cone(m=70, width=5, seed=75):
    """a cone whose reduced system is a narrow band of INEQUALITY rows (half bandwidth width - 1): dense Gaussian rows
    of `width` consecutive entries, each shifted by one (the generator of tests/test_simt_emul.py)"""
    rng = np.random.default_rng(seed)
    d = m - 1 + width
    A = np.zeros((m, d), np.float32)
    for i in range(m):
        A[i, i:i + width] = rng.standard_normal(width).astype(np.float32)
    return A, rng.standard_normal(d).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- families
SMALL = ("tsp20", "sp5", "generic", "setup", "built") + tuple("limit/" + n for n in LIMIT_NAMES)
LARGE = ("sp12", "tsp30", "band4")
PM1_ONLY = ("tsp20", "sp5", "built") + tuple("limit/" + n for n in LIMIT_NAMES)   # what the lite form takes


@functools.lru_cache(maxsize=None)
def family(name):
    if name in ("tsp20", "sp5"):
        s = np.load(os.path.join(GOLDEN, "structured.npz"))
        return _family(s[name + "_ctrs"][:4], SIGN * s[name + "_costs"][:4], 11)
    if name in ("generic", "setup"):
        g = np.load(os.path.join(GOLDEN, "generic.npz"))
        return _family(g[name + "_ctrs"][:4], SIGN * g[name + "_costs"][:4], 12)
    if name.startswith("limit/"):
        case = {c.name: c for c in LC.IN_CASES}[name[6:]]
        blk, _ = LC.cone(case, 11, 0)
        g = np.random.default_rng([13, case.d, case.p]).standard_normal(case.d)
        return _family(blk[None], g[None], 13)
    if name == "built":
        cones = _built()
        names = list(cones)
        g = np.stack([_built_gauss(i, n) for i, n in enumerate(names)])
        f = _family(np.stack([cones[n] for n in names]), g, 14)
        f["names"] = names
        return f
    if name in ("sp12", "tsp30"):
        from cave_amd import synth

        c, y, _ = synth.sp_batch(12, 12, 2, seed=5) if name == "sp12" else synth.tsp_batch(30, 2, seed=5)
        return _large_family(np.asarray(c, np.float32), SIGN * np.asarray(y, np.float32))
    if name == "band4":
        A, g = band_cone()
        A2, g2 = band_cone(seed=76)
        return _large_family(np.stack([A, A2]), np.stack([g, g2]))
    raise KeyError(name)


def _large_family(cones, gauss):
    """B = 2: two cones, each with its own Gaussian prediction (the other four kinds reach the large path through the
    small families, which the tests force onto it)"""
    y = np.asarray(gauss, np.float32)
    return {"ctrs": np.ascontiguousarray(cones, dtype=np.float32), "y": y, "pred": (np.float32(SIGN) * y).astype(np.float32),
            "cone_of": np.arange(len(cones)), "kind": np.zeros(len(cones), np.int64)}


# ---------------------------------------------------------------------------------------------- reference and bounds
@functools.lru_cache(maxsize=None)
def _cone(name, i):
    f = family(name)
    return I.reduced(f["ctrs"][int(np.flatnonzero(f["cone_of"] == i)[0])])


@functools.lru_cache(maxsize=None)
def reference(name, b, weights="f32", steps=K_MAX):
    """-> (reduced cone, states of the extended-precision run 0 .. steps)"""
    f = family(name)
    c = _cone(name, int(f["cone_of"][b]))
    return c, I.iterate(c, f["y"][b], steps, weights)


@functools.lru_cache(maxsize=None)
def spread(name, b, weights="f32", rcp=False):
    f = family(name)
    c, ref = reference(name, b, weights)
    return I.spread(ref, I.twins(c, f["y"][b], K_MAX, weights=weights, rcp=rcp))


@functools.lru_cache(maxsize=None)
def shift(name, b, weights="f32"):
    f = family(name)
    c, ref = reference(name, b, weights)
    return I.fixed_point_shift(c, f["y"][b], K_MAX, ref, weights)


def scale_of(name, b):
    return max(1.0, float(np.abs(family(name)["y"][b]).max()))


def E(name, b, k, weights="f32", fixed=False, rcp=False):
    """E_k per quantity.  rcp: the twins' reciprocals are those of a one-wave solver on the device (ipm_ref.twins)"""
    S = spread(name, b, weights, rcp)[k]
    F = shift(name, b, weights)[k] if fixed else {q: 0.0 for q in I.QUANT}
    return {q: I.TWIN_FACTOR * S[q] + F[q] for q in I.QUANT}


def capped(name, b, weights="f32", fixed=False, rcp=False):
    """is the case ill conditioned (left out of the comparisons): some E_k, k <= 6, above TOL sc / 4"""
    lim = TOL * scale_of(name, b) / 4
    return any(max(E(name, b, k, weights, fixed, rcp)[q] for q in COMPARED) > lim for k in K_STEPS)


def compare(out, name, k, weights="f32", fixed=False, what="", record=None, rows=None, rcp=False):
    """the float outputs `out` of an entry on family `name` at step count k against the reference -> worst
    error / bound.  Prints it, records it under `what`, then asserts: every instance OK, iters = k (0 without reduced
    rows), every output within its bound."""
    f = family(name)
    worst = {q: 0.0 for q in FIELDS}
    fails = []
    for b in (range(len(f["y"])) if rows is None else rows):
        c, ref = reference(name, b, weights)
        assert out["status"][b] == 0, (what, name, b, out["status"][b])
        want_it = k if (c["p"] > 0 and not c["empty"]) else 0
        assert out["iters"][b] == want_it, (what, name, b, out["iters"][b], want_it)
        if capped(name, b, weights, fixed, rcp):
            continue
        vals, bnd = I.output_bounds(c, f["y"][b], ref[k], E(name, b, k, weights, fixed, rcp), SIGN)
        for q in FIELDS:
            got = np.atleast_1d(np.asarray(out[q][b], np.float64))
            assert np.isfinite(got).all(), (what, name, b, q)
            err = np.abs(got - np.atleast_1d(I.L._f64(vals[q])))
            ratio = float((err / bnd[q]).max())
            worst[q] = max(worst[q], ratio)
            if ratio > 1.0:
                fails.append((b, q, ratio, float(err.max())))
    top = max(worst.values())
    print(f"{what} {name} k={k}: worst error / bound {top:.3f} " + " ".join(f"{q}={worst[q]:.3f}" for q in FIELDS))
    if record is not None:
        key = f"{what}|{name.split('/')[0]}|k={k}"
        record[key] = max(record.get(key, 0.0), top)
    assert not fails, (what, name, k, fails[:6])
    return top


# ---------------------------------------------------------------------------------------------- (b): the double state
STATE_KINDS = (("ipm_iter", "w1"), ("ipm_iter", "b4"), ("ipm_lite", "solo"))   # tests/prims/ipm_entries.h
STATE_STEPS = (1, 2, 3)


def state_rows(name, lite=False):
    """the rows of a family an entry takes: all, or (lite) those with at least one reduced row"""
    return [b for b in range(len(family(name)["y"])) if not lite or reference(name, b)[0]["p"] > 0]


def state_cases(name, k, rows):
    """the OpCases of rows of a family at k steps (emul_lib.op_run_host / prims_lib.Prims.op_run) -> (cases, pm1)"""
    import ops_cases as OC

    f = family(name)
    cases, pm1 = [], None
    for b in rows:
        c = reference(name, b)[0]
        assert not c["empty"] and (pm1 is None or pm1 == c["pm1"])
        pm1 = c["pm1"]
        oc = OC.make_cone(c["M"], pm1, usign=c["usign"], vkind=c["vkind"])
        d, p = c["d"], c["p"]
        cases.append(OC.case(oc, n_out=d + 2 * p + 3, fin=np.concatenate([f["y"][b], np.zeros(d, np.float32)]), ldh=p | 1, n_seq=k))
    return cases, pm1


def compare_state(outs, name, k, rows, fixed, what, record=None, lite=False, rcp=False):
    """rho (w.res), theta and z of the bound rows and M^T theta recomputed from the theta that comes back, each within E_k
    (no float32 term: these are doubles); theta of free rows is not compared (on a grid cone it is not identifiable)"""
    f = family(name)
    worst, fails = 0.0, []
    for b, o in zip(rows, outs):
        c, ref = reference(name, b)
        d, p = c["d"], c["p"]
        if lite:
            assert o["outi"][0] == 1, (what, name, b, "lite_build refused the cone")
        out = o["out"]
        rho, th, z, f_, iters, status = out[:d], out[d:d + p], out[d + p:d + 2 * p], out[d + 2 * p], out[d + 2 * p + 1], out[d + 2 * p + 2]
        assert status == 0 and iters == (k if p > 0 else 0), (what, name, b, status, iters)
        assert np.isfinite(out).all(), (what, name, b)
        if capped(name, b, "f32", fixed, rcp):
            continue
        e = E(name, b, k, "f32", fixed, rcp)
        bnd = c["vkind"] == 0
        mt = I.L._f64(np.dot(I.L._num(c["M"]).T, I.L._num(th)) - ref[k]["mtheta"]) if p else np.zeros(d)
        for q, err, lim in (("rho", I.L._f64(I.L._num(rho) - ref[k]["rho"]), e["proj"]),
                            ("theta_b", I.L._f64(I.L._num(th[bnd]) - ref[k]["theta_b"]), e["theta_b"]),
                            ("z_b", I.L._f64(I.L._num(z[bnd]) - ref[k]["z_b"]), e["z_b"]), ("mtheta", mt, e["mtheta"])):
            worst_q = float(np.abs(err).max(initial=0.0))
            if worst_q > 0.0:   # (an exact match needs no bound: E can be 0 where every twin agrees to the last bit)
                r = worst_q / lim if lim > 0 else np.inf
                worst = max(worst, r)
                if r > 1.0:
                    fails.append((b, q, r, worst_q))
    print(f"{what} {name} k={k}: double state, worst error / E_k {worst:.3f}")
    if record is not None:
        key = f"{what}|{name.split('/')[0]}|k={k}"
        record[key] = max(record.get(key, 0.0), worst)
    assert not fails, (what, name, k, fails[:6])
    return worst


RECORD: dict = {}


def write_record(tier, default=None):
    """the worst error / bound per entry, family and step count, into the JSON file CAVE_IPM_ITERATE_MARGINS names
    (tools/diag/ipm_iterate_margins.py sets it; it also redirects the GPU tier, whose default is the committed
    profiles/ipm_iterate_margins.json); without either: nothing"""
    import json

    path = os.environ.get("CAVE_IPM_ITERATE_MARGINS", default)
    if not path or not RECORD:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    for k, v in sorted(RECORD.items()):   # the SIMT_APPROX_RCP build is a tier of its own
        data.setdefault(tier + "_rcp24" if k.startswith("rcp24/") else tier, {})[k] = float("%.3g" % v)
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")
