"""Cases and checks of the model-step conformance suite (TEST INFRASTRUCTURE), shared by the CPU tier
(tests/test_model_emul.py: the SIMT emulation builds) and the GPU tier (tests/test_gpu_model.py: tests/prims/_prims.so).

A tier supplies `run(kind, H, theta, g, nF, reg_rel=, ord_=, seed=) -> dict(tc, moved, sact, ss, M)` over a batch of
one shape (emul_lib.model_run_host is the contract).  The systems, the extended-precision reference (model_ref.py),
the bound and the recorded margins are here and the same for every tier.  Cases are seeded and generated when a test
runs; nothing is stored.

What is asserted per case (B = (r + 1) p eps kappa_2 max(|theta|, |tc_ref|), r the reference's blocked rounds):
  1. same path, where the reference's decision margin exceeds 4 B / scale: the held set, `moved`, |tc - tc_ref| <= B;
  2. contracts, always, bitwise: held rows +0.0, bound rows >= 0, moved == any(tc != theta), no poison / NaN,
     lite: strict upper triangle of H untouched, dense: sact agrees with the zeros of tc;
  3. the face: with the kernel's own held set the form's end point, recomputed in extended precision, equals tc within
     B taken with r = nI (lite: the minimiser of the attempt's K over the face; dense: w + ss from the kernel's own
     working point w = tc - ss of the last round, w >= 0 -- see model_ref.py for why the dense form needs w);
  4. descent: m(tc) <= m(theta) for the form's regularised model, evaluated in extended precision.
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np

import linsys_cases as LC
import linsys_ref as L
import model_ref as MR

KAPPA_MAX = 1e6
FAMILIES = ("pm1", "gauss", "scaled")
SEEDS_PER_FAMILY = 3            # 9 systems per launch

LITE_SHAPES = ((1, 0), (1, 1), (8, 0), (9, 1), (21, 20), (26, 20), (28, 20), (32, 24), (32, 31), (24, 24))
# p > 64: the second row per lane; nF off the four-pivot grid: dense_factor pauses inside a block; nI in {0, 1, 9, 31, 32}
DENSE_SHAPES = ((1, 0), (2, 1), (9, 1), (33, 1), (40, 31), (63, 32), (64, 32), (65, 40), (66, 65), (128, 96), (128, 128),
                (127, 100))
DENSE_KINDS = ("dense_model_w1", "dense_model_w2", "dense_model_w4")
LIMIT_SHAPES = {"lite": ((28, 20), (32, 24), (8, 0), (24, 24)), "dense": ((33, 1), (128, 96), (128, 128), (1, 0))}
CONSTRUCTED_SHAPE = {"lite": (14, 8), "dense": (70, 60)}

EPS = {"lite": L.EPS_ONE_NEWTON, "dense": L.EPS_FULL}   # gj_partial: one Newton step on v_rcp_f64
EPS_RCP24 = {"lite": 2.0 ** -45, "dense": L.EPS_FULL}   # the SIMT_APPROX_RCP build, as test_linsys_emul.py holds it

MARGINS: dict = {}
UNDECIDED: dict = {}


def record(entry, ratio):
    MARGINS[entry] = max(MARGINS.get(entry, 0.0), float(ratio))


def dump_margins(tier, default=None, prefix=""):
    """as linsys_cases.dump_margins, into the file CAVE_MODEL_MARGINS names (the GPU tier: profiles/model_step_margins.json);
    prefix: the entries recorded under it are this tier's (written without it), the others belong to another tier"""
    path = os.environ.get("CAVE_MODEL_MARGINS", default)
    mine = {k[len(prefix):]: v for k, v in MARGINS.items() if (k.startswith(prefix) if prefix else not k.startswith("rcp24:"))}
    if not path or not mine:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[tier] = {k: float("%.3g" % v) for k, v in sorted(mine.items())}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


# ---- inputs
def draw_H(seed, family, p, reg_rel):
    """H of the family with kappa_2(H + reg_rel max diag I) <= 1e6; 'scaled' here: a gauss draw with rows and columns
    scaled symmetrically by e^u, u in [-1.5, 1.5] (the linear-solver suite's e^+-3 rows at kappa 1e8 leave 3.5 % of the
    cases undecided)"""
    for k in range(400):
        s = seed + 104729 * k
        H = L.draw_spd(s, "gauss" if family == "scaled" else family, p, reg_rel)
        if family == "scaled":
            dsc = np.exp(np.random.default_rng(s + 1).uniform(-1.5, 1.5, p))
            H = H * dsc[:, None] * dsc[None, :]
            H = 0.5 * (H + H.T)
        ev = np.linalg.eigvalsh(H + reg_rel * max(H.diagonal().max(), 0.0) * np.eye(p))
        if ev[0] > 0 and ev[-1] / ev[0] <= KAPPA_MAX:
            return H
    raise AssertionError("no draw with kappa <= 1e6")


def draw_case(seed, family, p, nF, reg_rel):
    H = draw_H(seed, family, p, reg_rel)
    rng = np.random.default_rng(seed + 7)
    nI = p - nF
    theta = rng.standard_normal(p)
    thI = rng.uniform(0.1, 2.0, nI)
    thI[rng.random(nI) >= 0.6] = 0.0
    theta[nF:] = thI
    g = rng.standard_normal(p) * 2.0 * float(np.sqrt(H.diagonal()).mean())
    return H, theta, g


def seeded_ord(p, nF, seed):
    """a permutation that interleaves free and bound rows in row order: ord[q] = reduced row at elimination position q"""
    rng = np.random.default_rng(seed)
    rows = rng.permutation(p)
    return np.concatenate([np.sort(rows[:nF]), np.sort(rows[nF:])]).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def random_group(form, p, nF, gi=0):
    """9 random systems of one shape (three per family) with their references; one reg_rel per group"""
    reg_rel = LC.reg_of(p, gi + nF)
    ref_fn = MR.lite if form == "lite" else MR.dense
    out = []
    for fi, fam in enumerate(FAMILIES):
        for k in range(SEEDS_PER_FAMILY):
            seed = 49979687 + 7919 * p + 131 * nF + 31 * (3 * fi + k) + 1000003 * gi + (0 if form == "lite" else 17)
            H, theta, g = draw_case(seed, fam, p, nF, reg_rel)
            out.append({"name": f"{fam}{k}", "H": H, "theta": theta, "g": g, "ref": ref_fn(H, theta, g, nF, reg_rel)})
    return reg_rel, out


def _blockdiag_bound(H, nF, HII):
    """H with its bound block replaced by HII and decoupled from the free rows"""
    H = H.copy()
    H[:nF, nF:] = 0.0
    H[nF:, :nF] = 0.0
    H[nF:, nF:] = HII
    return H


@functools.lru_cache(maxsize=None)
def constructed_group(form, reg_rel):
    """the constructed cases of one form that run at this reg_rel (0: the exactly-zero rows) -> list of case dicts with
    `expect`: what the reference itself must show (checked when the group is built)"""
    p, nF = CONSTRUCTED_SHAPE[form]
    nI = p - nF
    ref_fn = MR.lite if form == "lite" else MR.dense
    rng = np.random.default_rng(20240611 + p)
    base = draw_H(991 + p, "gauss", p, reg_rel)
    th0 = rng.standard_normal(p)
    out = []

    def add(name, H, theta, g, **expect):
        ref = ref_fn(H, theta, g, nF, reg_rel)
        for k, v in expect.items():
            got = ref[k] if k != "held_all" else bool(ref["held"].all())
            assert np.array_equal(got, v), (form, name, k, got, v)
        out.append({"name": name, "H": H, "theta": theta, "g": g, "ref": ref, "expect": expect})

    if reg_rel != 0.0:
        # (a) nothing moves: g_F = 0, every bound row at 0 with g >= 0, one of them exactly 0
        theta = th0.copy(); theta[nF:] = 0.0
        g = np.zeros(p); g[nF:] = rng.uniform(0.5, 2.0, nI); g[nF + 2] = 0.0
        add("a_nothing_moves", base, theta, g, moved=False, rounds=0)
        # (b) every bound row ends held, one per round: decoupled bound rows, distinct ratios theta h / g
        hI = rng.uniform(1.0, 3.0, nI)
        H = _blockdiag_bound(base, nF, np.diag(hI))
        theta = th0.copy(); theta[nF:] = rng.uniform(0.5, 1.5, nI)
        g = rng.standard_normal(p)
        g[nF:] = theta[nF:] * hI / np.linspace(0.15, 0.85, nI)   # ratio_i = 0.15 .. 0.85
        add("b_all_held", H, theta, g, rounds=nI, held_all=True)
        # (c) exact tie by symmetry: two identical, mutually decoupled blocks with identical theta and g
        m = nI // 2
        Bk = draw_H(577, "gauss", m, reg_rel)
        HII = np.zeros((nI, nI)); HII[:m, :m] = Bk; HII[m:2 * m, m:2 * m] = Bk
        for i in range(2 * m, nI):
            HII[i, i] = 1.0
        H = _blockdiag_bound(base, nF, HII)
        theta = th0.copy(); theta[nF:] = 1.0
        thb = rng.uniform(0.2, 1.0, m); theta[nF:nF + m] = thb; theta[nF + m:nF + 2 * m] = thb
        g = rng.standard_normal(p)
        gb = np.abs(rng.standard_normal(m)) * 3.0 * np.sqrt(Bk.diagonal()); g[nF:nF + m] = gb; g[nF + m:nF + 2 * m] = gb
        g[nF + 2 * m:] = -0.1
        add("c_twins", H, theta, g)
        assert out[-1]["ref"]["rounds"] >= 1 and out[-1]["ref"]["held"][:m].any()
        # (d) theta > 0 never blocked next to theta = 0, g < 0 whose step is negative: a round with a = 0
        HII = np.eye(nI); HII[0, 1] = HII[1, 0] = 0.9
        H = _blockdiag_bound(base, nF, HII)
        theta = th0.copy(); theta[nF:] = 1.0; theta[nF + 1] = 0.0
        g = rng.standard_normal(p); g[nF:] = -0.25; g[nF] = -1.0; g[nF + 1] = -0.1
        held = np.zeros(nI, bool); held[1] = True
        add("d_zero_step", H, theta, g, rounds=1, held=held)
        # (h) a row at the bound whose gradient is exactly 0 is HELD (release needs g < 0), although, coupled to a row that
        # moves, its free minimiser would be positive: releasing on g <= 0 moves it (case (a), where nothing else moves,
        # cannot tell the two rules apart)
        HII = np.eye(nI); HII[0, 1] = HII[1, 0] = -0.9
        H = _blockdiag_bound(base, nF, HII)
        theta = th0.copy(); theta[nF:] = 1.0; theta[nF + 1] = 0.0
        g = rng.standard_normal(p); g[nF:] = -0.25; g[nF] = -1.0; g[nF + 1] = 0.0
        add("h_zero_gradient_at_bound", H, theta, g, rounds=0, held=held)
        # (g) theta_I large with a small step: a lost -S theta_I term in the lite constant column shows
        theta = th0.copy(); theta[nF:] = 1e3
        g = rng.standard_normal(p) * 1e-2
        add("g_large_theta", base, theta, g, rounds=0)
    else:
        # (e1) an exactly-zero row and column among the bound rows with g < 0, next to rows that move: it stays at theta.
        # theta_z > 0: a frozen lane that took part in the ratio test would read its gradient as a step, block the
        # others at theta / (theta - g) and end held at 0 (at theta_z = 0 that mistake changes nothing)
        z = nF + 3
        H = base.copy(); H[z, :] = 0.0; H[:, z] = 0.0
        theta = th0.copy(); theta[nF:] = rng.uniform(0.5, 1.5, nI); theta[z] = 0.75
        g = rng.standard_normal(p); g[z] = -1.0
        add("e_zero_bound_row", H, theta, g, moved=True)
        assert out[-1]["ref"]["exempt"][3] and out[-1]["ref"]["tc"][z] == 0.75
        # (e2) ... as the only candidate: attempt 0 does not move, attempt 1 releases the same row, the function returns false
        theta = th0.copy(); theta[nF:] = 0.0
        g = np.zeros(p); g[nF:] = rng.uniform(0.5, 2.0, nI); g[z] = -1.0
        add("e_zero_row_only_candidate", H, theta, g, moved=False, attempt=1)
        # (f) an exactly-zero free row: dropped pivot in the first block, the row keeps theta
        H = base.copy(); H[1, :] = 0.0; H[:, 1] = 0.0
        theta = th0.copy(); theta[nF:] = rng.uniform(0.0, 1.0, nI)
        g = rng.standard_normal(p)
        add("f_zero_free_row", H, theta, g, moved=True)
        assert out[-1]["ref"]["dropped_free"][1] and out[-1]["ref"]["tc"][1] == theta[1]
    return out


# ---- the checks
def _poison_mask(a):
    from emul_lib import POISON_BITS
    return np.ascontiguousarray(a, np.float64).view(np.uint64) == np.uint64(POISON_BITS)


def launch(run, form, kind, p, nF, reg_rel, cases, ord_=None, seed=0, **kw):
    """one launch of a group -> the entry's outputs; tc and the inputs of every case are in elimination order after this"""
    B = len(cases)
    ordv = np.arange(p, dtype=np.uint16) if ord_ is None else np.asarray(ord_, np.uint16)
    theta = np.zeros((B, p)); g = np.zeros((B, p))
    Hs = []
    for i, c in enumerate(cases):
        theta[i, ordv] = c["theta"]
        g[i, ordv] = c["g"]
        if form == "lite":
            H = np.array(c["H"], np.float64)
            H[np.triu_indices(p, 1)] = np.nan   # LOWER: the upper triangle is never read
            Hs.append(H.ravel())
        else:
            Hs.append(L.fold_pack(c["H"]))
    o = run(kind, np.stack(Hs), theta, g, nF, reg_rel=reg_rel, ord_=np.tile(ordv, (B, 1)), seed=seed, **kw)
    o = dict(o)
    o["tc_e"] = o["tc"][:, ordv]
    o["theta_rows"] = theta
    return o


def check_group(run, form, kind, p, nF, reg_rel, cases, eps, tag, ord_=None, seed=0, **kw):
    """launches the group and asserts 1 - 4 per case -> (outputs, number of undecided cases)"""
    o = launch(run, form, kind, p, nF, reg_rel, cases, ord_, seed, **kw)
    nI = p - nF
    undecided, worst_path, worst_face, msgs = 0, 0.0, 0.0, []
    for i, c in enumerate(cases):
        ref, tc, th = c["ref"], o["tc_e"][i], c["theta"]
        what = (kind, p, nF, reg_rel, c["name"])
        # 2. contracts, bitwise
        assert np.isfinite(tc).all() and not _poison_mask(tc).any(), (what, "poison / NaN in tc", tc)
        tcI = tc[nF:]
        assert (tcI >= 0.0).all() and not np.signbit(tcI[tcI == 0.0]).any(), (what, "bound rows", tcI)
        assert o["moved"][i] in (0, 1) and bool(o["moved"][i]) == bool((tc != th).any()), (what, "moved", o["moved"][i])
        if form == "lite":
            M = o["M"][i].reshape(p, p | 1)
            up = np.triu(np.ones((p, p | 1), bool), 1)
            assert _poison_mask(M)[up].all(), (what, "the strict upper triangle of H was written")
            zeros = tcI == 0.0
            held = zeros & ~ref["exempt"]
        else:
            held = o["sact"][i][:nI].astype(bool)
            assert set(np.unique(o["sact"][i][:nI])) <= {0, 1}, (what, o["sact"][i])
            zeros = tcI == 0.0
            live = ~ref["exempt"]   # (a dropped row keeps theta, which may be 0, with its flag clear)
            assert (tcI[held] == 0.0).all() and np.array_equal(zeros[live], held[live]), (what, "sact against the zeros of tc", zeros, held)
        # 1. same path
        brel = MR.bound_rel(ref, eps)
        B = MR.bound(ref, eps)
        err = float(np.abs(tc - ref["tc"]).max(initial=0.0))
        if ref["margin"] > 4.0 * brel:
            ref_zero = ref["tc"][nF:] == 0.0
            assert np.array_equal(zeros, ref_zero), (what, "held set", zeros, ref_zero)
            if form == "dense":
                assert np.array_equal(held, ref["held"]), (what, "sact", held, ref["held"])
            assert bool(o["moved"][i]) == ref["moved"], (what, "moved", o["moved"][i], ref["moved"])
            r = 0.0 if err == 0.0 else (np.inf if B == 0.0 else err / B)
            worst_path = max(worst_path, r)
            if not r <= 1.0:
                msgs.append((c["name"], "path", r, ref["kappa"], ref["rounds"]))
        else:
            undecided += 1
        # 3. the face the kernel ended on
        if form == "lite":
            want, exempt = MR.face_point(ref, held)
        else:
            ss = o["ss"][i][:nI]
            w = L._num(tcI) - L._num(np.where(held, 0.0, ss))
            Bn = MR.bound(ref, eps, rounds=nI)
            assert np.isfinite(ss).all() and all(float(v) >= -Bn for v in w), (what, "working point of the last round", w)
            want, exempt = MR.face_point(ref, held, w=w)
        Bf = MR.bound(ref, eps, rounds=nI)
        cmp_rows = np.ones(p, bool)
        cmp_rows[nF:] = ~exempt
        ferr = float(np.abs(tc - want)[cmp_rows].max(initial=0.0))
        rf = 0.0 if ferr == 0.0 else (np.inf if Bf == 0.0 else ferr / Bf)
        worst_face = max(worst_face, rf)
        if not rf <= 1.0:
            msgs.append((c["name"], "face", rf, ref["kappa"], int(held.sum())))
        # 4. descent
        mv, _ = MR.model_value(ref, tc)
        assert mv <= 0.0, (what, "m(tc) > m(theta)", mv)
        # what the constructed case is about
        ex = c.get("expect", {})
        if "moved" in ex and not ex["moved"]:
            assert o["moved"][i] == 0 and np.array_equal(tc.view(np.uint64), th.view(np.uint64)), (what, "tc is not theta bitwise")
        if c["name"] == "c_twins":
            m = nI // 2
            a, b = tcI[:m], tcI[m:2 * m]
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, "twins differ", a, b)
        if c["name"] == "e_zero_bound_row":
            assert tc[nF + 3] == th[nF + 3]
        if c["name"] == "f_zero_free_row":
            assert tc[1] == th[1]
    record(tag + ":path", worst_path)
    record(tag + ":face", worst_face)
    UNDECIDED[(tag, p, nF, reg_rel, len(cases))] = undecided
    print(f"{kind} p={p} nF={nF} reg={reg_rel:g} seed={seed}: worst error/bound path {worst_path:.3g} face {worst_face:.3g}, "
          f"undecided {undecided}/{len(cases)}")
    assert not msgs, (kind, p, nF, reg_rel, msgs)
    return o, undecided


def shapes(form):
    return LITE_SHAPES if form == "lite" else DENSE_SHAPES


def undecided_in_reference(form, eps):
    """how many random cases of a form the reference alone leaves undecided: (total, cases, worst per group)"""
    tot = n = worst = 0
    for p, nF in shapes(form):
        for gi in ((0,) if form == "lite" else (0, 1)):
            _, cases = random_group(form, p, nF, gi)
            u = sum(1 for c in cases if not c["ref"]["margin"] > 4.0 * MR.bound_rel(c["ref"], eps))
            tot, n, worst = tot + u, n + len(cases), max(worst, u)
    return tot, n, worst
