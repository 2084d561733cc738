"""Cases and checks of the solver-level conformance suite (TEST INFRASTRUCTURE), shared by the CPU tier
(tests/test_linsys_emul.py: the SIMT emulation) and the GPU tier (tests/test_gpu_linsys.py: tests/prims/_prims.so).

A tier supplies `run(kind, H, rhs, act=, reg_rel=, nF=, bw=, ex=, x_in=, seed=) -> dict(x, M, aux, fail)` over a
batch of systems of one shape (emul_lib.prim_run_host is the contract); everything else -- the systems, the
extended-precision reference (linsys_ref.py), the bound, the margins that are recorded -- is here and is the same
for both.  Cases are seeded and generated when a test runs; nothing is stored.
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np

import linsys_ref as L

REGS = (0.0, 1e-12, 1e-6)
ACTS = ("none", "random20", "first_last", "run", "all_but_one")

# every dispatch threshold of wave_prims.h and its neighbours
SIZES_REG = (1, 2, 7, 8, 9, 16, 17, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 32, 33, 40, 41, 48, 49, 56, 57, 63, 64)
SIZES_DENSE = (1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128)
BANDWIDTHS = (1, 2, 3, 4, 12, 13, 33, 34)

REG_KINDS = ("gj", "gj_lower", "gjs", "gjs_tri", "spd_b2", "spd_b4", "spd_l2", "spd_l4", "spd_solo", "tri_l4", "tri_b4",
             "tri_b2")
KIND_PMAX = {"spd_b4": 32, "tri_b4": 32, "spd_solo": 8}
# one Newton step on v_rcp_f64 (gj_solve_regs, gj_partial_regs): 2^-47; two steps / rcp_full: 2^-52
ONE_NEWTON = {"gj", "gj_lower", "spd_l4", "tri_l4", "spd_solo", "partial"}
BAND_WAVE_KINDS = ("bandw1", "bandw2")
BAND_TEAM_KINDS = ("band_hot_w1", "band_hot_l2", "band_hot_l4", "band_cold_l4")


def eps_of(kind, eps_one=None):
    return (eps_one or L.EPS_ONE_NEWTON) if kind in ONE_NEWTON else L.EPS_FULL


def reg_sizes(kind):
    return tuple(p for p in SIZES_REG if p <= KIND_PMAX.get(kind, 64))


def dense_nF(p):
    """0, 1, p and values that are not multiples of 4 (the four-pivot block straddles the free / bound boundary);
    at most kDenseMaxBound = 32 bound rows"""
    c = {p, p - 1, p - 2, p - 3, p - 5, p - 7, p - 32, p - 31, 0, 1}
    return tuple(sorted(n for n in c if 0 <= n <= p and p - n <= 32))


def partial_nF(p):
    c = {p, p - 1, p - 2, p - 3, p - 5, p - 8, p // 2, 0, 1}
    return tuple(sorted(n for n in c if 0 <= n <= p))


def band_sizes(bw, full=True):
    c = (bw + 2, 63, 64, 65, 95, 96, 97, 127, 129, 300) if full else (bw + 2, 65, 300)
    return tuple(sorted({p for p in c if p >= bw + 2}))


# ---- margins: worst error / bound per entry, written when a run ends: the GPU tier into profiles/linsys_margins.json, the
# CPU tier only where the environment variable CAVE_LINSYS_MARGINS names a JSON file (it also redirects the GPU tier)
MARGINS: dict = {}


def record(entry, ratio):
    MARGINS[entry] = max(MARGINS.get(entry, 0.0), float(ratio))


def dump_margins(tier, default=None):
    path = os.environ.get("CAVE_LINSYS_MARGINS", default)
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


def _ratio(got, ref, p, eps, kappa):
    """max |got - ref| over the bound p eps kappa max |ref| (0 where both are empty; exact agreement at a zero scale)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return np.inf
    err = float(np.abs(got - ref).max())
    b = L.bound(p, eps, kappa, float(np.abs(ref).max()))
    return 0.0 if err == 0.0 else (np.inf if b == 0.0 else err / b)


def _layout(kind, H, bw=0):
    if "tri" in kind:
        return L.tri_pack(H)
    if kind.startswith("dense"):
        return L.fold_pack(H)
    if kind.startswith("band"):
        return L.band_pack(H, bw).ravel()
    out = np.array(H, np.float64)
    if kind in ("gj_lower", "spd_solo", "partial"):   # LOWER: the upper triangle is never read -- NaN there proves it
        out[np.triu_indices(H.shape[0], 1)] = np.nan
    return out.ravel()


# ---- full solves (register solvers, band): rows of (family x act pattern), one reg_rel per group
@functools.lru_cache(maxsize=None)
def solve_group(p, reg_rel, bw=None, n=5, zero_rows=None):
    """n systems of p rows (families and act patterns in rotation) with their references.  zero_rows: a tuple of tuples,
    the exactly-zero rows of each system (dropped pivots; no act rows then)"""
    out = []
    for i in range(n if zero_rows is None else len(zero_rows)):
        fam = L.FAMILIES[(i + p) % 3]
        seed = 7919 * p + 31 * i + 1009 * REGS.index(reg_rel) + (1000003 if bw is None else 17 * bw)
        while True:   # (draws whose masked system is above kappa 1e8 are rejected: the case count stays fixed)
            rng = np.random.default_rng(seed)
            zr = () if zero_rows is None else zero_rows[i]
            H = L.draw_spd(seed, fam, p, reg_rel, bw=bw, zero_rows=zr)
            rhs = rng.standard_normal(p)
            act = L.act_patterns(rng, p, bw)[ACTS[(i + p // 3) % 5]] if zero_rows is None else np.zeros(p, np.uint8)
            ref = L.solve(H, rhs, act, reg_rel)
            if ref["kappa"] <= L.KAPPA_MAX:
                break
            seed += 104729
        out.append((H, rhs, act, ref))
    return out


def check_solves(run, kind, p, reg_rel, bw=0, seed=0, zero_rows=None, tag=None, eps_one=None):
    grp = solve_group(p, reg_rel, bw or None, zero_rows=zero_rows)
    H = np.stack([_layout(kind, g[0], bw) for g in grp])
    rhs = np.stack([g[1] for g in grp])
    act = np.stack([g[2] for g in grp])
    o = run(kind, H, rhs, act=act, reg_rel=reg_rel, bw=bw, seed=seed)
    worst, msgs = 0.0, []
    for i, (_, _, a, ref) in enumerate(grp):
        if kind in BAND_WAVE_KINDS:
            assert o["fail"][i] == 0, (kind, p, bw, i, "hand-over failure word set")
        if zero_rows is not None:
            assert ref["dropped"].sum() == len(zero_rows[i]) and (o["x"][i][ref["dropped"]] == 0.0).all(), (kind, p, i, o["x"][i])
        r = _ratio(o["x"][i], ref["x"], p, eps_of(kind, eps_one), ref["kappa"])
        worst = max(worst, r)
        if not r <= 1.0:
            msgs.append((i, r, ref["kappa"]))
    record(tag or kind, worst)
    print(f"{kind} p={p} bw={bw} reg={reg_rel:g} seed={seed}: worst error/bound {worst:.3g}")
    assert not msgs, (kind, p, bw, reg_rel, msgs)


def reg_of(p, k):
    return REGS[(p + k) % 3]


ZERO_ROWS_24 = ((0,), (23,), (5,), (8, 10))   # first, last, inside a four-pivot block, two in one block
ZERO_ROWS_8 = ((0,), (7,), (5,), (4, 6))
ZERO_ROWS_40 = ((0,), (39,), (21,), (12, 14))


# ---- partial eliminations: the register form (gj_partial) and the blocked dense LDL^T
@functools.lru_cache(maxsize=None)
def partial_group(p, nF, reg_rel, zero_rows=None, n=3):
    out = []
    for i in range(n if zero_rows is None else len(zero_rows)):
        fam = L.FAMILIES[(i + p + nF) % 3]
        seed = 15485863 + 7919 * p + 131 * nF + 31 * i + REGS.index(reg_rel)
        rng = np.random.default_rng(seed)
        H = L.draw_spd(seed, fam, p, reg_rel, zero_rows=() if zero_rows is None else zero_rows[i])
        rhs = rng.standard_normal(p)
        xb = rng.standard_normal(p - nF)
        out.append((H, rhs, xb, L.partial(H, rhs, nF, reg_rel, x_bound=xb)))
    return out


def check_gj_partial(run, p, nF, reg_rel, seed=0, tag="partial", eps_one=None, zero_rows=None):
    """zero_rows: exactly-zero rows of H among the free rows (dropped pivots): their X row and xg entry are exactly
    zero, everything else is the reference's elimination without them"""
    grp = partial_group(p, nF, reg_rel, zero_rows)
    nI = p - nF
    o = run("partial", np.stack([_layout("partial", g[0]) for g in grp]), np.stack([g[1] for g in grp]), reg_rel=reg_rel,
            nF=nF, seed=seed)
    worst = {}
    for i, (_, _, _, ref) in enumerate(grp):
        XS = o["M"][i][:p * nI].reshape(p, nI)
        k, e = ref["kappa_ff"], eps_of("partial", eps_one)
        if zero_rows is not None:
            d = ref["dropped"]
            assert d.sum() == len(zero_rows[i]) and (XS[:nF][d] == 0.0).all() and (o["x"][i][:nF][d] == 0.0).all(), (p, nF, i)
        for name, got, want in (("X", XS[:nF], ref["X"]), ("S", XS[nF:], ref["S"]), ("xg", o["x"][i][:nF], ref["xg"]),
                                ("rI", o["x"][i][nF:], ref["rI"])):
            worst[name] = max(worst.get(name, 0.0), _ratio(got, want, p, e, k))
    for name, r in worst.items():
        record(tag + ":" + name, r)
    print(f"gj_partial p={p} nF={nF} reg={reg_rel:g}: worst error/bound {worst}")
    assert all(r <= 1.0 for r in worst.values()), (p, nF, reg_rel, worst)


def check_dense(run, kind, p, nF, reg_rel, seed=0, zero_rows=None, tag=None):
    """dense_factor (npiv = nF) then dense_backsub: factor rows, dinv, reduced z, Schur block, x.  With dropped pivots
    only x is compared (x_k = 0, the rest the reference's reduced solve)."""
    grp = partial_group(p, nF, reg_rel, zero_rows)
    x_in = np.full((len(grp), p), np.nan)
    for i, g in enumerate(grp):
        x_in[i, nF:] = g[2]
    o = run(kind, np.stack([_layout(kind, g[0]) for g in grp]), np.stack([g[1] for g in grp]), reg_rel=reg_rel, nF=nF,
            x_in=x_in, seed=seed)
    worst = {}
    for i, (_, _, xb, ref) in enumerate(grp):
        k, e = ref["kappa_ff"], L.EPS_FULL
        assert np.array_equal(o["x"][i][nF:], xb)   # the given part is not touched
        # x: the solution of the masked system (rows nF .. p-1 identity rows): ITS kappa_2 and norm, as for every solve
        xerr = float(np.abs(o["x"][i][:nF] - ref["xF"]).max(initial=0.0)) if np.isfinite(o["x"][i][:nF]).all() else np.inf
        xb_ = L.bound(p, e, ref["kappa_masked"], ref["x_scale"])
        worst["x"] = max(worst.get("x", 0.0), 0.0 if xerr == 0.0 else (xerr / xb_ if xb_ > 0 else np.inf))
        parts = []
        if zero_rows is None:
            A = L.fold_unpack(o["M"][i], p)
            dinv, z = o["aux"][i][:p], o["aux"][i][p:]
            parts += [("U", np.triu(A[:nF]), ref["U"]), ("S", np.triu(A[nF:, nF:]), np.triu(ref["S"])),
                      ("dinv", dinv[:nF], ref["dinv"]), ("zF", z[:nF], ref["zF"]), ("rI", z[nF:], ref["rI"])]
        else:
            assert (o["x"][i][:nF][ref["dropped"]] == 0.0).all() and ref["dropped"].sum() == len(zero_rows[i])
        for name, got, want in parts:
            worst[name] = max(worst.get(name, 0.0), _ratio(got, want, p, e, k))
    for name, r in worst.items():
        record((tag or kind) + ":" + name, r)
    print(f"{kind} p={p} nF={nF} reg={reg_rel:g} seed={seed}: worst error/bound {worst}")
    assert all(r <= 1.0 for r in worst.values()), (kind, p, nF, reg_rel, worst)
    return o


# ---- Jordan exchanges on the 8-row tableau of the lite solver's active-set loop
EXCHANGES = ((0, 1, 2, 3, 4, 5, 6, 7), (3,), (7, 0), (1, 4, 6, 4), (0, 2, 4, 6, 2, 6, 7, 0), (5, 5), (2, 3, 1, 0))


@functools.lru_cache(maxsize=None)
def tableau_group(nI, zero_row=None):
    out = []
    for i in range(3):
        seed = 32452843 + 97 * nI + i
        rng = np.random.default_rng(seed)
        S = np.eye(8)
        S[:nI, :nI] = L.draw_spd(seed, L.FAMILIES[i], nI, REGS[i])
        S[:nI, :nI] += REGS[i] * S[:nI, :nI].diagonal().max() * np.eye(nI)
        c = np.zeros(8)
        c[:nI] = rng.standard_normal(nI)
        if zero_row is not None:
            S[zero_row, :] = 0.0
            S[:, zero_row] = 0.0
        out.append(np.hstack([S, c[:, None]]))
    return out


def check_tableau(run, seq, nI, seed=0, zero_row=None, tag="tableau"):
    grp = tableau_group(nI, zero_row)
    o = run("tableau", np.stack([T.ravel() for T in grp]), np.zeros((len(grp), 8)), ex=seq, seed=seed)
    worst = 0.0
    for i, T in enumerate(grp):
        want, refused = L.exchange(T, seq)
        assert o["fail"][i] == refused, (seq, nI, i, o["fail"][i], refused)
        live = [j for j in range(8) if j != zero_row]
        kappa = float(np.linalg.cond(T[np.ix_(live, live)]))
        worst = max(worst, _ratio(o["M"][i].reshape(8, 9), want, 8, L.EPS_FULL, kappa))
    record(tag, worst)
    print(f"tableau_exchange seq={seq} nI={nI}: worst error/bound {worst:.3g}")
    assert worst <= 1.0, (seq, nI, worst)
