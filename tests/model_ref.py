"""Extended-precision restatement of the model minimisation of one Newton iteration (TEST INFRASTRUCTURE, numpy only).

lite_model_step (cone_core.h) and dense_model_step (cone_dense.h) minimise the model

    m(t) = g . (t - theta) + 1/2 (t - theta)^T K (t - theta)        over  t_i >= 0 on the bound rows

by the same documented procedure -- eliminate the free rows once, run an active-set loop on the Schur complement S of
the bound rows, substitute back -- and differ in how they regularise and in how they carry the loop (a tableau of
y = S x + c in absolute coordinates against a gradient updated round by round).  This module restates the procedure
once and the regularisation per form, in the working precision of linsys_ref (long double, or mpmath numbers where
long double is too narrow), and records for every comparison on the path how far it is from flipping.

Everything is in ELIMINATION order: rows [free | bound], nF free rows first.  The caller permutes.

  * attempt 0 holds a bound row iff theta_i <= 0 and not g_i < 0; attempt 1 runs only if attempt 0 did not move and
    gmin = min(0, min g_i over the bound rows with theta_i <= 0) < 0, and releases the rows with g_i <= gmin;
  * every round minimises over the not-held rows with the held rows at 0, takes the ratio test from the working point
    st, and if amin < 1 steps by a = max(amin, 0) and holds every free row with t < 0 and
    st <= a (st - t) (1 + 1e-12); at most nI + 1 rounds;
  * free rows follow from x_F = K_FF^-1 (-g_F - K_FI (st - theta_I)).

Regularisation as the code applies it:
  lite    reg1 = reg_rel * max diag(H) on every row (gj_partial); then reg2 = reg_rel * max diag(S) over the bound
          rows not held when the attempt starts, on the tableau's diagonal.  One K per attempt: the loop's end point IS
          the minimiser of that K over the final face, whatever the path.
  dense   reg_f = reg_rel * max diag(H) on every row (dense_factor); then each round's register solve adds
          rho = reg_rel * max diag(S over the rows free in that round) to ITS matrix only -- the gradient the loop
          carries (sg += a S ss) is that of S without rho.  The end point is therefore w + ss with
          (S_ff + rho I) ss = -(S w + c)_f, w the working point of the last round: for rho > 0 it depends on the path
          at O(rho), and the face check of the dense form is stated with the kernel's own w = tc - ss.
  A pivot that is not above PIVOT_MIN is dropped (free rows: x_k = 0; dense round solve: ss_k = 0) or its exchange
  refused (lite tableau: the row is frozen at theta_i), as in linsys_ref.
"""

from __future__ import annotations

import numpy as np

import linsys_ref as L

TIE = 1e-12   # the tie rule's relative slack, as both forms write it


def _zeros(shape):
    return L._num(np.zeros(shape))


def _dot(a, b):
    """np.dot that survives empty operands of the mpmath (object) form"""
    if a.size == 0 or b.size == 0:
        out_shape = a.shape[:-1] + b.shape[1:]
        return _zeros(out_shape) if out_shape else L._num(0.0)[()]
    return np.dot(a, b)


def _f(v):
    return float(v)


def _partial(K, b, nF):
    """pivots k < nF of [K | b] with dropping: R (kept free rows), W = R^-T K_FI, yz = R^-T b_F, S, rI"""
    p = K.shape[0]
    nI = p - nF
    R, keep = L.cholesky_dropping(K[:nF, :nF]) if nF else (_zeros((0, 0)), np.zeros(0, bool))
    Fk = np.flatnonzero(keep)
    nk = len(Fk)
    S = K[nF:, nF:].copy()
    rI = b[nF:].copy()
    W, yz = _zeros((nk, nI)), _zeros(nk)
    if nk:
        yz = L._fwd(R, b[Fk])
        if nI:
            W = L._fwd(R, K[np.ix_(Fk, np.arange(nF, p))])
            S = S - _dot(W.T, W)
            rI = rI - _dot(W.T, yz)
    return {"R": R, "Fk": Fk, "W": W, "yz": yz, "S": S, "rI": rI, "dropped": ~keep}


def _free_rows(part, nF, xI):
    """x_F = K_FF^-1 (b_F - K_FI x_I) over the kept rows, 0 on the dropped ones"""
    x = _zeros(nF)
    if len(part["Fk"]):
        r = part["yz"] - _dot(part["W"], xI) if len(xI) else part["yz"]
        x[part["Fk"]] = L._bwd(part["R"], r)
    return x


def _masked_solve(S, rhs, act, reg_rel):
    """linsys_ref.solve without the rounding to float64: act rows x = rhs, free rows of S + rho I, dropped pivots 0
    -> (x, dropped mask, rho)"""
    n = S.shape[0]
    free = ~act
    F, A = np.flatnonzero(free), np.flatnonzero(act)
    md = max(max([_f(S[i, i]) for i in F], default=0.0), 0.0)
    rho = L._num(reg_rel)[()] * L._num(md)[()]
    x = _zeros(n)
    dropped = np.zeros(n, bool)
    x[A] = rhs[A]
    if len(F):
        Kf = S[np.ix_(F, F)].copy()
        for i in range(len(F)):
            Kf[i, i] = Kf[i, i] + rho
        R, keep = L.cholesky_dropping(Kf)
        Fk = F[keep]
        dropped[F[~keep]] = True
        if len(Fk):
            r = rhs[Fk].copy()
            for a in A:
                r = r - S[Fk, a] * rhs[a]
            x[Fk] = L._spd_solve(R, r)
    return x, dropped, rho


class _Margin:
    """smallest relative distance of any comparison on the path from flipping"""

    def __init__(self):
        self.v = np.inf

    def add(self, dist, scale):
        dist, scale = abs(_f(dist)), abs(_f(scale))
        if scale > 0.0 and dist > 0.0:   # an exact zero is decided in any precision (inputs compared as given, ties at a = 0)
            self.v = min(self.v, dist / scale)


def _ratio_round(st, t, cand, mg):
    """ratio test of one round over the candidate rows -> (blocked, a, fixnow mask); records the margins"""
    n = len(st)
    ratio = {}
    for i in np.flatnonzero(cand):
        mg.add(t[i], max(abs(_f(t[i])), abs(_f(st[i]))))
        if _f(t[i]) < 0.0:
            ratio[i] = st[i] / (st[i] - t[i])
    fix = np.zeros(n, bool)
    if not ratio:
        return False, L._num(1.0)[()], fix
    amin = min(ratio.values())
    mg.add(1.0 - _f(amin), 1.0)
    a = amin if _f(amin) > 0.0 else L._num(0.0)[()]
    for i in ratio:
        lhs, rhs = st[i], a * (st[i] - t[i]) * (1 + L._num(TIE)[()])
        fix[i] = bool(lhs <= rhs)
        if _f(a) > 0.0 and ratio[i] != amin:   # exact ties (twin rows) and a = 0 do not count
            mg.add(ratio[i] - a * (1 + L._num(TIE)[()]), ratio[i])
    return True, a, fix


def _kappa_live(K64):
    live = np.flatnonzero(np.abs(K64).sum(1) > 0)
    return L._kappa2(K64[np.ix_(live, live)]) if len(live) else 1.0


def _attempts(theta_I, g_I, mg, run_attempt):
    """the two attempts around one form's inner loop; run_attempt(act0, attempt) -> (tc, extra) -> (tc, extra, attempt)"""
    gmax = float(np.abs(g_I).max(initial=0.0))
    out = None
    for attempt in range(2):
        at_bound = theta_I <= 0.0
        if attempt == 0:
            for i in np.flatnonzero(at_bound):
                mg.add(g_I[i], gmax)
            release = g_I < 0.0
        else:
            gmin = min(0.0, float(g_I[at_bound].min(initial=0.0)))
            if not gmin < 0.0:
                break
            release = g_I <= gmin
        out = run_attempt(at_bound & ~release, attempt) + (attempt,)
        if out[0][1]:
            break
    return out


def _common(H, theta, g, nF, reg_rel):
    H64 = np.asarray(H, np.float64)
    p = H64.shape[0]
    md = max(float(H64.diagonal().max(initial=0.0)), 0.0)
    reg = L._num(reg_rel)[()] * L._num(md)[()]
    K = L._num(H64)
    for i in range(p):
        K[i, i] = K[i, i] + reg
    th, gg = L._num(np.asarray(theta, np.float64)), L._num(np.asarray(g, np.float64))
    return H64, p, p - nF, reg, K, th, gg, _partial(K, -gg, nF)


def _finish(form, H64, K, extraK, th, gg, nF, part, res, mg, reg_rel):
    (tcI, moved_dummy, info), attempt = res[0], res[-1]
    p, nI = H64.shape[0], H64.shape[0] - nF
    xF = _free_rows(part, nF, tcI - th[nF:])
    tc = _zeros(p)
    tc[:nF] = th[:nF] + xF
    tc[nF:] = tcI
    tc64, th64 = L._f64(tc), np.asarray(L._f64(th))
    Kd = L._f64(K)
    for i, e in enumerate(info.get("reg2_diag", [])):
        Kd[nF + i, nF + i] += e
    return {"form": form, "tc": tc64, "tc_ext": tc, "held": info["held"].copy(), "moved": bool((tc64 != th64).any()),
            "rounds": info["rounds"], "kappa": _kappa_live(Kd), "margin": mg.v, "attempt": attempt,
            "dropped_free": part["dropped"].copy(), "exempt": info["exempt"].copy(), "K64": Kd, "H64": H64, "nF": nF,
            "reg_rel": reg_rel, "reg2": (info.get("reg2_diag") or [0.0])[0],
            "w_last": L._f64(info["w_last"]), "theta": th64, "g": np.asarray(L._f64(gg))}


def lite(H, theta, g, nF, reg_rel=0.0):
    """lite_model_step restated -> dict(tc, held [nI bool], moved, rounds, kappa, margin, ...)"""
    H64, p, nI, reg1, K, th, gg, part = _common(H, theta, g, nF, reg_rel)
    S, rI = part["S"], part["rI"]
    mg = _Margin()
    th_I, g_I64 = th[nF:], np.asarray(g, np.float64)[nF:]

    def run_attempt(act0, attempt):
        free0 = np.flatnonzero(~act0)
        dmax = max(max([_f(S[i, i]) for i in free0], default=0.0), 0.0)
        reg2 = L._num(reg_rel)[()] * L._num(dmax)[()]
        T = S.copy()
        for i in range(nI):
            T[i, i] = T[i, i] + reg2
        c = -rI - _dot(T, th_I) if nI else _zeros(0)
        # exchanges in index order: a pivot that is not positive is refused and the row frozen (never retried)
        frozen = np.zeros(nI, bool)
        if len(free0):
            _, keep = L.cholesky_dropping(T[np.ix_(free0, free0)])
            frozen[free0[~keep]] = True
        act, st = act0.copy(), th_I.copy()
        rounds = 0
        w_last = st.copy()
        for _ in range(nI + 1):
            A = np.flatnonzero(~act & ~frozen)
            t = st.copy()
            t[act] = 0
            if len(A):
                R, keep = L.cholesky_dropping(T[np.ix_(A, A)])
                t[A[keep]] = L._spd_solve(R, -c[A[keep]])
            cand = ~act & ~frozen
            blocked, a, fix = _ratio_round(st, t, cand, mg)
            w_last = st.copy()
            st = st + a * (t - st) if blocked else t.copy()
            act = act | fix
            st[act] = 0
            if not blocked:
                break
            rounds += 1
        info = {"held": act, "rounds": rounds, "exempt": frozen, "reg2_diag": [_f(reg2)] * nI, "w_last": w_last}
        xF = _free_rows(part, nF, st - th_I)
        moved = bool((L._f64(st) != L._f64(th_I)).any() or (L._f64(th[:nF] + xF) != L._f64(th[:nF])).any())
        return (st, moved, info), None

    if nI == 0:
        res = ((_zeros(0), True, {"held": np.zeros(0, bool), "rounds": 0, "exempt": np.zeros(0, bool), "w_last": _zeros(0)}), None, 0)
    else:
        res = _attempts(L._f64(th_I), g_I64, mg, run_attempt)
        if res is None:   # attempt 1 not entered: nothing moved
            res = ((th_I.copy(), False, {"held": (L._f64(th_I) <= 0.0), "rounds": 0, "exempt": np.zeros(nI, bool),
                                         "w_last": th_I.copy()}), None, 0)
    return _finish("lite", H64, K, None, th, gg, nF, part, res, mg, reg_rel)


def dense(H, theta, g, nF, reg_rel=0.0):
    """dense_model_step restated (same outputs as lite; w_last: the working point of the last round)"""
    H64, p, nI, reg_f, K, th, gg, part = _common(H, theta, g, nF, reg_rel)
    S, rI = part["S"], part["rI"]
    mg = _Margin()
    th_I, g_I64 = th[nF:], np.asarray(g, np.float64)[nF:]

    def run_attempt(act0, attempt):
        act, st, sg = act0.copy(), th_I.copy(), -rI.copy()
        rounds = 0
        exempt = np.zeros(nI, bool)
        w_last = st.copy()
        for _ in range(nI + 1):
            sr = -sg.copy()
            sr[act] = -st[act]
            ss, dropped, _ = _masked_solve(S, sr, act, reg_rel)
            exempt = dropped
            t = st + ss
            blocked, a, fix = _ratio_round(st, t, ~act, mg)
            w_last = st.copy()
            if blocked:
                sg = sg + a * _dot(S, ss)
            st = st + a * ss
            act = act | fix
            st[act] = 0
            if not blocked:
                break
            rounds += 1
        info = {"held": act, "rounds": rounds, "exempt": exempt, "w_last": w_last}
        xF = _free_rows(part, nF, st - th_I)
        moved = bool((L._f64(st) != L._f64(th_I)).any() or (L._f64(th[:nF] + xF) != L._f64(th[:nF])).any())
        return (st, moved, info), None

    if nI == 0:
        res = ((_zeros(0), True, {"held": np.zeros(0, bool), "rounds": 0, "exempt": np.zeros(0, bool), "w_last": _zeros(0)}), None, 0)
    else:
        res = _attempts(L._f64(th_I), g_I64, mg, run_attempt)
        if res is None:
            res = ((th_I.copy(), False, {"held": (L._f64(th_I) <= 0.0), "rounds": 0, "exempt": np.zeros(nI, bool),
                                         "w_last": th_I.copy()}), None, 0)
    return _finish("dense", H64, K, None, th, gg, nF, part, res, mg, reg_rel)


def bound_rel(ref, eps, rounds=None):
    """(r + 1) p eps kappa_2: the project's forward bound, once per solve on the path"""
    r = ref["rounds"] if rounds is None else rounds
    return (r + 1) * len(ref["tc"]) * eps * ref["kappa"]


def bound(ref, eps, rounds=None):
    scale = max(float(np.abs(ref["theta"]).max(initial=0.0)), float(np.abs(ref["tc"]).max(initial=0.0)))
    return bound_rel(ref, eps, rounds) * scale


def face_point(ref, held, attempt=None, w=None):
    """The point the form must end at on the face {t_Z = 0}, Z = `held` (the kernel's own final flags), in extended
    precision -> (tc [p] float64, exempt [nI]).  lite: the minimiser of the attempt's K over the face.  dense: w + ss with
    (S_ff + rho I) ss = -(S w + c)_f for the working point w the kernel's last round started from (w = tc - ss_out)."""
    nF, reg_rel = ref["nF"], ref["reg_rel"]
    th, gg = L._num(ref["theta"]), L._num(ref["g"])
    p = len(ref["theta"])
    nI = p - nF
    held = np.asarray(held, bool)
    K = L._num(ref["H64"])
    md = max(float(ref["H64"].diagonal().max(initial=0.0)), 0.0)
    reg = L._num(reg_rel)[()] * L._num(md)[()]
    for i in range(p):
        K[i, i] = K[i, i] + reg
    part = _partial(K, -gg, nF)
    S, rI, th_I = part["S"], part["rI"], th[nF:]
    exempt = np.zeros(nI, bool)
    if nI == 0:
        st = _zeros(0)
    elif ref["form"] == "lite":
        T = S.copy()
        reg2 = L._num(ref["reg2"])[()]
        for i in range(nI):
            T[i, i] = T[i, i] + reg2
        c = -rI - _dot(T, th_I)
        exempt = ref["exempt"].copy()
        A = np.flatnonzero(~held & ~exempt)
        st = _zeros(nI)
        st[exempt] = th_I[exempt]
        if len(A):
            R, keep = L.cholesky_dropping(T[np.ix_(A, A)])
            sol = _zeros(len(A))
            if keep.any():
                sol[keep] = L._spd_solve(R, -c[A][keep])
            st[A] = sol
            exempt[A[~keep]] = True
    else:
        wv = w.copy()   # (working precision already: tc - ss is formed there)
        wv[held] = 0
        c = -rI - _dot(S, th_I)
        grad = _dot(S, wv) + c
        rhs = -grad
        rhs[held] = 0   # held rows: "stay at zero"
        ss, dropped, _ = _masked_solve(S, rhs, held, reg_rel)
        ss[held] = 0
        exempt = dropped
        st = wv + ss
        st[held] = 0
    xF = _free_rows(part, nF, st - th_I)
    tc = _zeros(p)
    tc[:nF] = th[:nF] + xF
    tc[nF:] = st
    return L._f64(tc), exempt


def model_value(ref, tc):
    """m(tc) - m(theta) of the form's regularised model, and the 1-norm of its gradient at tc, in extended precision"""
    K = L._num(ref["K64"])
    d = L._num(np.asarray(tc, np.float64)) - L._num(ref["theta"])
    gg = L._num(ref["g"])
    Kd = _dot(K, d)
    grad = gg + Kd
    return _f(_dot(gg, d) + _dot(d, Kd) / 2), float(sum(abs(_f(v)) for v in grad))
