"""Extended-precision reference for the linear solvers of the Newton loop (TEST INFRASTRUCTURE, numpy only).

Every solver of cave_amd/csrc (the register Gauss-Jordan forms of wave_prims.h, the blocked dense LDL^T of
cone_dense.h, the band eliminations of cone_band.h) documents the same semantics:

  * rows flagged `act` are identity rows, x = rhs;
  * free rows are rows of H + reg_rel * max diag(free) * I;
  * a free row whose pivot is not positive is dropped, x_k = 0.

This module restates them in plain code and solves in np.longdouble (64-bit mantissa on x86: eps = 1.08e-19) with a
hand-written Cholesky and substitution.  Where the platform's long double is no wider than that requirement
(eps > 2^-63) the same code runs on mpmath numbers instead: the reference never skips.

It also draws the test systems (seeded, nothing stored) and states the bound the tests assert:

    || x - x_ref ||_inf  <=  p * eps * kappa_2 * || x_ref ||_inf

the first-order forward bound eps * kappa_2 of an elimination without pivoting on an SPD system, with the factor p as
the margin; eps = 2^-47 for the forms whose reciprocal takes one Newton step, 2^-52 for the others.
"""

from __future__ import annotations

import numpy as np

EPS_ONE_NEWTON = 2.0 ** -47   # gj_solve_regs, gj_partial_regs: v_rcp_f64 + one Newton step
EPS_FULL = 2.0 ** -52         # two Newton steps / rcp_full: gj_solve_regs_small, tableau_exchange, dense, band
KAPPA_MAX = 1e8
PIVOT_MIN = 1e-300            # "not positive" as every solver tests it

FORCE_MPMATH = False          # tests flip this to run the fallback once


def _wide_enough() -> bool:
    return (not FORCE_MPMATH) and float(np.finfo(np.longdouble).eps) <= 2.0 ** -63


def _num(a):
    """array of the working precision: long double, or mpmath numbers (100 bits) where long double is too narrow"""
    if _wide_enough():
        assert np.finfo(np.longdouble).eps <= 2.0 ** -63
        return np.array(a, dtype=np.longdouble)
    import mpmath

    mpmath.mp.prec = 100
    a = np.asarray(a)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        v = a[idx]
        out[idx] = v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v))
    return out


def _sqrt(v):
    if isinstance(v, np.floating):
        return np.sqrt(v)
    import mpmath

    return mpmath.sqrt(v)


def _f64(a):
    return np.array([float(v) for v in np.asarray(a).ravel()], dtype=np.float64).reshape(np.shape(a))


def cholesky_dropping(K):
    """Upper factor R of K[keep][:, keep] = R^T R, eliminating in index order; a row whose running pivot is not
    positive is dropped (with its column), as the solvers do.  -> (R over the kept rows, keep mask)"""
    K = _num(K)
    n = K.shape[0]
    keep = np.zeros(n, bool)
    R = _num(np.zeros((n, n)))
    for k in range(n):   # (rows of R of dropped pivots stay zero: they take no part in the sums)
        row = K[k, k:] - np.dot(R[:k, k], R[:k, k:]) if k else K[k, k:].copy()
        d = row[0]
        if not (float(d) > PIVOT_MIN):
            continue
        keep[k] = True
        R[k, k:] = row / _sqrt(d)
    idx = np.flatnonzero(keep)
    return R[np.ix_(idx, idx)], keep


def _fwd(R, b):  # R^T y = b
    n = R.shape[0]
    y = _num(np.zeros(np.shape(b)))
    for i in range(n):
        s = b[i] - np.dot(R[:i, i], y[:i]) if i else b[i]
        y[i] = s / R[i, i]
    return y


def _bwd(R, y):  # R x = y
    n = R.shape[0]
    x = _num(np.zeros(np.shape(y)))
    for i in range(n - 1, -1, -1):
        s = y[i] - np.dot(R[i, i + 1:], x[i + 1:]) if i + 1 < n else y[i]
        x[i] = s / R[i, i]
    return x


def _spd_solve(R, b):
    return _bwd(R, _fwd(R, b))


def _kappa2(A):
    A = np.asarray(A, np.float64)
    if A.size == 0:
        return 1.0
    s = np.linalg.svd(A, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else np.inf


def solve(H, rhs, act=None, reg_rel=0.0):
    """x of the masked, regularised system -> dict(x [float64], kappa, kappa_ff, dropped [bool p])."""
    H64 = np.asarray(H, np.float64)
    p = H64.shape[0]
    act = np.zeros(p, bool) if act is None else np.asarray(act).astype(bool)
    free = ~act
    md = max(float(H64.diagonal()[free].max(initial=0.0)), 0.0)
    reg = _num(reg_rel) * _num(md)
    Hn, b = _num(H64), _num(np.asarray(rhs, np.float64))
    F, A = np.flatnonzero(free), np.flatnonzero(act)
    K = Hn[np.ix_(F, F)]
    for i in range(len(F)):
        K[i, i] = K[i, i] + reg
    R, keep = cholesky_dropping(K)
    Fk = F[keep]
    x = _num(np.zeros(p))
    x[A] = b[A]
    r = b[Fk]
    for a in A:
        r = r - Hn[Fk, a] * b[a]
    if len(Fk):
        x[Fk] = _spd_solve(R, r)
    # the system as the solvers see it: [[K_FF, H_FA], [0, I]] without the dropped rows / columns
    live = np.concatenate([Fk, A]).astype(int)
    Mfull = np.zeros((len(live), len(live)))
    nk = len(Fk)
    Mfull[:nk, :nk] = _f64(K[np.ix_(keep, keep)])
    Mfull[:nk, nk:] = H64[np.ix_(Fk, A)]
    Mfull[nk:, nk:] = np.eye(len(A))
    dropped = np.zeros(p, bool)
    dropped[F[~keep]] = True
    return {"x": _f64(x), "kappa": _kappa2(Mfull), "kappa_ff": _kappa2(Mfull[:nk, :nk]), "dropped": dropped}


def partial(H, rhs, nF, reg_rel=0.0, x_bound=None):
    """Elimination of the pivots k < nF of [H + reg I | rhs] (reg = reg_rel * largest diagonal entry, every row):
    X = K_FF^-1 H_FI, xg = K_FF^-1 rhs_F, the Schur complement S = K_II - H_IF X, rI = rhs_I - H_IF xg, and the LDL^T
    view of the same elimination: U (rows k < nF as the earlier pivots leave them), dinv, the reduced z of the free
    rows.  x_bound given: x_F = K_FF^-1 (rhs_F - H_FI x_bound) too.  Dropped pivots give zero rows of X and xg."""
    H64 = np.asarray(H, np.float64)
    p = H64.shape[0]
    nI = p - nF
    md = max(float(H64.diagonal().max(initial=0.0)), 0.0)
    reg = _num(reg_rel) * _num(md)
    K = _num(H64)
    for i in range(p):
        K[i, i] = K[i, i] + reg
    b = _num(np.asarray(rhs, np.float64))
    R, keep = cholesky_dropping(K[:nF, :nF])
    Fk = np.flatnonzero(keep)
    nk = len(Fk)
    X = _num(np.zeros((nF, nI)))
    xg = _num(np.zeros(nF))
    W = _num(np.zeros((nk, nI)))   # R^-T H_FI
    for j in range(nI):
        W[:, j] = _fwd(R, K[Fk, nF + j]) if nk else W[:, j]
    yz = _fwd(R, b[Fk]) if nk else _num(np.zeros(0))
    if nk:
        for j in range(nI):
            X[Fk, j] = _bwd(R, W[:, j])
        xg[Fk] = _bwd(R, yz)
    S = K[nF:, nF:].copy()
    rI = b[nF:].copy()
    if nk and nI:
        S = S - np.dot(W.T, W)
        rI = rI - np.dot(W.T, yz)
    out = {"X": _f64(X), "xg": _f64(xg), "S": _f64(S), "rI": _f64(rI), "dropped": ~keep,
           "kappa_ff": _kappa2(_f64(K[np.ix_(Fk, Fk)])), "kappa": _kappa2(_f64(K))}
    # LDL^T view: row k of U = r_kk * (row k of [R | W]), d_k = r_kk^2, z_k = r_kk * (R^-T rhs_F)_k
    U = np.zeros((nF, p))
    dinv = np.zeros(nF)
    zF = np.zeros(nF)
    for a, k in enumerate(Fk):
        rkk = R[a, a]
        U[k, Fk[a:]] = _f64(rkk * R[a, a:])
        if nI:
            U[k, nF:] = _f64(rkk * W[a])
        dinv[k] = float(1 / (rkk * rkk))
        zF[k] = float(rkk * yz[a])
    out.update(U=U, dinv=dinv, zF=zF)
    if x_bound is not None:
        xb = _num(np.asarray(x_bound, np.float64))
        r = b[Fk]
        for j in range(nI):
            r = r - K[Fk, nF + j] * xb[j]
        xF = _num(np.zeros(nF))
        if nk:
            xF[Fk] = _spd_solve(R, r)
        out["xF"] = _f64(xF)
        # x_F with x_I given is the solve of the masked system [[K_FF, H_FI], [0, I]]: its kappa_2, its whole solution
        Mm = np.eye(nk + nI)
        Mm[:nk, :nk] = _f64(K[np.ix_(Fk, Fk)])
        Mm[:nk, nk:] = _f64(K[Fk, nF:]) if nI else Mm[:nk, nk:]
        out["kappa_masked"] = _kappa2(Mm)
        out["x_scale"] = float(max(np.abs(out["xF"]).max(initial=0.0), np.abs(_f64(xb)).max(initial=0.0)))
    return out


def exchange(T, seq):
    """Jordan exchanges of the pivots (J, J), J in seq, on the tableau T [n, n + 1] of y = S x + c
    (wave_prims.h tableau_exchange); an exchange whose pivot is not positive is refused.  -> (T', refused mask)"""
    T = _num(np.asarray(T, np.float64))
    n = T.shape[0]
    refused = 0
    for J in seq:
        d = T[J, J]
        if not (float(d) > PIVOT_MIN):
            refused |= 1 << J
            continue
        N = _num(np.zeros(T.shape))
        for i in range(n):
            for k in range(n + 1):
                if i == J and k == J:
                    N[i, k] = 1 / d
                elif i == J:
                    N[i, k] = -T[J, k] / d
                elif k == J:
                    N[i, k] = T[i, J] / d
                else:
                    N[i, k] = T[i, k] - T[i, J] * T[J, k] / d
        T = N
    return _f64(T), refused


def bound(p, eps, kappa, scale):
    return p * eps * kappa * scale


# ---------------------------------------------------------------------------------------------------------------
# systems: H = M W M^T, the form every Hessian of the Newton loop has
FAMILIES = ("pm1", "gauss", "scaled")


def _pm1_rows(rng, p, bw):
    """+-1 / 0 rows with 0/1 weights, built like the domain's cones: every column is an EDGE (two +-1 entries: the rows
    of a TSP degree system or of a node-arc incidence matrix) or a single +-1 entry.  A chain of edges (i, i + 1) of
    weight 1 and one single-entry column on row 0 keep H = M W M^T positive definite whatever the 0/1 weights of the
    other columns are; with a half bandwidth, edges join rows at most bw apart and (0, bw) has weight 1."""
    cols, w = [], []

    def edge(i, j, wt):
        c = np.zeros(p)
        c[i], c[j] = rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])
        cols.append(c)
        w.append(wt)

    def single(i, wt):
        c = np.zeros(p)
        c[i] = rng.choice([-1.0, 1.0])
        cols.append(c)
        w.append(wt)

    single(0, 1.0)
    for i in range(p - 1):
        edge(i, i + 1, 1.0)
    reach = p - 1 if bw is None else min(bw, p - 1)
    if reach >= 2:
        edge(0, reach, 1.0)
        for _ in range(2 * p):
            i = int(rng.integers(0, p - 2))
            j = int(rng.integers(i + 2, min(p, i + reach + 1))) if i + 2 < min(p, i + reach + 1) else i + 1
            edge(i, j, float(rng.random() < 0.7))
    for i in range(1, p):
        if rng.random() < 0.3:
            single(i, float(rng.random() < 0.7))
    return np.array(cols).T.reshape(p, -1), np.array(w)


def _real_rows(rng, family, p, bw):
    """Gaussian sparse rows (3 - 8 entries over 2 p columns; with a half bandwidth: the bw + 1 consecutive columns
    from the row's own on, the own entry raised to 1.5 + |g| and the others scaled by 0.7 / sqrt(bw): a random
    band M gives condition numbers that grow exponentially with p), weights in [0.2, 1]; family 'scaled':
    every row times e^u, u in [-3, 3]"""
    if bw is None:
        d = 2 * p + 2
        M = np.zeros((p, d))
        for i in range(p):
            cols = rng.choice(d, size=int(min(d, rng.integers(3, 9))), replace=False)
            M[i, cols] = rng.standard_normal(len(cols))
    else:
        d = p + bw
        M = np.zeros((p, d))
        for i in range(p):
            M[i, i:i + bw + 1] = rng.standard_normal(bw + 1)
            M[i, i + 1:i + bw + 1] *= 0.7 / np.sqrt(bw)
            M[i, i] = np.copysign(1.5 + abs(M[i, i]), M[i, i])
            for c in (i, i + bw):   # the ends of the window stay away from zero: the half bandwidth is exact
                if abs(M[i, c]) < 0.05:
                    M[i, c] = 0.25
    if family == "scaled":
        M *= np.exp(rng.uniform(-3.0, 3.0, p))[:, None]
    return M, rng.uniform(0.2, 1.0, d)


def draw_spd(seed, family, p, reg_rel=0.0, bw=None, zero_rows=()):
    """H [p, p] = M W M^T of the family with kappa_2(H + reg_rel max diag I) <= 1e8 (draws above are rejected and
    redrawn, so a seed always yields a case); bw: half bandwidth; zero_rows: rows / columns of H set exactly to zero
    afterwards (dropped pivots; kappa is that of the rest)."""
    rng = np.random.default_rng(seed)
    zero_rows = np.asarray(sorted(zero_rows), int)
    for _ in range(200):
        M, w = _pm1_rows(rng, p, bw) if family == "pm1" else _real_rows(rng, family, p, bw)
        H = (M * w) @ M.T
        H = 0.5 * (H + H.T)
        H[zero_rows, :] = 0.0
        H[:, zero_rows] = 0.0
        live = np.setdiff1d(np.arange(p), zero_rows)
        if len(live) == 0:
            return H
        K = H[np.ix_(live, live)] + reg_rel * max(H.diagonal().max(initial=0.0), 0.0) * np.eye(len(live))
        ev = np.linalg.eigvalsh(K)
        if ev[0] > 0 and ev[-1] / ev[0] <= KAPPA_MAX * 0.5:   # (room for the masked form's kappa, checked by the caller)
            return H
    raise AssertionError("no well-conditioned draw in 200 tries")


def act_patterns(rng, p, bw=None):
    """The `act` masks of the issue: none, random 20 %, first and last row, a run longer than the bandwidth, all but one."""
    pats = {"none": np.zeros(p, np.uint8)}
    a = (rng.random(p) < 0.2).astype(np.uint8)
    pats["random20"] = a
    a = np.zeros(p, np.uint8); a[0] = 1; a[-1] = 1
    pats["first_last"] = a
    run = min(p - 1, (bw if bw is not None else 3) + 2)
    a = np.zeros(p, np.uint8)
    s = int(rng.integers(0, p - run + 1))
    a[s:s + run] = 1
    pats["run"] = a
    a = np.ones(p, np.uint8); a[int(rng.integers(0, p))] = 0
    pats["all_but_one"] = a
    return pats


def band_pack(H, bw):
    """Hb[j * (bw + 1) + t] = H(j + t, j), the band form of cone_band.h"""
    p = H.shape[0]
    ld = bw + 1
    Hb = np.zeros((p, ld))
    for j in range(p):
        for t in range(min(ld, p - j)):
            Hb[j, t] = H[j + t, j]
    return Hb


def tri_pack(H):
    """packed lower triangle: H(i, j), j <= i, at i (i + 1) / 2 + j"""
    p = H.shape[0]
    return np.concatenate([H[i, :i + 1] for i in range(p)]) if p else np.zeros(0)


def fold_base(p, r):
    h = (p + 1) // 2
    return r * (p + 1) if r < h else (p - 1 - r) * (p + 1) + (r + 1)


def fold_pack(H):
    """folded upper triangle of cone_dense.h: entry (r, j >= r) at fold_base(p, r) + (j - r)"""
    p = H.shape[0]
    A = np.zeros(((p + 1) // 2) * (p + 1))
    for r in range(p):
        A[fold_base(p, r): fold_base(p, r) + p - r] = H[r, r:]
    return A


def fold_unpack(A, p):
    U = np.zeros((p, p))
    for r in range(p):
        U[r, r:] = A[fold_base(p, r): fold_base(p, r) + p - r]
    return U
