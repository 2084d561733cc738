"""Extended-precision restatement of the operators of the Newton loop (TEST INFRASTRUCTURE, numpy only).

The operators of cave_amd/csrc that build what the linear solvers are given and consume what they return -- the gathers
y - M^T theta, the gradient g = -M Pi(r), the Hessian M W M^T, the weight functions, the line search, the epilogue --
restated in a few lines each on the working precision of linsys_ref (np.longdouble, 64-bit mantissa; mpmath where long
double is narrower), from the documented behaviour and nothing else, together with the bound each test asserts.

Bounds (u = 2^-52 throughout, i.e. twice the unit round-off of a double: a product and the add that consumes it):

  * sums in floating point (gather_*, gradient in its team / long-row / streamed forms, dphi, the norm of
    refresh_clipped): element i is a sum of n_i terms formed by n_i additions in some tree.  Every add rounds once
    (relative 2^-53 of a partial sum that is at most S_i = sum |terms of i|), every product once, and a term passes
    through at most (chain on its lane) + (depth c of the reduction tree) adds.  So
        |err_i| <= (n_i + c) u S_i,
    n_i taken as ALL additions into i (never less than the longest chain), c = 8: six levels of a wave reduction plus
    at most two levels across the waves of a workgroup.
  * lite_gradient forms row i as P(last entry of i) - P(last entry of i - 1), P the prefix sum over ALL entries of the
    cone in storage order: a prefix is a lane run (chn8 adds), six scan levels and one add of (run + base), and the
    row takes two of them and a subtraction: n = 2 (chn8 + 7) + 1 adds, each relative to a partial sum bounded by
    S = sum over the whole cone |entry rc|.  |err_i| <= (2 (chn8 + 7) + 1) u S -- it does not scale with the row.
  * fixed point (dense_gradient, band_hessian, dense_hessian): a term x is added as llrint(x scale): rounding of the
    product(s) (u |x|) and to the grid (0.5 / scale); integer adds are exact; the final int64 -> double conversion and
    the multiplication by the power of two 1 / scale round once more (2^-53 of the sum), which the u of the first term
    (a single product needs only 2^-53 of it) leaves room for.  |err| <= n (0.5 / scale + u max|product|), n the number of
    terms added into the element, scale = fixed_scale(...) recomputed here.
  * +-1 cones with weights on the 1/16 grid: every partial sum is a multiple of 1/16 below 2^12: exact.
  * band_weight: five correctly rounded operations, 8 u relative where z >= 0 (CPU tier), 16 u with the device's rsqrt
    (a condition: a correct formula on a faithfully rounded rsqrt stays within it).  For z < 0 the final 1 + q cancels
    and a relative bound does not exist: see band_weight_scale for the absolute form both signs are held to.
  * epilogue: float outputs within 2^-24 |ref| (their rounding to float) + d u scale (the norms and dot products are
    sums of d terms) of the restatement.
"""

from __future__ import annotations

import math

import numpy as np

import linsys_ref as L

U = 2.0 ** -52
C_TREE = 8
K_LONG_ROW, K_TEAM_ROW = 64, 1024
NORM_CLAMP = 1e-8
INSIDE_RNORM = float(np.float32(1e-7))
MODE_PROJECT, MODE_EXACT, MODE_INNER, MODE_HEURISTIC, MODE_AVG, MODE_IPM = range(6)

_num, _f64 = L._num, L._f64


def _abs(a):
    return np.abs(a) if a.dtype != object else np.array([abs(v) for v in a.ravel()], dtype=object).reshape(a.shape)


def fixed_scale(vmax, rmax):
    """cone_dense.h: the power of two that takes the bound vmax * rmax to just below 2^61"""
    bound = max(float(vmax) * float(rmax), 1e-300)
    e = math.frexp(bound)[1]
    return math.ldexp(1.0, max(-1000, min(1000, 61 - e)))


def cone_scales(c):
    """largest |entry| and longest row (at least 1) of the reduced cone"""
    vm = 1.0 if c["pm1"] else float(np.abs(c["M"]).max(initial=0.0))
    ml = float(max(1, np.diff(np.asarray(c["mptr"], np.int64)).max(initial=1)))
    return vm, ml


# ------------------------------------------------------------------------------------------------- gathers, gradient
def gather(c, th, sgn, base):
    """out = base + sgn M^T th -> (out, bound)"""
    M, th = _num(c["M"]), _num(th)
    b = _num(np.zeros(c["d"]) if base is None else np.asarray(base, np.float64))
    out = b + sgn * np.dot(M.T, th)
    S = _abs(b) + np.dot(_abs(M).T, _abs(th))
    n = np.maximum(np.diff(np.asarray(c["cptr"], np.int64)), 1)
    return out, _f64(S) * (n + C_TREE) * U


def gradient(c, rc):
    """g = -M rc -> (g, bound, S): row-wise bound (n_i + c) u S_i"""
    M, rc = _num(c["M"]), _num(rc)
    g = -np.dot(M, rc)
    S = _f64(np.dot(_abs(M), _abs(rc)))
    n = np.diff(np.asarray(c["mptr"], np.int64))
    return g, (n + C_TREE) * U * S, S


def lite_gradient_bound(c, rc, chn8):
    S = float(np.dot(np.abs(c["M"]), np.abs(np.asarray(rc, np.float64))).sum())
    return (2 * (chn8 + 7) + 1) * U * S


def dense_gradient_bound(c, rc, gcol_bound):
    """fixed-point column-wise form; entries with rc == 0 add nothing"""
    rc = np.asarray(rc, np.float64)
    sc = fixed_scale(np.abs(rc).max(initial=0.0), gcol_bound)
    A = np.abs(c["M"]) * np.abs(rc)[None, :]
    n = (A != 0).sum(axis=1)
    return n * (0.5 / sc + U * A.max(axis=1, initial=0.0)), sc


# ------------------------------------------------------------------------------------------------------- clip, search
def clip(r, u):
    """residual left after the best multipliers of the +e_k / -e_k rows: u = 0: r, 1: min(r, 0), 2: max(r, 0), 3: 0"""
    r = _num(r)
    out = r.copy()
    for k, uk in enumerate(np.asarray(u)):
        rk = r[k]
        out[k] = rk if uk == 0 else (min(rk, 0 * rk) if uk == 1 else (max(rk, 0 * rk) if uk == 2 else 0 * rk))
    return out


def active(r, u):
    r = _f64(r)
    u = np.asarray(u)
    return (u == 0) | ((u == 1) & (r < 0)) | ((u == 2) & (r > 0))


def refresh(c, r, nt):
    """rc = Pi(r) (exact: the clip returns r or 0), f = 1/2 |rc|^2 -> (rc, f, bound of f)"""
    rc = clip(r, c["usign"])
    sq = rc * rc
    f = sq.sum() / 2
    n = -(-c["d"] // nt)
    return rc, f, (n + C_TREE) * U * float(f) * 2


def dphi(c, r, q, alpha, nt):
    """phi'(alpha), phi''(alpha) of phi = 1/2 |Pi(r - alpha q)|^2 -> (d1, d2, bound d1, bound d2, min |r - alpha q|)"""
    r, q = _num(r), _num(q)
    rr = r - alpha * q
    t = clip(rr, c["usign"])
    d1 = -(t * q).sum()
    d2 = (q * q)[active(rr, c["usign"])].sum() if c["d"] else 0
    n = -(-c["d"] // nt)
    S1 = float(((_abs(r) + abs(alpha) * _abs(q)) * _abs(q)).sum())
    return d1, d2, (n + C_TREE + 3) * U * S1, (n + C_TREE) * U * float(d2), float(min(_abs(rr))) if c["d"] else 1.0


def update_theta(c, theta, tc, dv, alpha, amax):
    """theta + alpha dv, exact zeros for variables parked at / blocked by a bound -> (t, tol, must_be_zero)"""
    th, dv_, tc = np.asarray(theta, np.float64), np.asarray(dv, np.float64), np.asarray(tc, np.float64)
    t = _num(th) + alpha * _num(dv_)
    bound = np.asarray(c["vkind"]) == 0
    zero = bound & (((alpha == 1.0) & (tc == 0.0)) | (_f64(t) < 0.0) |
                    ((alpha >= amax) & (dv_ < 0.0) & (th <= -amax * dv_ * (1.0 + 1e-12))))
    t[zero] = 0 * t[zero]
    return t, 2 * U * (np.abs(th) + abs(alpha) * np.abs(dv_)), zero


def phi_pl(x, y, a):
    """the piecewise-linear phi' of exact_step's driver at a (end segments extended)"""
    j = 0
    while j + 2 < len(x) and a >= x[j + 1]:
        j += 1
    sl = (y[j + 1] - y[j]) / (x[j + 1] - x[j])
    return y[j] + sl * (a - x[j])


# ------------------------------------------------------------------------------------------------------------ weights
def band_weight(u, r, inv_mu):
    """1 (u = 0), 0 (u = 3), else 1/2 (1 + z / sqrt(1 + z^2)), z = t / mu, t the residual on the side that carries it;
    mu = 0: the binary weight"""
    r = _num(np.asarray(r, np.float64))
    out = _num(np.zeros(len(r)))
    for k, uk in enumerate(np.asarray(u)):
        if uk == 0:
            out[k] = out[k] * 0 + 1
        elif uk == 3:
            out[k] = out[k] * 0
        else:
            t = r[k] if uk == 2 else -r[k]
            if inv_mu > 0:
                z = t * _num([inv_mu])[0]
                out[k] = (1 + z / L._sqrt(1 + z * z)) / 2
            else:
                out[k] = out[k] * 0 + (1 if t > 0 else 0)
    return out


def band_weight_scale(u, w, inv_mu):
    """scale of band_weight's rounding error: with q = z / sqrt(1 + z^2) (relative error 5 x 2^-53: z, z^2, 1 + z^2, the
    root, the quotient) the weight (1 + q) / 2 carries 2.5 x 2^-53 |q| + 2^-53 w absolutely -- for z < 0 the sum cancels,
    so the error is NOT relative to w.  The tests assert |err| <= k u (w + |q| / 2), k = 4 under emulation (8 u w where
    z >= 0) and 8 on the device (16 u w); 0 (exact) where the weight is 0, 1 or binary"""
    w = _num(w)
    out = np.zeros(len(w))
    for k, uk in enumerate(np.asarray(u)):
        if uk in (1, 2) and inv_mu > 0:
            out[k] = float(w[k]) + abs(float(2 * w[k] - 1)) / 2
    return out


def lite_weight(u, r, mu):
    """quantised weight of lite_hessian -> (level in sixteenths, distance of the rounded argument from the nearest
    half-integer boundary, as a fraction of a level)"""
    r = _num(np.asarray(r, np.float64))
    lev, dist = np.zeros(len(r)), np.ones(len(r))
    for k, uk in enumerate(np.asarray(u)):
        if uk == 0:
            lev[k] = 16
        elif uk == 3:
            lev[k] = 0
        else:
            t = r[k] if uk == 2 else -r[k]
            lev[k] = 16 if t > 0 else 0
            if mu > 0:
                z = t / _num([mu])[0]
                if abs(float(z)) < 4.0:
                    a = 8 * (1 + z / L._sqrt(1 + z * z)) + 0.5
                    lev[k] = math.floor(float(a))
                    dist[k] = abs(float(a) - round(float(a)))
    return lev, dist


# ------------------------------------------------------------------------------------------------------------ Hessian
def hessian(c, w):
    """H = M diag(w) M^T over the weights > 1e-14 -> (H, number of terms per entry, largest |term| per entry)"""
    M = c["M"]
    w = np.asarray(w, np.float64)
    on = w > 1e-14
    Ml = _num(M[:, on])
    H = np.dot(Ml * _num(w[on])[None, :], Ml.T) if on.any() else _num(np.zeros((c["p"], c["p"])))
    nzm = (M[:, on] != 0).astype(np.float64)
    n = nzm @ nzm.T
    A = np.abs(M[:, on])
    mx = np.zeros((c["p"], c["p"]))
    for k in range(A.shape[1]):
        col = A[:, k]
        np.maximum(mx, w[on][k] * np.outer(col, col), out=mx)
    return H, n, mx


def band_layout(H, ldh):
    """H[j ldh + t] = H(j + t, j), t < ldh; past the matrix: 0"""
    p = H.shape[0]
    out = np.zeros((p, ldh), dtype=H.dtype) if H.dtype != object else _num(np.zeros((p, ldh)))
    for j in range(p):
        for t in range(min(ldh, p - j)):
            out[j, t] = H[j + t, j]
    return out.ravel()


def fold_base(p, r):
    h = (p + 1) // 2
    return r * (p + 1) if r < h else (p - 1 - r) * (p + 1) + (r + 1)


def fold_entries(p):
    return ((p + 1) // 2) * (p + 1)


def fold_layout(H, pos):
    """folded upper triangle in elimination order: entry (a, b >= a) of positions at fold_base(a) + (b - a)"""
    p = H.shape[0]
    ordr = np.argsort(pos)
    Hp = H[np.ix_(ordr, ordr)]
    out = _num(np.zeros(fold_entries(p))) if H.dtype == object else np.zeros(fold_entries(p), dtype=H.dtype)
    for a in range(p):
        fb = fold_base(p, a)
        out[fb:fb + p - a] = Hp[a, a:]
    return out


def dense_order(vkind):
    """rows with free multipliers first, rows with bounds last, both in their stored order -> (pos, ord, nF)"""
    vk = np.asarray(vkind)
    ordr = np.concatenate([np.flatnonzero(vk != 0), np.flatnonzero(vk == 0)])
    pos = np.empty(len(vk), np.int64)
    pos[ordr] = np.arange(len(vk))
    return pos, ordr, int((vk != 0).sum())


# ----------------------------------------------------------------------------------------------------------- epilogue
def epilogue(mode, sign, inner_ratio, empty, y, res, f, avg):
    """-> dict of long-double values BEFORE the final rounding to float (proj, rnorm, target, loss, grad) and the scale
    of each output's accumulated error.  The projection and the target are rounded to float where the product's are
    (the reference returns float32 tensors); the target is held constant in the derivative."""
    y32 = np.asarray(y, np.float32)
    yl, d = _num(y32.astype(np.float64)), len(y32)
    out, scale = {}, {}
    if mode == MODE_AVG:
        out["target"], scale["target"] = _num(np.asarray(avg, np.float64)), 0.0
        return out, scale
    has_proj = mode != MODE_HEURISTIC
    rn32 = np.float32(0)
    if has_proj:
        pk = yl.copy() if empty else yl - _num(res)
        out["proj"], scale["proj"] = pk, float(max(_abs(yl))) + float(np.abs(np.asarray(res, np.float64)).max(initial=0.0))
        p32 = _num(_f64(pk).astype(np.float32).astype(np.float64))
        out["rnorm"] = _num([0.0])[0] if empty else L._sqrt(2 * _num([f])[0])
        scale["rnorm"] = float(out["rnorm"])
        rn32 = np.float32(float(out["rnorm"]))
        pp = (p32 * p32).sum()
    if mode == MODE_PROJECT:
        return out, scale
    ss = (yl * yl).sum()
    ns = L._sqrt(ss)
    ns_c = max(ns, NORM_CLAMP)
    r = _num([float(np.float32(inner_ratio))])[0]
    al = _num(np.asarray(avg, np.float32).astype(np.float64))
    if has_proj:
        np_c = max(L._sqrt(pp), NORM_CLAMP)
        pn = p32 / np_c
    if mode in (MODE_EXACT, MODE_IPM):
        t = pn
    elif mode == MODE_INNER:
        t = pn if rn32 < np.float32(INSIDE_RNORM) else (1 - r) * pn + r * al
    else:
        t = (1 - r) * (yl / ns_c) + r * al
    out["target"], scale["target"] = t, 1.0
    t32 = _num(_f64(t).astype(np.float32).astype(np.float64))
    nt_c = max(L._sqrt((t32 * t32).sum()), NORM_CLAMP)
    st = (yl * t32).sum()
    out["loss"], scale["loss"] = 1 - st / (ns_c * nt_c), 1.0
    radial = st / (ns_c * ns_c * ns * nt_c) if float(ns) > NORM_CLAMP else 0 * st
    out["grad"] = -sign * (t32 / (ns_c * nt_c) - radial * yl)
    scale["grad"] = float(max(_abs(t32)) / (ns_c * nt_c) + abs(radial) * max(_abs(yl)))
    out["_cos"] = lambda s: (s * t32).sum() / (max(L._sqrt((s * s).sum()), NORM_CLAMP) * nt_c)  # target held constant
    return out, scale
