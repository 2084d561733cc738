"""The APGD projector of include/cave_hip.h (cave_hip_cone_apgd) restated in extended precision (TEST INFRASTRUCTURE).

`run(A, pred, sign, n_iter, power_iter)` is the algorithm of the header comment -- the reference's `project_apgd`
(src/qpsolver.py:11-110) with `tol_grad=None` -- in np.longdouble, vectorised over the batch: A is the dense
(B, m_max, d) block as given, zero rows included.  `run(..., order=...)` runs the same program in double with every row
sum and column sum taken in a stated order: 'asc' (index order, what the kernel does), 'desc' and 'pair' (a balanced
tree).  The three twins sample the distribution of summation orders; `spread` is their largest deviation from the
long-double result, relative to the largest magnitude of the quantity: the S of the bounds below.

Bounds (derived, not chosen; the factor 8 covers a fourth sample of the order distribution, the device's fma contraction):
  float outputs against the restatement        2^-24 |ref| + 8 S scale
  fp64 state and pgrad                         8 S scale + one ulp
  float outputs against the fp32 reference     |ref32 - ref64| + 2^-24 |ref64| + 8 S scale   (triangle inequality)
"""

from __future__ import annotations

import numpy as np

LD = np.longdouble
EPS32 = 2.0 ** -24
SNAP = (1, 2, 3, 20, 200, 400)


def _sum(P, axis, order, dt):
    """sum of P along `axis` in the stated order (None: numpy's own, for the long-double run)"""
    if order is None:
        return P.sum(axis=axis)
    P = np.moveaxis(P, axis, -1)
    n = P.shape[-1]
    if order == "pair":
        while P.shape[-1] > 1:
            if P.shape[-1] & 1:
                P = np.concatenate([P, np.zeros(P.shape[:-1] + (1,), dt)], axis=-1)
            P = P[..., 0::2] + P[..., 1::2]
        return P[..., 0] if n else np.zeros(P.shape[:-1], dt)
    acc = np.zeros(P.shape[:-1], dt)
    for j in (range(n) if order == "asc" else range(n - 1, -1, -1)):
        acc = acc + P[..., j]
    return acc


class Result:
    """x_curr, x_prev [B, m], step [B], proj [B, d], rnorm [B] (un-squared), target [B, d], loss [B], grad [B, d] (d loss /
    d pred), pgrad [B]; `snaps[k]`: the Result after k iterations for the k asked for"""


def run(A, pred, sign=1.0, n_iter=200, power_iter=8, order=None, snaps=()):
    dt = LD if order is None else np.float64
    A = np.asarray(A, np.float32).astype(dt)
    B, m, d = A.shape
    y = dt(sign) * np.asarray(pred, np.float32).astype(dt)
    At = lambda v: _sum(A * v[:, :, None], 1, order, dt)   # A^T v: column sums over the rows
    Ax = lambda u: _sum(A * u[:, None, :], 2, order, dt)   # A u: row sums over the columns
    norm = lambda v: np.sqrt(_sum(v * v, 1, order if order is None else "asc", dt))
    tiny = dt(1e-8)
    v = np.full((B, m), dt(1) / np.sqrt(dt(m)), dt)
    for _ in range(power_iter):
        v = Ax(At(v))
        v = v / np.maximum(norm(v), tiny)[:, None]
    u = At(v)
    s = dt(1) / np.maximum(_sum(u * u, 1, order if order is None else "asc", dt), tiny)
    xc = np.zeros((B, m), dt)
    xp = xc.copy()

    def results():
        r = Result()
        r.x_curr, r.x_prev, r.step = xc.copy(), xp.copy(), s.copy()
        r.proj = At(xc)
        g = Ax(r.proj - y)
        r.pgrad = np.where(xc > 0, np.abs(g), np.maximum(-g, 0)).max(axis=1) if m else np.zeros(B, dt)
        # pgrad is a residual: its rounding error is relative to the terms that cancel in it, max_i sum_c |a_ic| (|proj_c| + |y_c|)
        r.gscale = (np.abs(A) * (np.abs(r.proj) + np.abs(y))[:, None, :]).sum(axis=2).max(axis=1).astype(np.float64) if m else np.zeros(B)
        r.yscale = norm(y).astype(np.float64)  # and rnorm = ||y - proj|| is one too: relative to ||y||
        r.rnorm = norm(y - r.proj)
        t = r.proj / np.maximum(norm(r.proj), tiny)[:, None]
        r.target = t
        t = t.astype(np.float32).astype(dt)  # the target is a float32 vector: loss and gradient are those of the rounded one
        ns, nt = norm(y), norm(t)
        ns_c, nt_c = np.maximum(ns, tiny), np.maximum(nt, tiny)
        st = _sum(y * t, 1, order if order is None else "asc", dt)
        r.loss = 1 - st / (ns_c * nt_c)
        radial = np.where(ns > tiny, st / (ns_c * ns_c * np.where(ns > 0, ns, 1) * nt_c), 0)
        r.grad = -dt(sign) * (t / (ns_c * nt_c)[:, None] - radial[:, None] * y)
        return r

    out = {}
    if 0 in snaps:
        out[0] = results()
    for k in range(n_iter):
        beta = dt(0) if k == 0 else dt(k - 2) / dt(k + 1)
        yk = xc + beta * (xc - xp)
        g = Ax(At(yk) - y)
        xp, xc = xc, np.maximum(yk - s[:, None] * g, 0)
        if k + 1 in snaps:
            out[k + 1] = results()
    r = results()
    r.snaps = out
    return r


FIELDS = ("x_curr", "x_prev", "step", "proj", "rnorm", "target", "loss", "grad", "pgrad")


def scale(ref, name):
    """the magnitude a deviation of `name` is relative to: the largest entry of the instance (1 at the least for the
    unit-scale quantities target / loss / grad; for the residual quantities pgrad and rnorm the magnitude of the terms that cancel in them)"""
    if name == "pgrad":
        return np.maximum(ref.gscale, np.abs(np.asarray(ref.pgrad, np.float64)))
    if name == "rnorm":
        return np.maximum(ref.yscale, np.abs(np.asarray(ref.rnorm, np.float64)))
    a = np.abs(np.asarray(getattr(ref, name), np.float64))
    mx = a.reshape(a.shape[0], -1).max(axis=1) if a.size else np.zeros(a.shape[0])
    if name in ("target", "loss", "grad"):
        mx = np.maximum(mx, 1.0)
    return mx


def spread(ref, twins, fields=FIELDS):
    """S: the largest deviation of a twin from the long-double result over `fields`, relative to scale()"""
    S = 0.0
    for name in fields:
        r = getattr(ref, name)
        sc = np.maximum(scale(ref, name), np.finfo(np.float64).tiny)
        for t in twins:
            dev = np.abs(getattr(t, name).astype(LD) - r).astype(np.float64)
            dev = dev.reshape(dev.shape[0], -1).max(axis=1) if dev.size else np.zeros(dev.shape[0])
            S = max(S, float((dev / sc).max()) if dev.size else 0.0)
    return S


def twins(A, pred, sign, n_iter, power_iter, snaps=()):
    return [run(A, pred, sign, n_iter, power_iter, order=o, snaps=snaps) for o in ("asc", "desc", "pair")]


def float_bound(ref, name, S):
    """[B] or [B, 1]: 2^-24 |ref| + 8 S scale, elementwise in |ref|"""
    r = np.abs(np.asarray(getattr(ref, name), np.float64))
    sc = scale(ref, name)
    return EPS32 * r + 8 * S * (sc if r.ndim == 1 else sc[:, None])


def state_bound(ref, name, S):
    """8 S scale + one ulp (of the entry)"""
    r = np.abs(np.asarray(getattr(ref, name), np.float64))
    sc = scale(ref, name)
    return 8 * S * (sc if r.ndim == 1 else sc[:, None]) + np.spacing(r)


def densify(m, d, rows, cols, vals):
    A = np.zeros((m, d), np.float32)
    A[rows, cols] = vals
    return A
