"""The interior-point iterate of CAVE_MODE_INNER_IPM, restated in extended precision (TEST INFRASTRUCTURE, numpy only).

DESIGN section 3c and the comment above solve_cone_ipm_impl (cave_amd/csrc/cone_core.h) define a deterministic
procedure; every implementation of the mode -- the LDS-resident general kernels, the band / dense forms of the large
path, lite_solve_ipm, the serial build -- claims to run it.  `iterate` below runs it on the working precision of
linsys_ref (np.longdouble, 64-bit mantissa; mpmath numbers where long double is no wider than double), from that text
and from the reduction of build_ref.reduce_instance, not from the code's loops:

    y      the float32 prediction times `sign`, ymax = max |y_k|
    tau0   = 0.1 ymax^2 (1e-300 when ymax = 0), floor tau_min = max(1e-14 ymax^2, 1e-300)
    theta  = z = sqrt(tau0) on the bound rows (vkind = 0), 0 on the free rows (vkind = 1: a +a / -a pair)
    smoothing at tau of s = y - M^T theta by usign:   q = sqrt(s^2 + 4 tau)
        0 (no unit row)   rho = s              rho' = 1
        1 (+e_k)          rho = (s - q) / 2    rho' = (1 - s / q) / 2
        2 (-e_k)          rho = (s + q) / 2    rho' = (1 + s / q) / 2
        3 (both)          rho = 0              rho' = 0
    one step:  (M diag(rho') M^T + diag(z / theta) + 1e-12 max diag I) dtheta = M rho + tau / theta   (bound rows carry
               the barrier terms; a pivot that is not positive is dropped, dtheta_k = 0, as every solver here does)
               dz = tau / theta - z - (z / theta) dtheta                                              (bound rows)
               alpha_p = min(1, 0.995 min_{dtheta_i < 0} -theta_i / dtheta_i), alpha_d the same for z, dz
               theta += alpha_p dtheta (every row), z += alpha_d dz
               tau <- 0.2 sum theta_i z_i / nineq   (0.2 tau when no row carries a bound), floored at tau_min
    result after k steps: s = y - M^T theta, smoothed at the NEW tau: rho, proj = y - rho, f = 1/2 |rho|^2,
               rnorm = sqrt(2 f).  A cone without reduced rows (p = 0) runs no step: the smoothing of y at tau0.

`weights`: how rho' enters the Hessian.  The LDS-resident and lite forms keep it in a float array (w.wold): 'f32'
rounds it to float32 first; the band / dense forms of the large path keep it in doubles (w.q): 'f64'.  This is part of
what each form computes -- at 1.7e-8 of the state it is larger than anything else in it.

`twins` restates the same steps in IEEE double eight times over -- reduced rows permuted by a seeded draw, sums taken
forward or reversed, Cholesky or LDL^T, M rho row by row or as differences of one running sum -- and `spread` measures how far those correct double realisations drift from
the extended-precision run, per step and quantity: S_k.  It is measured on the reference alone, never on a kernel.

`fixed_point_shift` pushes the entry-wise bound of the fixed-point Hessian of the multi-wave general kernels
(ops_ref.py: n (0.5 / scale + 2^-52 max |product|)) through the steps: four seeded sign patterns of a dH of that size,
the largest change of each quantity: F_k.
"""

from __future__ import annotations

import numpy as np

import build_ref as BR
import linsys_ref as L
import ops_ref as R

CONSTS = {"tau0": 0.1, "frac": 0.995, "sigma": 0.2, "floor": 1e-14, "shift": 1e-12}
QUANT = ("proj", "rnorm", "f", "theta_b", "z_b", "mtheta")   # what a spread / shift is measured on


# ------------------------------------------------------------------------------------------------ arithmetic helpers
class _Wide:
    """working precision of linsys_ref: long double, or mpmath numbers"""
    num = staticmethod(L._num)

    @staticmethod
    def sqrt(a):
        a = np.asarray(a)
        if a.dtype != object:
            return np.sqrt(a)
        out = np.empty(a.shape, dtype=object)
        for idx in np.ndindex(a.shape):
            out[idx] = L._sqrt(a[idx])
        return out if a.shape else out[()]

    # M^T th, M rho, M diag(dr) M^T
    mt = staticmethod(lambda M, th, rev: np.dot(M.T, th))
    mrho = staticmethod(lambda M, rho, rev: np.dot(M, rho))
    hess = staticmethod(lambda M, dr, rev: np.dot(M * dr[None, :], M.T))


class _Double:
    """IEEE double, sums in a stated order (einsum without `optimize` adds term after term)"""
    num = staticmethod(lambda a: np.array(a, dtype=np.float64))
    sqrt = staticmethod(np.sqrt)

    @staticmethod
    def mt(M, th, rev):
        return np.einsum("ik,i->k", M[::-1], th[::-1]) if rev else np.einsum("ik,i->k", M, th)

    @staticmethod
    def mrho(M, rho, rev):
        return np.einsum("ik,k->i", M[:, ::-1], rho[::-1]) if rev else np.einsum("ik,k->i", M, rho)

    @staticmethod
    def mrho_prefix(M, rho, rev):
        """M rho as lite_gradient forms it (ops_ref.py): row i = P(last entry of i) - P(last entry of i - 1), P the
        running sum over ALL entries of the cone in storage order -- its rounding is relative to the whole cone's sum"""
        r, k = np.nonzero(M)
        P = np.concatenate([[0.0], np.cumsum(M[r, k] * rho[k])])
        ends = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M.shape[0]))])
        return P[ends[1:]] - P[ends[:-1]]

    @staticmethod
    def hess(M, dr, rev):
        if rev:
            return np.einsum("ik,k,jk->ij", M[:, ::-1], dr[::-1], M[:, ::-1])
        return np.einsum("ik,k,jk->ij", M, dr, M)


def _f32_round(a):
    """a double rounded to float32 and back, as `(float)dr` does to a double"""
    return L._f64(a).astype(np.float32).astype(np.float64)


def _solve_chol(K, b, ar):
    """(K) x = b by an upper Cholesky factor in index order; a pivot that is not positive is dropped (x_k = 0)"""
    n = len(b)
    Rm = ar.num(np.zeros((n, n)))
    keep = np.zeros(n, bool)
    for k in range(n):
        row = K[k, k:] - np.dot(Rm[:k, k], Rm[:k, k:]) if k else K[k, k:].copy()
        if not (float(row[0]) > L.PIVOT_MIN):
            continue
        keep[k] = True
        Rm[k, k:] = row / ar.sqrt(row[0])
    idx = np.flatnonzero(keep)
    x = ar.num(np.zeros(n))
    if len(idx):
        Rk = Rm[np.ix_(idx, idx)]
        yv = ar.num(np.zeros(len(idx)))
        for i in range(len(idx)):
            yv[i] = (b[idx[i]] - (np.dot(Rk[:i, i], yv[:i]) if i else 0)) / Rk[i, i]
        xv = ar.num(np.zeros(len(idx)))
        for i in range(len(idx) - 1, -1, -1):
            xv[i] = (yv[i] - (np.dot(Rk[i, i + 1:], xv[i + 1:]) if i + 1 < len(idx) else 0)) / Rk[i, i]
        x[idx] = xv
    return x


RCP_EPS = 2.0 ** -47   # linsys_ref.EPS_ONE_NEWTON: the register Gauss-Jordan forms take v_rcp_f64 + one Newton step


def _solve_ldl(K, b, ar, rcp=None):
    """the same system by LDL^T (no square roots), same pivot rule.  rcp: a generator -> every pivot's reciprocal is
    off by a relative error drawn from +-RCP_EPS, as the solvers of one wave are documented to be on the device"""
    n = len(b)
    A = K.copy()
    z = b.copy()
    dinv = ar.num(np.zeros(n))
    keep = np.zeros(n, bool)
    for k in range(n):
        dk = A[k, k]
        if not (float(dk) > L.PIVOT_MIN):
            A[k, :] = A[k, :] * 0
            A[:, k] = A[:, k] * 0
            continue
        keep[k] = True
        dinv[k] = 1 / dk if rcp is None else (1 / dk) * (1 + rcp.uniform(-RCP_EPS, RCP_EPS))
        if k + 1 < n:
            l = A[k, k + 1:] * dinv[k]
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - np.outer(l, A[k, k + 1:])
            z[k + 1:] = z[k + 1:] - l * z[k]
    x = ar.num(np.zeros(n))
    for k in range(n - 1, -1, -1):
        if keep[k]:
            x[k] = (z[k] - (np.dot(A[k, k + 1:], x[k + 1:]) if k + 1 < n else 0)) * dinv[k]
    return x


# ------------------------------------------------------------------------------------------------------ the procedure
def _smooth(s, us, tau, ar):
    q = ar.sqrt(s * s + 4 * tau)
    one = s * 0 + 1
    sq = s / q
    rho = np.where(us == 1, (s - q) / 2, np.where(us == 2, (s + q) / 2, np.where(us == 3, s * 0, s)))
    dr = np.where(us == 1, (one - sq) / 2, np.where(us == 2, (one + sq) / 2, np.where(us == 3, s * 0, one)))
    return rho, dr


def _run(M, vk, us, y, steps, weights, ar, solver=_solve_chol, rev=False, consts=None, dH=None, mutate=(), prefix=False):
    """the steps on the reduced cone (M [p, d] float64, vkind, usign) -> list of states, one per step count 0 .. steps.
    dH(step, H, dr) -> a perturbation added to the step matrix (fixed_point_shift).  `mutate`: names of deliberate
    departures from the procedure (tests of the tests: the sensitivity table of DESIGN section 2)."""
    c = dict(CONSTS, **(consts or {}))
    p, d = M.shape
    Mn = ar.num(M)
    yn = ar.num(np.asarray(y, np.float32).astype(np.float64))
    bound = np.asarray(vk) == 0
    if "nineq_all" in mutate:
        nineq = p
    else:
        nineq = int(bound.sum())
    ymax = max([abs(v) for v in yn], default=yn.sum() * 0)
    tau = ar.num(c["tau0"])[()] * ymax * ymax
    if not (float(tau) > 0.0):
        tau = ar.num(1e-300)[()]
    tau_min = ar.num(c["floor"])[()] * ymax * ymax
    if not (float(tau_min) > 1e-300):
        tau_min = ar.num(1e-300)[()]
    th = ar.num(np.zeros(p))
    z = ar.num(np.zeros(p))
    th[bound] = ar.sqrt(tau)
    z[bound] = ar.sqrt(tau)
    usm = np.asarray(us)
    if "swap_u" in mutate:
        usm = np.where(usm == 1, 2, np.where(usm == 2, 1, usm))
    states = []

    def snapshot(tau_smooth, ap, ad, kappa):
        mt = ar.mt(Mn, th, rev) if p else yn * 0
        s = yn - mt
        rho, _ = _smooth(s, usm, tau_smooth, ar)
        f = (rho * rho).sum() / 2
        states.append({"s": s, "rho": rho, "proj": yn - rho, "f": f, "rnorm": ar.sqrt(2 * f), "theta": th.copy(), "z": z.copy(),
                       "theta_b": th[bound].copy(), "z_b": z[bound].copy(), "mtheta": mt, "tau": tau, "alpha_p": ap,
                       "alpha_d": ad, "kappa": kappa})

    snapshot(tau, None, None, None)
    for it in range(steps if p > 0 else 0):
        tau_old = tau
        mt = ar.mt(Mn, th, rev)
        s = yn - mt
        rho, dr = _smooth(s, usm, tau, ar)
        if weights == "f32":
            dr = ar.num(_f32_round(dr))
        else:
            assert weights == "f64", weights
        mrho, H = (ar.mrho_prefix if prefix else ar.mrho)(Mn, rho, rev), ar.hess(Mn, dr, rev)
        rhs = mrho.copy()
        inv = 1 / th[bound]
        if "no_rhs_barrier" not in mutate:
            rhs[bound] = rhs[bound] + tau * inv
        H = H.copy()
        if "no_diag_barrier" not in mutate:
            H[bound, bound] = H[bound, bound] + z[bound] * inv
        if dH is not None:
            H = H + ar.num(dH(it, L._f64(H), L._f64(dr)))
        md = max([v for v in H.diagonal()], default=tau * 0)
        if not (float(md) > 0.0):
            md = md * 0
        K = H.copy()
        K[np.arange(p), np.arange(p)] = K[np.arange(p), np.arange(p)] + ar.num(c["shift"])[()] * md
        kappa = L._kappa2(L._f64(K))
        dth = solver(K, rhs, ar)
        dz = z * 0
        dz[bound] = tau * inv - ("no_minus_z" not in mutate) * z[bound] - z[bound] * inv * dth[bound]
        ap = min([-th[i] / dth[i] for i in np.flatnonzero(bound) if float(dth[i]) < 0.0], default=ar.num(1e300)[()])
        ad = min([-z[i] / dz[i] for i in np.flatnonzero(bound) if float(dz[i]) < 0.0], default=ar.num(1e300)[()])
        fr = ar.num(c["frac"])[()]
        alpha_p = min(fr * ap, fr * 0 + 1)
        alpha_d = min(fr * ad, fr * 0 + 1)
        th = th + (alpha_d if "alpha_d_on_theta" in mutate else alpha_p) * dth
        z = z + alpha_d * dz
        gap = (th * z).sum()
        sg = ar.num(c["sigma"])[()]
        tau = sg * gap / nineq if nineq > 0 else sg * tau
        if not (float(tau) > float(tau_min)):
            tau = tau_min
        snapshot(tau_old if "old_tau" in mutate else tau, alpha_p, alpha_d, kappa)
    return states


def reduced(A):
    """the reduction of one dense instance in the terms the procedure needs"""
    red = BR.reduce_instance(A)
    return {"M": red["M"].astype(np.float64), "vkind": red["vkind"], "usign": red["usign"], "p": red["p"], "d": red["d"],
            "empty": red["n_valid"] == 0, "pm1": red["pm1"], "avg": red["avg"]}


def _empty_states(y, steps, ar):
    yn = ar.num(np.asarray(y, np.float32).astype(np.float64))
    st = {"s": yn, "rho": yn * 0, "proj": yn, "f": yn.sum() * 0, "rnorm": yn.sum() * 0, "theta": ar.num(np.zeros(0)),
          "z": ar.num(np.zeros(0)), "theta_b": ar.num(np.zeros(0)), "z_b": ar.num(np.zeros(0)), "mtheta": yn * 0,
          "tau": None, "alpha_p": None, "alpha_d": None, "kappa": None}
    return [st] * (steps + 1)


def iterate(A, y, steps, weights="f32", **kw):
    """A [m, d] float32 (one dense instance), y [d] float32 (ALREADY times sign) -> the state after every step count
    j = 0 .. steps (list of dicts: s, rho, proj, f, rnorm, theta, z, theta_b / z_b (bound rows), mtheta, tau, alpha_p,
    alpha_d, kappa; extended precision).  A cone without valid rows returns y itself (src/cave.py:304-305)."""
    c = A if isinstance(A, dict) else reduced(A)
    if c["empty"]:
        return _empty_states(y, steps, _Wide)
    st = _run(c["M"], c["vkind"], c["usign"], y, steps, weights, _Wide, **kw)
    return st + [st[-1]] * (steps + 1 - len(st))   # p = 0: no step is ever run


def twins(A, y, steps, n=8, weights="f32", rcp=False):
    """n restatements in IEEE double -> list of state lists.  Twin t: rows permuted by the draw of seed t (twin 0: as
    stored), sums forward (t even) or reversed (t odd), Cholesky (t & 2 == 0) or LDL^T, M rho row by row (t & 4 == 0) or
    as differences of one running sum over the whole cone (the form of lite_gradient, whose rounding does not scale
    with the row: a correct realisation that row-wise sums alone do not sample).  rcp: the LDL^T twins take reciprocals
    accurate to 2^-47 only (linsys_ref.EPS_ONE_NEWTON) -- for the forms whose solver is a register Gauss-Jordan of one
    wave (WaveCtx::solve_spd, gj_solve of the lite form) where the tier has the device's reciprocal (the _rcp24
    emulation, the MI355X); the plain emulation divides exactly.  theta / z come back in the stored row order."""
    c = A if isinstance(A, dict) else reduced(A)
    if c["empty"]:
        return [_empty_states(y, steps, _Double) for _ in range(n)]
    out = []
    p = c["p"]
    for t in range(n):
        perm = np.arange(p) if t == 0 else np.random.default_rng([t, p, c["d"]]).permutation(p)
        st = _run(c["M"][perm], c["vkind"][perm], c["usign"], y, steps, weights, _Double,
                  solver=_ldl_of(t, rcp) if t & 2 else _solve_chol, rev=bool(t & 1), prefix=bool(t & 4))
        back = np.argsort(perm)
        for s_ in st:
            s_["theta"], s_["z"] = s_["theta"][back], s_["z"][back]
            b = c["vkind"] == 0
            s_["theta_b"], s_["z_b"] = s_["theta"][b], s_["z"][b]
        out.append(st + [st[-1]] * (steps + 1 - len(st)))
    return out


def _ldl_of(t, rcp):
    if not rcp:
        return _solve_ldl
    rng = np.random.default_rng([t, 47])
    return lambda K, b, ar: _solve_ldl(K, b, ar, rng)


def _dev(a, b):
    return float(np.abs(np.atleast_1d(L._f64(np.asarray(a) - np.asarray(b)))).max(initial=0.0))


def spread(ref, tw):
    """S_j per quantity: the largest deviation of a twin from the extended-precision run at step count j"""
    return [{q: max(_dev(t[j][q], ref[j][q]) for t in tw) for q in QUANT} for j in range(len(ref))]


def hessian_terms(M, dr):
    """per entry of M diag(dr) M^T over the weights > 0: (number of terms, largest |term|)"""
    on = dr > 0
    A = np.abs(M[:, on])
    nz = (A != 0).astype(np.float64)
    n = nz @ nz.T
    mx = np.zeros((M.shape[0], M.shape[0]))
    for k, wk in zip(range(A.shape[1]), dr[on]):
        np.maximum(mx, wk * np.outer(A[:, k], A[:, k]), out=mx)
    return n, mx


def hessian_scale(c):
    """cone_instance.h: fixed_scale(vm, vm * ml), vm the largest |entry| (1 for a +-1 cone), ml the longest reduced row"""
    vm = 1.0 if c["pm1"] else float(np.abs(c["M"]).max(initial=0.0))
    ml = float(max(1, (c["M"] != 0).sum(axis=1).max(initial=1)))
    return R.fixed_scale(vm, vm * ml)


def fixed_point_shift(A, y, steps, ref, weights="f32", patterns=4):
    """F_j per quantity: the largest change of the state when every step's Hessian is moved by a dH of the fixed-point
    sum's entry-wise bound, over `patterns` seeded symmetric sign patterns"""
    c = A if isinstance(A, dict) else reduced(A)
    zero = [{q: 0.0 for q in QUANT} for _ in range(len(ref))]
    if c["empty"] or c["p"] == 0:
        return zero
    scale = hessian_scale(c)
    out = zero
    for t in range(patterns):
        rng = np.random.default_rng([77, t, c["p"], c["d"]])

        def dH(step, H, dr):
            n, mx = hessian_terms(c["M"], dr)
            mag = n * (0.5 / scale + R.U * mx)
            sg = np.triu(rng.choice([-1.0, 1.0], size=H.shape))
            sg = sg + np.triu(sg, 1).T
            return sg * mag

        st = iterate(c, y, steps, weights, dH=dH)
        out = [{q: max(out[j][q], _dev(st[j][q], ref[j][q])) for q in QUANT} for j in range(len(ref))]
    return out


# ------------------------------------------------------------------------------------------------ outputs and bounds
U32 = 2.0 ** -24
TWIN_FACTOR = 8.0   # eight twins sample the drift between correct double realisations; they do not bound it


def outputs(c, y, state, sign=-1.0):
    """the five float outputs of the mode from a state of the reference, before their rounding to float, and the scale
    of the epilogue's own accumulated error (ops_ref.epilogue) -> (values, scales)"""
    return R.epilogue(R.MODE_IPM, sign, 0.0, bool(c["empty"]), y, L._f64(state["rho"]), float(state["f"]),
                      L._f64(c["avg"]).astype(np.float32))


def output_bounds(c, y, state, E, sign=-1.0):
    """|float output - reference| <= these, E = {"proj": E_k, "rnorm": E_k} the bound of the double state.
    proj, rnorm: 2^-24 |ref| (the rounding to float; 2^-149, the spacing of the subnormal floats, where that is smaller:
    the zero prediction has proj ~ 1e-150) + d u scale (ops_ref: the epilogue's sums) + E.
    target = p / |p|, p the float-rounded projection: a change dp of p moves it by at most 2 |dp|_2 / |p|_2, and
    |dp|_2 <= sqrt(d) E: G = 2 sqrt(d) E / max(|p|_2, 1e-8).  loss = 1 - cos(y, target) moves by at most
    2 |dt|_2 / |t|_2 <= 2 sqrt(d) G; grad's two terms are 1 / (|y| |t|) times unit-sized vectors: 4 sqrt(d) G times
    its scale.  All three keep the epilogue's own bound beside it."""
    vals, scale = outputs(c, y, state, sign)
    d = len(y)
    out = {}
    pn = float(np.sqrt((L._f64(vals["proj"]).astype(np.float32).astype(np.float64) ** 2).sum()))
    G = 2.0 * np.sqrt(d) * E["proj"] / max(pn, R.NORM_CLAMP)
    extra = {"proj": E["proj"], "rnorm": E["rnorm"], "target": G, "loss": 2.0 * np.sqrt(d) * G,
             "grad": 4.0 * np.sqrt(d) * G * scale["grad"]}
    for k in ("proj", "rnorm", "target", "loss", "grad"):
        ref = np.atleast_1d(L._f64(vals[k]))
        out[k] = U32 * np.abs(ref) + 2.0 ** -149 + d * R.U * scale[k] + extra[k]
    return vals, out
