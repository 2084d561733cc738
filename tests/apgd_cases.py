"""Cases of the APGD projector shared by the CPU tier (tests/test_apgd_emul.py, the SIMT emulation) and the GPU tier
(tests/test_gpu_apgd.py, the C ABI): the fixture inputs, the shape cases, and the comparisons against tests/apgd_ref.py.

A runner is `run(cones, pred, **kw) -> (rc, outputs dict)` as `emul_apgd_lib.SimtApgd.run` defines it; `gpu_run` is the
same over cave_hip_cone_apgd / cave_hip_cone_apgd_sparse.  `cones`: a dense (B, m, d) float32 array, or the sparse triple
(m, d, ent_off, key, val).
"""

from __future__ import annotations

import functools
import os

import numpy as np

import apgd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SNAP = R.SNAP
FLOAT_OUT = ("proj", "rnorm", "target", "loss", "grad")
STATE_OUT = ("x_curr", "x_prev", "step", "pgrad")
ALL_OUT = FLOAT_OUT + STATE_OUT + ("status", "iters")
ST_OK, ST_TOO_LARGE, ST_BAD_INPUT = 0, 2, 3


@functools.lru_cache(maxsize=None)
def fixture_inputs():
    """name -> (ctrs (B, m, d) float32, pred (B, d) float32, sign): regenerated from seeds, not stored"""
    import torch

    from cave_amd import synth

    out = {}
    for name, (c, y, _) in (("tsp20", synth.tsp_batch(20, 16, seed=0)), ("tsp10", synth.tsp_batch(10, 16, seed=1)),
                            ("sp5", synth.sp_batch(5, 5, 16, seed=0))):
        out[name] = (np.ascontiguousarray(c, np.float32), np.ascontiguousarray(y, np.float32), -1.0)
    torch.manual_seed(1)
    c, y = torch.randn(8, 15, 10), torch.randn(8, 10)
    out["randn"] = (c.numpy().copy(), y.numpy().copy(), 1.0)
    torch.manual_seed(0)  # the data of the reference's TestAPGD.setUp (test/test_func.py:235-243), MINIMIZE
    y = torch.rand(8, 10)
    c = torch.rand(8, 15, 10)
    out["setup"] = (c.numpy().copy(), y.numpy().copy(), -1.0)
    return out


@functools.lru_cache(maxsize=None)
def converged_input():
    from cave_amd import synth

    c, y, _ = synth.sp_batch(5, 5, 8, seed=0)
    return np.ascontiguousarray(c, np.float32), np.ascontiguousarray(y, np.float32), -1.0


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "apgd.npz")))


def to_sparse(A):
    """dense (B, m, d) -> the sparse triple (m, d, ent_off, key, val)"""
    B, m, d = A.shape
    off, keys, vals = [0], [], []
    for b in range(B):
        r, c = np.nonzero(A[b])
        keys.append(((r.astype(np.int64) << 16) | c).astype(np.uint32))
        vals.append(A[b][r, c].astype(np.float32))
        off.append(off[-1] + len(r))
    return (m, d, np.asarray(off, np.int64), np.concatenate(keys) if keys else np.zeros(0, np.uint32),
            np.concatenate(vals) if vals else np.zeros(0, np.float32))


def max_nnz(A):
    return int(max(1, (A != 0).reshape(A.shape[0], -1).sum(axis=1).max())) if A.shape[0] else 1


# ---- shape cases: small, every path.  name -> (A, pred, sign)
@functools.lru_cache(maxsize=None)
def shape_cases():
    rng = np.random.default_rng(7)
    cases = {}

    def rand(B, m, d, dens):
        A = (rng.standard_normal((B, m, d)) * (rng.random((B, m, d)) < dens)).astype(np.float32)
        return A, rng.standard_normal((B, d)).astype(np.float32)

    for m in (1, 63, 64, 65, 257):
        for d in (1, 2, 70):
            cases[f"m{m}_d{d}"] = rand(3, m, d, 0.3 if d > 2 else 0.8) + (1.0 if (m + d) & 1 else -1.0,)
    A, y = rand(4, 9, 12, 0.4)
    A[1] = 0                      # an empty cone
    A[2, 3:] = 0                  # padding rows
    A[3, :, 5] = 0                # a column without entries
    cases["empty_padding_nocol"] = (A, y, -1.0)
    A = np.zeros((2, 80, 70), np.float32)   # a dense 70-entry row beside unit rows
    A[:, 0, :] = rng.standard_normal((2, 70)).astype(np.float32)
    for k in range(70):
        A[:, 1 + k, k] = 1.0 if k & 1 else -1.0
    cases["dense_row_units"] = (A, rng.standard_normal((2, 70)).astype(np.float32), 1.0)
    A, y = rand(2, 6, 8, 0.6)               # exact +a/-a pairs and repeated rows
    A = np.concatenate([A, -A, A[:, :2]], axis=1)
    cases["pairs_repeats"] = (A, y, -1.0)
    # few entries in a large block: one wave by the capacity rule with several rows per lane, and four waves are one
    # capacity away (the GPU tier reaches the other workgroup size through nnz_cap)
    for m, d in ((257, 70), (65, 70), (64, 2)):
        cases[f"m{m}_d{d}_thin"] = rand(3, m, d, 0.02 if d > 2 else 0.5) + (-1.0,)
    return cases


@functools.lru_cache(maxsize=None)
def reference(name, n_iter, power_iter=8):
    """(long-double restatement with snapshots, S) of a shape case"""
    A, y, sign = shape_cases()[name]
    ref = R.run(A, y, sign, n_iter, power_iter)
    S = R.spread(ref, R.twins(A, y, sign, n_iter, power_iter))
    return ref, S


def check_against(o, ref, S, mode_exact=True, ok=None, margins=None, tag=""):
    """every output of a launch against the restatement `ref` within the derived bounds; -> the largest ratio reached"""
    worst = 0.0
    B = o["status"].shape[0]
    ok = np.ones(B, bool) if ok is None else ok
    assert (o["status"][ok] == ST_OK).all(), (tag, o["status"])
    for name in FLOAT_OUT if mode_exact else ("proj", "rnorm"):
        dev = np.abs(o[name].astype(np.float64) - np.asarray(getattr(ref, name), np.float64))
        bound = R.float_bound(ref, name, S) + np.spacing(np.abs(np.asarray(getattr(ref, name), np.float64)))
        ratio = (dev / np.maximum(bound, 1e-300))[ok]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert (dev[ok] <= bound[ok]).all(), (tag, name, float(ratio.max()))
    for name in STATE_OUT:
        if o.get(name) is None:
            continue
        dev = np.abs(o[name].astype(R.LD) - getattr(ref, name)).astype(np.float64)
        bound = R.state_bound(ref, name, S)
        ratio = (dev / np.maximum(bound, 1e-300))[ok]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert (dev[ok] <= bound[ok]).all(), (tag, name, float(ratio.max()))
    if margins is not None:
        margins[tag] = worst
    return worst


def same_bits(a, b, names=ALL_OUT, rows=None):
    for n in names:
        if a.get(n) is None or b.get(n) is None:
            continue
        x, y = (a[n], b[n]) if rows is None else (a[n][rows[0]], b[n][rows[1]])
        assert x.tobytes() == y.tobytes(), n


def fixture_ref(name, k, rows=slice(None)):
    """the stored long-double restatement of a fixture input (its instances `rows`) after k iterations as a Result-like
    object (float64), and S"""
    f = fixture()
    A, y, sign = fixture_inputs()[name] if name != "conv" else converged_input()
    y = y[rows]
    r = R.Result()
    p = f[f"{name}_{k}_ld_proj"][rows]
    r.proj, r.rnorm, r.loss, r.pgrad = p, f[f"{name}_{k}_ld_rnorm"][rows], f[f"{name}_{k}_ld_loss"][rows], f[f"{name}_{k}_ld_pgrad"][rows]
    r.gscale = f[f"{name}_{k}_ld_gscale"][rows]
    # target and gradient follow from the projection in closed form (fp64 is ample beside their float32 bounds)
    yv = sign * y.astype(np.float64)
    r.yscale = np.linalg.norm(yv, axis=1)
    t = p / np.maximum(np.linalg.norm(p, axis=1), 1e-8)[:, None]
    r.target = t
    t = t.astype(np.float32).astype(np.float64)
    ns, nt = np.linalg.norm(yv, axis=1), np.linalg.norm(t, axis=1)
    ns_c, nt_c = np.maximum(ns, 1e-8), np.maximum(nt, 1e-8)
    st = (yv * t).sum(axis=1)
    radial = np.where(ns > 1e-8, st / (ns_c * ns_c * np.where(ns > 0, ns, 1) * nt_c), 0)
    r.grad = -sign * (t / (ns_c * nt_c)[:, None] - radial[:, None] * yv)
    return r, float(f[f"{name}_{k}_S"])


def check_fixture_floats(o, name, k, mode_exact=True, tag="", rows=slice(None)):
    """float outputs against the stored restatement (2^-24 |ref| + 8 S) and against the reference's fp32 run
    (|ref32 - ref64| + 2^-24 |ref64| + 8 S); -> the largest ratio"""
    f = fixture()
    ref, S = fixture_ref(name, k, rows)
    worst = 0.0
    assert (o["status"] == ST_OK).all()
    for n in FLOAT_OUT if mode_exact else ("proj", "rnorm"):
        rv = np.asarray(getattr(ref, n), np.float64)
        dev = np.abs(o[n].astype(np.float64) - rv)
        # (the stored restatement is the long-double result rounded to double: one ulp of it is part of the bound)
        bound = R.float_bound(ref, n, S) + np.spacing(np.abs(rv))
        assert (dev <= bound).all(), (tag, name, k, n, float((dev / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((dev / np.maximum(bound, 1e-300)).max()))
    p32, p64 = f[f"{name}_{k}_ref32_proj"][rows].astype(np.float64), f[f"{name}_{k}_ref64_proj"][rows]
    sc = np.abs(p64).max(axis=1)[:, None]
    bound = np.abs(p32 - p64) + R.EPS32 * np.abs(p64) + 8 * S * sc
    dev = np.abs(o["proj"].astype(np.float64) - p32)
    assert (dev <= bound).all(), (tag, name, k, "proj vs fp32 reference", float((dev / np.maximum(bound, 1e-300)).max()))
    worst = max(worst, float((dev / np.maximum(bound, 1e-300)).max()))
    return worst


# ---- the GPU runner: the C ABI itself
def gpu_run(cones, pred, mode=1, sign=1.0, n_iter=20, power_iter=8, cap=None, k_start=0, state=None, want_state=True, **_):
    import ctypes as C

    import torch

    from cave_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda")
    sparse = not isinstance(cones, np.ndarray)
    if sparse:
        m, d, ent_off, key, val = cones
        B = len(ent_off) - 1
        t = (torch.tensor(np.asarray(ent_off, np.int64), device=dev), torch.tensor(np.asarray(key, np.uint32).view(np.int32), device=dev),
             torch.tensor(np.asarray(val, np.float32), device=dev))
        c = _lib.SparseConesC(B=B, m_max=m, d=d, ent_off=t[0].data_ptr(), key=t[1].data_ptr() if len(key) else 8,
                              val=t[2].data_ptr() if len(key) else 8)
    else:
        B, m, d = cones.shape
        t = torch.tensor(np.ascontiguousarray(cones, np.float32), device=dev)
    p = torch.tensor(np.ascontiguousarray(pred, np.float32), device=dev)
    if cap is None:
        cap = m * d
    o = {n: torch.full((B, d) if n in ("proj", "target", "grad") else (B,), 77.0, dtype=torch.float32, device=dev) for n in FLOAT_OUT}
    o["status"] = torch.full((B,), -7, dtype=torch.int32, device=dev)
    o["iters"] = torch.full((B,), -7, dtype=torch.int32, device=dev)
    o["pgrad"] = torch.full((B,), 77.0, dtype=torch.float64, device=dev)
    if state is not None:
        o["x_curr"], o["x_prev"], o["step"] = (torch.tensor(np.asarray(a, np.float64), device=dev) for a in state)
    elif want_state:
        o["x_curr"] = torch.full((B, m), 77.0, dtype=torch.float64, device=dev)
        o["x_prev"] = torch.full((B, m), 77.0, dtype=torch.float64, device=dev)
        o["step"] = torch.full((B,), 77.0, dtype=torch.float64, device=dev)
    ptr = _lib.ptr
    tail = (mode, sign, k_start, n_iter, power_iter, cap, *(ptr(o.get(n)) for n in ("x_curr", "x_prev", "step", "proj", "rnorm", "target",
                                                                                      "loss", "grad", "status", "iters", "pgrad")),
            _lib.current_stream())
    rc = lib.cave_hip_cone_apgd_sparse(C.byref(c), ptr(p), *tail) if sparse else lib.cave_hip_cone_apgd(ptr(t), ptr(p), B, m, d, *tail)
    torch.cuda.synchronize()
    return int(rc), {k: v.cpu().numpy() for k, v in o.items()}
