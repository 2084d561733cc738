"""GPU tier of the APGD projector: cave_hip_cone_apgd / cave_hip_cone_apgd_sparse through the C ABI, the host layer
(qpsolver.project_apgd_hip) and the module route (inner='apgd'), against the long-double restatement (tests/apgd_ref.py)
within the derived bounds and against the unmodified reference's fp32 / fp64 runs (tests/golden/apgd.npz).  The cases are
those of the CPU tier (tests/apgd_cases.py).  With CAVE_APGD_MARGINS=<path> the largest ratio each check reached is
written there as JSON (profiles/apgd_margins.json)."""

import json
import os

import numpy as np
import pytest

import apgd_cases as AC
import apgd_ref as R

pytestmark = pytest.mark.gpu
run = AC.gpu_run
MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _margins():
    yield
    path = os.environ.get("CAVE_APGD_MARGINS")
    if path:
        with open(path, "w") as fh:
            json.dump({"what": "largest deviation / bound reached per check of tests/test_gpu_apgd.py (1 = at the bound)",
                       "ratios": MARGINS}, fh, indent=1, sort_keys=True)


@pytest.mark.parametrize("name", ["tsp20", "tsp10", "sp5", "randn", "setup"])
def test_fixture_inputs_at_every_stored_count(name):
    A, y, sign = AC.fixture_inputs()[name]
    cap = AC.max_nnz(A)
    for k in AC.SNAP:
        rc, o = run(A, y, sign=sign, n_iter=k, cap=cap)
        assert rc == 0
        MARGINS[f"fixture/{name}/{k}"] = AC.check_fixture_floats(o, name, k, tag="gpu")
        ref, S = AC.fixture_ref(name, k)
        dev = np.abs(o["pgrad"] - ref.pgrad)
        assert (dev <= R.state_bound(ref, "pgrad", S)).all(), (name, k, "pgrad")
    rc, s = run(AC.to_sparse(A), y, sign=sign, n_iter=AC.SNAP[-1], cap=cap)
    AC.same_bits(o, s)
    if name == "setup":  # the projection is exactly zero: target 0, loss 1
        assert not o["proj"].any() and not o["target"].any() and (o["loss"] == 1.0).all() and (o["rnorm"] > 0).all()


@pytest.mark.parametrize("name", sorted(AC.shape_cases()))
def test_shapes_against_restatement(name):
    A, y, sign = AC.shape_cases()[name]
    B, m, d = A.shape
    ref, S = AC.reference(name, 20)
    cap = AC.max_nnz(A)
    rc, o = run(A, y, sign=sign, n_iter=20, cap=cap)
    assert rc == 0
    AC.check_against(o, ref, S, tag=f"shape/{name}", margins=MARGINS)
    rc, s = run(AC.to_sparse(A), y, sign=sign, n_iter=20, cap=cap)
    AC.same_bits(o, s)           # format agreement
    rc, again = run(A, y, sign=sign, n_iter=20, cap=cap)
    AC.same_bits(o, again)       # relaunch
    other = 513 if cap <= 512 else 512   # the other workgroup size, through the entry capacity
    if cap <= other <= m * d and m <= 512 and d <= 512:
        rc, w = run(A, y, sign=sign, n_iter=20, cap=other)
        assert rc == 0
        AC.check_against(w, ref, S, tag=f"shape/{name}/other-size", margins=MARGINS)
        AC.same_bits(o, w)


@pytest.mark.parametrize("name", ["m65_d70", "m1_d2", "pairs_repeats"])
def test_power_iter_zero_and_project_mode(name):
    A, y, sign = AC.shape_cases()[name]
    ref, S = AC.reference(name, 20, 0)
    rc, o = run(A, y, sign=sign, n_iter=20, power_iter=0)
    assert rc == 0
    AC.check_against(o, ref, S, tag=f"power0/{name}", margins=MARGINS)
    rc, p = run(A, y, mode=0, sign=sign, n_iter=20, power_iter=0)
    AC.same_bits(o, p, ("proj", "rnorm", "x_curr", "x_prev", "step", "pgrad", "status", "iters"))
    for n in ("target", "loss", "grad"):
        assert (p[n] == 77.0).all()


def test_capacity_exact_and_one_over():
    rng = np.random.default_rng(3)
    A = np.zeros((3, 9, 12), np.float32)
    for b, nnz in enumerate((20, 21, 7)):
        idx = rng.choice(9 * 12, nnz, replace=False)
        A[b].reshape(-1)[idx] = rng.standard_normal(nnz).astype(np.float32)
    y = rng.standard_normal((3, 12)).astype(np.float32)
    for cones, rest in ((A, A[[0, 2]]), (AC.to_sparse(A), AC.to_sparse(A[[0, 2]]))):
        rc, o = run(cones, y, n_iter=10, cap=20)
        assert rc == 0 and list(o["status"]) == [0, AC.ST_TOO_LARGE, 0] and o["iters"][1] == 0
        for n in AC.FLOAT_OUT + ("pgrad",):
            assert np.isnan(o[n][1]).all(), n
        assert (o["x_curr"][1] == 77.0).all() and o["step"][1] == 77.0
        rc, r = run(rest, y[[0, 2]], n_iter=10, cap=20)
        AC.same_bits(o, r, rows=([0, 2], [0, 1]))
        rc, full = run(cones, y, n_iter=10, cap=21)
        assert rc == 0 and (full["status"] == 0).all()
        AC.same_bits(o, full, rows=([0, 2], [0, 2]))


def test_bad_input_per_instance():
    A, y, sign = AC.shape_cases()["empty_padding_nocol"]
    m, d, off, key, val = AC.to_sparse(A)
    rc, good = run((m, d, off, key, val), y, n_iter=5)
    assert rc == 0 and (good["status"] == 0).all()

    def expect_bad(cones, pred, b):
        rc, o = run(cones, pred, n_iter=5)
        assert rc == 0 and o["status"][b] == AC.ST_BAD_INPUT and np.isnan(o["proj"][b]).all() and np.isnan(o["pgrad"][b])
        keep = [i for i in range(len(o["status"])) if i != b]
        AC.same_bits(o, good, AC.FLOAT_OUT + ("pgrad", "status"), rows=(keep, keep))

    k2 = key.copy(); k2[1] = (m << 16) | 0               # a row out of range
    expect_bad((m, d, off, k2, val), y, 0)
    k2 = key.copy(); k2[0] = (int(key[0]) & 0xffff0000) | d  # a column out of range
    expect_bad((m, d, off, k2, val), y, 0)
    k2 = key.copy(); k2[1], k2[2] = key[2], key[1]       # unsorted
    expect_bad((m, d, off, k2, val), y, 0)
    for bad in (np.inf, np.nan):                         # a non-finite value
        v2 = val.copy(); v2[int(off[2])] = bad
        expect_bad((m, d, off, key, v2), y, 2)
    y2 = y.copy(); y2[3, 1] = np.nan                     # a non-finite prediction, both formats
    expect_bad((m, d, off, key, val), y2, 3)
    expect_bad(A, y2, 3)
    A2 = A.copy(); A2[0, 0, 0] = -np.inf                 # a non-finite dense entry
    expect_bad(A2, y, 0)


def test_argument_errors_and_their_texts():
    import torch

    from cave_amd import _lib

    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    none11 = [None] * 11

    def err(text, ctrs=p, pred=p, dims=(2, 3, 4), mode=1, sign=1.0, k_start=0, n_iter=5, power_iter=8, cap=12, ptrs=none11):
        rc = lib.cave_hip_cone_apgd(ctrs, pred, *dims, mode, sign, k_start, n_iter, power_iter, cap, *ptrs, None)
        assert rc == -1 and text in lib.cave_hip_last_error().decode(), (text, rc, lib.cave_hip_last_error())

    assert lib.cave_hip_cone_apgd(None, None, 0, 0, 0, 9, 0.0, -1, -1, -1, -1, *none11, None) == 0  # B == 0 before anything else
    err("bad B", dims=(-1, 3, 4))
    err("bad shape", dims=(2, 0, 4)); err("bad shape", dims=(2, 3, 65536))
    for mode in (2, 3, 4, 5, 6, -1):
        err("bad mode", mode=mode)
    err("sign must be", sign=0.5)
    err("bad k_start", k_start=-1); err("bad k_start", k_start=2 ** 30 + 1)
    err("bad n_iter", n_iter=-1); err("bad n_iter", n_iter=100001)
    err("bad power_iter", power_iter=-1); err("bad power_iter", power_iter=65)
    err("bad nnz_cap", cap=0); err("bad nnz_cap", cap=13)
    err("exceeds 160 KiB", dims=(2, 235, 190), cap=235 * 190)
    err("null or misaligned pred", pred=None)
    err("null or misaligned ctrs", ctrs=None); err("null or misaligned ctrs", ctrs=p + 2)
    err("go together", ptrs=[p, None, p] + [None] * 8)
    err("continuation", k_start=3)
    err("batch too large", dims=(2 ** 31, 3, 4))  # (refused before anything is read or launched)
    err("misaligned x_curr", ptrs=[p + 4, p, p] + [None] * 8)
    err("misaligned pgrad", ptrs=[None] * 10 + [p + 4])
    rc = lib.cave_hip_cone_apgd_sparse(None, p, 1, 1.0, 0, 5, 8, 12, *none11, None)
    assert rc == -1 and b"cones is null" in lib.cave_hip_last_error()
    import ctypes as C

    c = _lib.SparseConesC(B=2, m_max=3, d=4, ent_off=0, key=p, val=p)
    rc = lib.cave_hip_cone_apgd_sparse(C.byref(c), p, 1, 1.0, 0, 5, 8, 12, *none11, None)
    assert rc == -1 and b"null or misaligned ent_off" in lib.cave_hip_last_error()
    assert lib.cave_hip_apgd_lds_bytes(235, 190, 1200) == 27280 and lib.cave_hip_apgd_lds_bytes(235, 190, 235 * 190) == -1


def test_batch_independence_and_the_large_batch():
    A, y, sign = AC.fixture_inputs()["tsp20"]
    cap = AC.max_nnz(A)
    rc, o = run(A, y, sign=sign, n_iter=20, cap=cap)
    perm = [4, 0, 15]
    rc, p = run(A[perm], y[perm], sign=sign, n_iter=20, cap=cap)
    AC.same_bits(o, p, rows=(perm, [0, 1, 2]))
    rc, one = run(A[3:4], y[3:4], sign=sign, n_iter=20, cap=cap)
    AC.same_bits(o, one, rows=([3], [0]))
    # TSP-20 at B = 1024, the one large case: every copy of an instance gives the bits of the batch of 16
    reps = 64
    rc, big = run(np.tile(A, (reps, 1, 1)), np.tile(y, (reps, 1)), sign=sign, n_iter=20, cap=cap)
    assert rc == 0 and (big["status"] == 0).all()
    for n in AC.FLOAT_OUT + AC.STATE_OUT:
        assert big[n].tobytes() == np.tile(o[n], (reps,) + (1,) * (o[n].ndim - 1)).tobytes(), n


@pytest.mark.parametrize("name,split", [("sp5", (1, 199)), ("sp5", (200, 200)), ("tsp20", (1, 199)), ("tsp20", (200, 200))])
def test_continuation(name, split):
    A, y, sign = AC.fixture_inputs()[name]
    cap = AC.max_nnz(A)
    rc, whole = run(A, y, sign=sign, n_iter=sum(split), cap=cap)
    rc, a = run(A, y, sign=sign, n_iter=split[0], cap=cap)
    rc, b = run(A, y, sign=sign, n_iter=split[1], k_start=split[0], cap=cap, state=(a["x_curr"], a["x_prev"], a["step"]))
    assert rc == 0
    AC.same_bits(whole, b, AC.FLOAT_OUT + AC.STATE_OUT + ("status",))
    assert (b["iters"] == split[1]).all()
    rc, n = run(A, y, sign=sign, n_iter=sum(split), cap=cap, want_state=False)  # the state may be null for a single launch
    AC.same_bits(whole, n, AC.FLOAT_OUT + ("pgrad", "status", "iters"))


# ------------------------------------------------------------------------------------------------ host layer
@pytest.mark.parametrize("name", ["tsp20", "tsp10", "sp5", "randn", "setup"])
def test_project_apgd_hip_without_tolerance(name):
    import torch

    from cave_amd import qpsolver
    from cave_amd.sparse import SparseCones

    A, y, sign = AC.fixture_inputs()[name]
    f = AC.fixture()
    signed = torch.tensor(sign * y, device="cuda")
    for k in (3, 200, 400):
        info = {}
        proj, rn = qpsolver.project_apgd_hip(torch.tensor(A, device="cuda"), signed, tol_grad=None, max_iters=k, info=info)
        assert info == {"chunks": max(1, -(-k // 200)), "pgrad": []} and proj.dtype == torch.float32
        o = {"proj": proj.cpu().numpy(), "status": np.zeros(len(A), np.int32)}
        ref, S = AC.fixture_ref(name, k)
        p32, p64 = f[f"{name}_{k}_ref32_proj"].astype(np.float64), f[f"{name}_{k}_ref64_proj"]
        bound = np.abs(p32 - p64) + R.EPS32 * np.abs(p64) + 8 * S * np.abs(p64).max(axis=1)[:, None]
        assert (np.abs(o["proj"] - p32) <= bound).all(), (name, k)
        assert (np.abs(o["proj"] - ref.proj) <= R.float_bound(ref, "proj", S) + np.spacing(np.abs(ref.proj))).all()
    ps, rs = qpsolver.project_apgd_hip(SparseCones.from_dense(A).cuda(), signed, tol_grad=None, max_iters=400)
    assert torch.equal(ps, proj) and torch.equal(rs, rn)
    pu, ru = qpsolver.project_apgd_hip(torch.tensor(A, device="cuda"), signed, tol_grad=None, max_iters=400, check=False)
    assert torch.equal(pu, proj) and torch.equal(ru, rn)  # (no host read at all; the shape's capacity has settled above)


def test_project_apgd_hip_converged_record():
    """the reference's stopping rule: the same chunk count, proj within the fp32-fixture bound, the squared rnorm within
    the propagated bound.  (The squared rnorm is the square of the float32 un-squared output: 2^-23 r64 is that output's
    rounding, squared; it is asked for in float64 here, since one more rounding to float32 is not part of the bound.)"""
    import torch

    from cave_amd import qpsolver

    A, y, sign = AC.converged_input()
    f = AC.fixture()
    chunks = int(f["conv_chunks"])
    signed = torch.tensor(sign * y, device="cuda")
    info = {}
    proj, rn = qpsolver.project_apgd_hip(torch.tensor(A, device="cuda"), signed.double(), info=info)
    got_chunks, seen = info["chunks"], info["pgrad"]
    assert got_chunks == chunks == len(seen) and seen[-1] <= 1e-4 < seen[0]
    ref, S = AC.fixture_ref("conv", 200 * chunks)
    for j, s in enumerate(seen):  # the check quantity per chunk against the reference's fp64 run and the restatement
        r, Sj = AC.fixture_ref("conv", 200 * (j + 1))
        assert abs(s - r.pgrad.max()) <= R.state_bound(r, "pgrad", Sj).max()
        assert abs(s - f["conv_ref64_pgrad"][j]) <= 1e-3 * f["conv_ref64_pgrad"][j]
    p32, p64 = f["conv_ref32_proj"].astype(np.float64), f["conv_ref64_proj"]
    bound = np.abs(p32 - p64) + R.EPS32 * np.abs(p64) + 8 * S * np.abs(p64).max(axis=1)[:, None]
    dev = np.abs(proj.cpu().numpy() - p32)
    MARGINS["converged/proj"] = float((dev / bound).max())
    assert (dev <= bound).all()
    r32, r64 = f["conv_ref32_rn"].astype(np.float64), f["conv_ref64_rn"]
    bound = np.abs(r32 - r64) + 2.0 ** -23 * r64 + 2 * np.sqrt(r64) * 8 * S * ref.yscale
    dev = np.abs(rn.cpu().numpy() - r32)
    MARGINS["converged/rnorm_squared"] = float((dev / bound).max())
    assert rn.dtype == torch.float64 and (dev <= bound).all(), (dev / bound).max()


def test_dense_capacity_settles_and_names_the_limit():
    import torch

    from cave_amd import qpsolver

    rng = np.random.default_rng(2)
    A = rng.standard_normal((2, 40, 30)).astype(np.float32)  # full rows: 1200 entries, beyond the first guess (274)
    y = rng.standard_normal((2, 30)).astype(np.float32)
    qpsolver._apgd_cap.pop((40, 30), None)
    o = qpsolver.cone_op_apgd(torch.tensor(A, device="cuda"), torch.tensor(y, device="cuda"), n_iter=5)
    assert qpsolver._apgd_cap[(40, 30)] == qpsolver.apgd_full_cap(40, 30) == 1200 and bool((o["status"] == 0).all())
    rc, ref = run(A, y, mode=0, n_iter=5)
    assert np.array_equal(o["proj"].cpu().numpy(), ref["proj"])
    u = qpsolver.cone_op_apgd(torch.tensor(A, device="cuda"), torch.tensor(y, device="cuda"), n_iter=5, nnz_cap=100, check=False)
    assert bool((u["status"] == AC.ST_TOO_LARGE).all()) and bool(torch.isnan(u["proj"]).all())
    big = np.ones((1, 300, 300), np.float32)  # 90 000 entries: beyond any arena
    with pytest.raises(qpsolver.HipSolverError, match="non-zeros does not fit the 160 KiB LDS arena"):
        qpsolver.cone_op_apgd(torch.tensor(big, device="cuda"), torch.ones(1, 300, device="cuda"), n_iter=1)


# ------------------------------------------------------------------------------------------------ module route
class _Model:
    def __init__(self, sense):
        self.modelSense = sense


def _ref_loss_and_grad(name, k, pred, sign, rows=slice(None)):
    """autograd of 1 - cos(sign * pred, target_ref64) with the restatement's float32 target"""
    import torch

    ref, S = AC.fixture_ref(name, k, rows)
    t = torch.tensor(ref.target.astype(np.float32).astype(np.float64))
    p = torch.tensor(pred.astype(np.float64), requires_grad=True)
    loss = 1 - torch.nn.functional.cosine_similarity(sign * p, t, dim=1)
    return loss, p, S


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_module_route_loss_and_gradient(reduction):
    import torch

    from cave_amd.cave import EPO, innerConeAlignedCosine

    A, y, sign = AC.fixture_inputs()["sp5"]
    mod = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", solver_kwargs={"inner": "apgd", "max_iters": 20},
                                 max_iter=7, reduction=reduction, seed=0)
    pred = torch.tensor(y, device="cuda", requires_grad=True)
    loss = mod(pred, torch.tensor(A, device="cuda"))
    w = torch.arange(1, len(A) + 1, dtype=torch.float32, device="cuda")
    (loss * w).sum().backward() if reduction == "none" else loss.backward()
    rl, rp, S = _ref_loss_and_grad("sp5", 20, y, sign)
    red = {"mean": rl.mean, "sum": rl.sum, "none": lambda: rl}[reduction]()
    (red * w.cpu().double()).sum().backward() if reduction == "none" else red.backward()
    # Bounds.  The kernel's loss_b and grad_b are float32 roundings of fp64 values that agree with the restatement's to
    # 8 S: 2^-24 |.| + 8 S each.  'none': that is all for the loss; the gradient is multiplied by its weight in float32,
    # one more rounding.  'sum' / 'mean': a float32 sum of n terms in any order adds at most (n - 1) 2^-24 sum|l_b|, the
    # mean one rounding for the division; their gradient is grad_b times 1 or 1/n in float32, one more rounding.
    # (1 + 2^-20 covers the second-order terms.)
    n, u, so = len(A), 2.0 ** -24, 1 + 2.0 ** -20
    l_ref = rl.detach().numpy()
    dev_l = np.abs(loss.detach().cpu().numpy() - red.detach().numpy())
    if reduction == "none":
        assert (dev_l <= so * u * np.abs(l_ref) + 8 * S).all()
    else:
        div = n if reduction == "mean" else 1
        assert dev_l <= so * (n + 1) * u * np.abs(l_ref).sum() / div + 8 * S * n / div
    # The gradient is a difference of two terms of magnitude at most weight_b / ||y_b||: that is what its 8 S is relative to.
    g_ref = rp.grad.numpy()
    weight = {"mean": np.full((n, 1), 1.0 / n), "sum": np.ones((n, 1)), "none": w.cpu().numpy().astype(np.float64)[:, None]}[reduction]
    scale = weight / np.linalg.norm(y.astype(np.float64), axis=1, keepdims=True)
    assert (np.abs(pred.grad.cpu().numpy() - g_ref) <= so * 2 * u * np.abs(g_ref) + 8 * S * scale).all()


def test_module_route_senses_formats_and_errors():
    import torch

    from cave_amd import cave, qpsolver
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.dataset import ConeStore
    from cave_amd.sparse import SparseCones

    A, y, _ = AC.fixture_inputs()["tsp10"]
    ctrs = torch.tensor(A, device="cuda")
    kw = {"inner": "apgd", "max_iters": 40, "check_frequency": 25, "power_iter": 8, "tol_grad": None}
    out = {}
    for sense, sign in ((EPO.MINIMIZE, -1.0), (EPO.MAXIMIZE, 1.0)):
        mod = innerConeAlignedCosine(_Model(sense), solver="hip", solver_kwargs=dict(kw), reduction="none", seed=0)
        pred = torch.tensor(y, device="cuda", requires_grad=True)
        loss = mod(pred, ctrs)
        loss.sum().backward()
        rc, o = run(A, y, sign=sign, n_iter=40, cap=AC.max_nnz(A))  # chunks of 25 + 15 equal the single launch
        assert np.array_equal(loss.detach().cpu().numpy(), o["loss"]) and np.array_equal(pred.grad.cpu().numpy(), o["grad"])
        out[sign] = loss.detach()
        for other in (SparseCones.from_dense(A).cuda(), qpsolver.prepare_cones(ctrs)):  # SparseCones; PreparedCones unwrapped
            assert torch.equal(mod(torch.tensor(y, device="cuda"), other), out[sign])
        tgt = mod._get_projection(torch.tensor(sign * y, device="cuda"), ctrs)
        assert np.array_equal(tgt.cpu().numpy(), o["target"])
    assert not torch.equal(out[-1.0], out[1.0])
    from cave_amd.dataset import PackedBatch

    with pytest.raises(ValueError, match="reduced cones"):
        mod(torch.tensor(y, device="cuda"), PackedBatch(ConeStore.from_dense(ctrs), torch.arange(len(A), device="cuda")))
    # the hybrid's heuristic branch is unchanged: the new keys never reach an existing entry
    hyb = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", solver_kwargs=dict(kw), solve_ratio=0.0, reduction="none", seed=0)
    plain = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", solve_ratio=0.0, reduction="none", seed=0)
    assert torch.equal(hyb(torch.tensor(y, device="cuda"), ctrs), plain(torch.tensor(y, device="cuda"), ctrs))
    with pytest.raises(ImportError):
        innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="apgd")
    with pytest.raises(ValueError, match="'push', 'ipm' or 'apgd'"):
        innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", solver_kwargs={"inner": "bogus"})


def test_module_route_tolerance_stops_like_the_reference():
    import torch

    from cave_amd import qpsolver
    from cave_amd.cave import EPO, innerConeAlignedCosine

    A, y, sign = AC.converged_input()
    mod = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none", seed=0,
                                 solver_kwargs={"inner": "apgd", "max_iters": None, "tol_grad": 1e-4})
    loss = mod(torch.tensor(y, device="cuda"), torch.tensor(A, device="cuda"))
    rc, o = run(A, y, sign=sign, n_iter=200 * int(AC.fixture()["conv_chunks"]), cap=AC.max_nnz(A))
    assert np.array_equal(loss.cpu().numpy(), o["loss"])


def test_module_route_lazy_check_masks_a_too_large_instance():
    import torch

    from cave_amd import cave, qpsolver
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.sparse import SparseCones

    rng = np.random.default_rng(4)
    A = (rng.standard_normal((3, 20, 16)) * (rng.random((3, 20, 16)) < 0.2)).astype(np.float32)
    y = rng.standard_normal((3, 16)).astype(np.float32)
    cones = SparseCones.from_dense(A).cuda()
    cones._max_nnz = int(cones.nnz_per_instance.min())  # a capacity one instance at least does not fit
    too = (cones.nnz_per_instance > cones._max_nnz).cpu().numpy()
    assert too.any() and not too.all()
    for check in (False, "lazy"):
        mod = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none", seed=0,
                                     solver_kwargs={"inner": "apgd", "max_iters": 10, "check": check})
        pred = torch.tensor(y, device="cuda", requires_grad=True)
        loss = mod(pred, cones)
        loss.sum().backward()
        l, g = loss.detach().cpu().numpy(), pred.grad.cpu().numpy()
        if check == "lazy":  # masked on the device; the verdict arrives later
            assert (l[too] == 0).all() and (g[too] == 0).all() and np.isfinite(l).all()
            with pytest.raises(qpsolver.HipSolverError):
                cave.flush_checks()
        else:
            assert np.isnan(l[too]).all()
        rc, o = run(A, y, sign=-1.0, n_iter=10)
        assert np.array_equal(l[~too], o["loss"][~too]) and np.array_equal(g[~too], o["grad"][~too])
    with pytest.raises(qpsolver.HipSolverError, match="160 KiB"):  # check=True raises at once
        innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", solver_kwargs={"inner": "apgd", "max_iters": 10})(
            torch.tensor(y, device="cuda"), cones)


def test_integration_doc_stub_as_written():
    """INTEGRATION.md §17's `project_apgd_hip` against the package's and the converged record's chunk count"""
    import torch

    from cave_amd import qpsolver
    from test_apgd_emul import _doc_stub

    ns = _doc_stub()[0]
    A, y, sign = AC.converged_input()
    ctrs, signed = torch.tensor(A, device="cuda"), torch.tensor(sign * y, device="cuda")
    for kw in ({}, {"tol_grad": None, "max_iters": 30, "check_frequency": 7}):
        proj, rn = ns["project_apgd_hip"](ctrs, signed, **kw)
        p2, r2 = qpsolver.project_apgd_hip(ctrs, signed, **kw)
        assert torch.equal(proj, p2) and float((rn - r2).abs().max()) <= 2.0 ** -22 * float(r2.max())


def test_empty_batch_through_the_host_layer_and_the_module():
    """B == 0: the C ABI answers CAVE_OK before it looks at anything; the host layer and the module return empty tensors"""
    import torch

    from cave_amd import qpsolver
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.sparse import SparseCones

    dense = torch.zeros(0, 9, 12, device="cuda")
    sparse = SparseCones.from_dense(np.zeros((0, 9, 12), np.float32)).cuda()
    pred = torch.zeros(0, 12, device="cuda")
    for cones in (dense, sparse):
        for kw in ({}, {"tol_grad": None}, {"tol_grad": None, "max_iters": 450, "check": False}):
            info = {}
            proj, rn = qpsolver.project_apgd_hip(cones, pred, info=info, **kw)
            assert proj.shape == (0, 12) and rn.shape == (0,) and info == {"chunks": 0, "pgrad": []}
        for op in (qpsolver.cone_op_apgd_sparse if cones is sparse else qpsolver.cone_op_apgd,):
            o = op(cones, pred, 1, -1.0, pgrad=True, outputs=("loss", "grad"))
            assert o["loss"].shape == (0,) and o["grad"].shape == (0, 12) and o["pgrad"].shape == (0,) and o["state"][0].shape == (0, 9)
        for red, shape in (("none", (0,)), ("sum", ())):
            for tol in (None, 1e-4):
                mod = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction=red, seed=0,
                                             solver_kwargs={"inner": "apgd", "max_iters": 20, "tol_grad": tol})
                p = pred.clone().requires_grad_(True)
                loss = mod(p, cones)
                assert loss.shape == shape
                loss.sum().backward()
                assert p.grad.shape == (0, 12)
                assert mod._get_projection(pred, cones).shape == (0, 12)


def test_the_class_chooses_the_arm_and_warm_start_runs_cold():
    """exactConeAlignedCosine ignores solver_kwargs['inner'] as it always has (the exact projection, not APGD); on the APGD
    arm `warm_start` runs cold and makes no multiplier cache"""
    import torch

    from cave_amd.cave import EPO, exactConeAlignedCosine, innerConeAlignedCosine

    A, y, _ = AC.fixture_inputs()["sp5"]
    ctrs, pred = torch.tensor(A, device="cuda"), torch.tensor(y, device="cuda")
    plain = exactConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none")(pred, ctrs)
    keyed = exactConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none", solver_kwargs={"inner": "apgd"})(pred, ctrs)
    assert torch.equal(plain, keyed)
    kw = {"inner": "apgd", "max_iters": 20}
    cold = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none", seed=0, solver_kwargs=dict(kw))
    warm = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none", seed=0, solver_kwargs=dict(kw, warm_start=True))
    assert torch.equal(cold(pred, ctrs), warm(pred, ctrs)) and warm._warm is None
    assert not torch.equal(cold(pred, ctrs), plain)  # 20 iterations are not the exact projection
