"""GPU tier: the interior-point iterate of CAVE_MODE_INNER_IPM on the MI355X against its own definition.

The same inputs, reference and bounds as tests/test_ipm_iterate_emul.py (tests/ipm_cases.py, tests/ipm_ref.py), through
every entry point that serves the mode:

  cone_op_dense at waves 0 / 1 / 2 / 4 / 8                      the LDS-resident general kernels
  ConeStore.cone_op on the packed route and on the lite slots    cave_hip_cone_packed / the solve-only step launch
  cone_op_prepared on dense and sparse chains                    cave_hip_cone_step_ipm / cave_hip_cone_step_sparse_ipm
  ConeStore.cone_op on the large path at 4 / 2 / 1 waves         cave_hip_cone_packed_large: band and dense forms, B = 2
  tests/prims/_prims.so                                          the solver alone: the double state (assertion (b))

Here v_rcp_f64 / v_sqrt_f64, the 64-bit LDS atomics and the MFMA trailing update of dense_factor act; the emulation
divides exactly.  Where the solver of an entry is a register Gauss-Jordan of one wave (WaveCtx, the lite form), the
twins that give E_k take reciprocals accurate to 2^-47, as linsys_ref documents those solvers (ipm_ref.twins, rcp).
Nothing is compared with another kernel."""

import os

import numpy as np
import pytest

import ipm_cases as IC
import limit_cones as LC
from golden_cases import TOL
from ipm_ref import L

pytestmark = pytest.mark.gpu
ALL = ("proj", "rnorm", "target", "loss", "grad")
OUT = ALL + ("status", "iters")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    IC.write_record("mi355x", os.path.join(ROOT, "profiles", "ipm_iterate_margins.json"))


def _dev(a):
    import torch

    return torch.tensor(a, device="cuda")


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items() if hasattr(v, "cpu")}


def _same_bits(a, b, what):
    for f in OUT:
        assert np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), (what, f)


def _scaling(out, name, what, k, weights="f32"):
    from test_ipm_iterate_emul import check_scaling

    return check_scaling(out, name, what, k, weights)


# ------------------------------------------------------------------------------------------------ general kernels
@pytest.mark.parametrize("waves", [0, 1, 2, 4, 8])
@pytest.mark.parametrize("name", IC.SMALL)
def test_cone_op_dense(name, waves):
    """waves = 1: WaveCtx, sums in lane order; 2 / 4 / 8: BlockCtx, the Hessian in 64-bit fixed point through LDS atomics
    (F_k joins the bound); 0: the library's choice, held to the bound of either"""
    from cave_amd.qpsolver import cone_op_dense

    f = IC.family(name)
    kw = {"nnz_cap": LC.dense_nnz(f["ctrs"]) + 64, "lds_bytes": 160 * 1024} if name.startswith("limit/") else {}
    ctrs, pred = _dev(f["ctrs"]), _dev(f["pred"])
    outs = {}
    for k in IC.K_STEPS:
        o = _np(cone_op_dense(ctrs, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=k, waves=waves, check=False, outputs=ALL, **kw))
        IC.compare(o, name, k, "f32", waves != 1, f"gpu/cone_op_dense/w{waves}", IC.RECORD, rcp=waves in (0, 1))
        _scaling(o, name, f"gpu/cone_op_dense/w{waves}", k)
        outs[k] = o
    o0 = _np(cone_op_dense(ctrs, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=0, waves=waves, check=False, outputs=ALL, **kw))
    _same_bits(o0, outs[3], (name, waves, "max_iter = 0 means 3"))


@pytest.mark.parametrize("name", IC.SMALL)
def test_store_packed_route(name):
    """ConeStore.cone_op with a wave count of the caller's: cave_hip_cone_packed on WaveCtx and BlockCtx<4>"""
    import torch

    from cave_amd.dataset import ConeStore

    f = IC.family(name)
    store = ConeStore.from_dense(_dev(f["ctrs"]))
    ids, pred = torch.arange(len(f["y"]), device="cuda"), _dev(f["pred"])
    for waves in (1, 4):
        store.waves = waves
        for k in IC.K_STEPS:
            o = _np(store.cone_op(ids, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=k, check=False, outputs=ALL))
            IC.compare(o, name, k, "f32", True, f"gpu/store_packed/w{waves}", IC.RECORD, rcp=waves == 1)
            _scaling(o, name, f"gpu/store_packed/w{waves}", k)


# ------------------------------------------------------------------------------------------------------- lite form
@pytest.mark.parametrize("name", IC.PM1_ONLY)
def test_store_lite_slots(name):
    """the solve-only launch of the step kernel from a store's lite slots: lite_solve_ipm"""
    import torch

    from cave_amd.dataset import ConeStore

    f = IC.family(name)
    store = ConeStore.from_dense(_dev(f["ctrs"]))
    assert store.lite_slots is not None and store.waves == 0 and not store.large, name
    assert (store.lite_slots.t["hdr"].cpu().numpy()[0::8] == 1).all(), "a cone the lite form refused"
    ids, pred = torch.arange(len(f["y"]), device="cuda"), _dev(f["pred"])
    outs = {}
    for k in IC.K_STEPS:
        o = _np(store.cone_op(ids, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=k, check=False, outputs=ALL))
        IC.compare(o, name, k, "f32", False, "gpu/store_lite_slots", IC.RECORD, rcp=True)
        _scaling(o, name, "gpu/store_lite_slots", k)
        outs[k] = o
    _same_bits(_np(store.cone_op(ids, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=0, check=False, outputs=ALL)), outs[3], (name, "max_iter = 0"))


@pytest.mark.parametrize("wire", ["dense", "sparse"])
@pytest.mark.parametrize("name", ["tsp20", "sp5", "built"])
def test_fused_step_kernels(name, wire):
    """cave_hip_cone_step_ipm / cave_hip_cone_step_sparse_ipm through prepare_cones + cone_op_prepared: a pack-only
    launch, then the interior-point solve half on what it packed"""
    from cave_amd import cave, qpsolver as Q
    from cave_amd.sparse import SparseCones

    f = IC.family(name)
    B, m, d = f["ctrs"].shape
    import torch

    torch.cuda.synchronize()
    cave._pending_checks.clear()
    Q.forget_shape(int(m), int(d))
    Q._step_pool.clear()
    cones = _dev(f["ctrs"]) if wire == "dense" else SparseCones.from_dense(f["ctrs"]).cuda()
    pred = _dev(f["pred"])
    for k in IC.K_STEPS:
        prep = Q.prepare_cones(cones)
        assert isinstance(prep, Q.PreparedCones), (name, wire, "the shape did not qualify for the step kernel")
        o = _np(Q.cone_op_prepared(prep, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=k, check=False, outputs=ALL))
        IC.compare(o, name, k, "f32", False, f"gpu/cone_op_prepared/{wire}", IC.RECORD, rcp=True)
        _scaling(o, name, f"gpu/cone_op_prepared/{wire}", k)


# ------------------------------------------------------------------------------------------------------ large path
@pytest.mark.parametrize("waves", [4, 2, 1])
@pytest.mark.parametrize("name", IC.LARGE)
def test_large_path(name, waves):
    """cave_hip_cone_packed_large, B = 2: band_hessian + solve_spd_band / solve_spd_band_wave (sp12, band4),
    dense_hessian + dense_factor with its MFMA trailing update (tsp30); rho' stays in doubles there: weights = 'f64'"""
    import torch

    from cave_amd.dataset import ConeStore

    f = IC.family(name)
    st = ConeStore.from_dense(_dev(f["ctrs"]), chunk=2)
    st.large, st.large_waves = True, waves
    if not st.band_entries:
        st.band_entries, st.max_bw = st._max_band_entries()
        st.large_lds = 64 * 1024
    ids, pred = torch.arange(len(f["y"]), device="cuda"), _dev(f["pred"])
    for k in IC.K_STEPS:
        o = _np(st.cone_op(ids, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=k, check=False, outputs=ALL))
        IC.compare(o, name, k, "f64", False, f"gpu/cone_packed_large/w{waves}", IC.RECORD)


# --------------------------------------------------------------------------------------- (b): the solver alone, doubles
@pytest.fixture(scope="module")
def prims():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tests", "prims"))
    import prims_lib

    return prims_lib.Prims()


@pytest.mark.parametrize("op,ctx", IC.STATE_KINDS)
def test_double_state_of_the_solver_alone(prims, op, ctx):
    """rho, theta and z of the bound rows, M^T theta in double after 1, 2, 3 steps, within E_k; two launches give the
    same bits where the sums are ordered (fixed point, one wave in lane order)"""
    lite = op == "ipm_lite"
    for name in (IC.PM1_ONLY if lite else IC.SMALL):
        rows = IC.state_rows(name, lite)
        for k in IC.STATE_STEPS:
            cases, pm1 = IC.state_cases(name, k, rows)
            outs = prims.op_run(op, ctx, pm1, cases)
            IC.compare_state(outs, name, k, rows, ctx == "b4", f"gpu/{op}/{ctx}", IC.RECORD, lite=lite, rcp=ctx != "b4")
            if ctx != "w1":
                again = prims.op_run(op, ctx, pm1, cases)
                for a, b in zip(outs, again):
                    assert np.array_equal(a["out"], b["out"]), (name, k, op, ctx, "second launch")


# ------------------------------------------------------------------------------------------------- (c): on the floor
@pytest.mark.parametrize("name", list(IC.FLOOR_ROWS))
def test_floor_of_tau_at_24_steps(name):
    from cave_amd.dataset import ConeStore
    from cave_amd.qpsolver import cone_op_dense
    import torch

    f = IC.family(name)
    rows = np.array(IC.FLOOR_ROWS[name])
    ctrs, pred = _dev(f["ctrs"][rows]), _dev(f["pred"][rows])
    k = IC.K_FLOOR
    runs = {f"gpu/cone_op_dense/w{w}": (lambda w=w: cone_op_dense(ctrs, pred, IC.MODE_IPM, IC.SIGN, 0.0, max_iter=k, waves=w,
                                                                  check=False, outputs=ALL)) for w in (1, 4)}
    if name in IC.PM1_ONLY:
        store = ConeStore.from_dense(ctrs)
        assert store.lite_slots is not None
        runs["gpu/store_lite_slots"] = lambda: store.cone_op(torch.arange(len(rows), device="cuda"), pred, IC.MODE_IPM, IC.SIGN, 0.0,
                                                             max_iter=k, check=False, outputs=ALL)
    for what, run in runs.items():
        o = _np(run())
        assert (o["status"] == 0).all() and (o["iters"] == k).all(), what
        for j, b in enumerate(rows):
            ref = IC.reference(name, int(b), "f32", k)[1][k]
            err = float(np.abs(o["proj"][j] - L._f64(ref["proj"])).max()) / (TOL * IC.scale_of(name, int(b)))
            key = f"{what}|{name}|k={k} (error / TOL sc)"
            IC.RECORD[key] = max(IC.RECORD.get(key, 0.0), err)
            assert err <= 1.0, (what, name, int(b), err)
