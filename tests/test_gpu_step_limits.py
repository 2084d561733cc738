"""GPU tier: the fused step kernel at the lite solver's limits (the cones of tests/limit_cones.py through the real
library), against the certified fp64 oracle of tests/test_step_emul.py and against the CPU emulation of the same code.

Routes: prepare_dense -> cone_op_prepared (the fused launch: a solve beside a pack of the same cones), ConeStore
.from_dense / .from_sparse -> cone_op (the solve-only launch over the lite slots of a store, the only form cones with
d > ~228 can take), SparseCones batches through a loss module.  Tolerances: tests/golden_cases.py."""

import ctypes as C

import numpy as np
import pytest

import limit_cones as LC
from certificate import assert_projection
from golden_cases import MODE_AVG, MODE_EXACT, MODE_HEURISTIC, MODE_INNER, MODE_PROJECT, TOL
from test_step_emul import MODES, RATIO, SEEDS, SOLVE_MODES, _batch, _projection, assert_matches, reference, slot_words

pytestmark = pytest.mark.gpu

ALL = ("proj", "rnorm", "target", "loss", "grad")


class _M:
    from cave_amd.abcmodule import EPO

    modelSense = EPO.MINIMIZE


def _defined(mode):
    """the outputs a mode writes (the others are left as they were allocated: PROJECT stops after proj / rnorm, HEURISTIC
    projects nothing, AVG writes the average normal as the target)"""
    return {MODE_AVG: ("target",), MODE_PROJECT: ("proj", "rnorm"), MODE_HEURISTIC: ("target", "loss", "grad")}.get(mode, ALL)


def _np(o):
    return {k: v.detach().cpu().numpy() for k, v in o.items()}


def _step_lds(m, d):
    from cave_amd import _lib

    return int(_lib.load_library().cave_hip_step_lds_bytes(m, d))


def _fused_cases():
    """the "in" cases whose dense batch has a fused launch (as drawn, not padded)"""
    out = []
    for c in LC.IN_CASES:
        bt = _batch(c.name, SEEDS[0])
        if _step_lds(bt["ctrs"].shape[1], c.d) > 0:
            out.append(c)
    return out


def _fresh_shape_state(m, d):
    """What the host layer remembers about the dense shape (m_max, d) is dropped (the shapes of these batches recur
    between tests: a shape an earlier test saw refused must qualify again), and so is any lazily deferred verdict an
    earlier test left unexamined."""
    import torch

    from cave_amd import cave, qpsolver

    torch.cuda.synchronize()
    cave._pending_checks.clear()
    qpsolver.forget_shape(int(m), int(d))


def test_launch_forms_by_shape():
    """cave_hip_step_lds_bytes: d = 256 has a solve-only launch (four workgroups of 28672 bytes per compute unit) and no
    fused one (six do not fit); d = 257 is CAVE_E_INVALID; the benchmark shape keeps its figures."""
    assert _step_lds(0, 256) == 28672 and _step_lds(0, 190) == 25344 and _step_lds(232, 190) == 26624
    for m in (1, 190, 400, 1000):
        assert _step_lds(m, 256) == -1 and _step_lds(m, 229) == -1
    assert _step_lds(64, 228) > 0
    assert _step_lds(0, 257) == -1 and _step_lds(100, 257) == -1
    names = [c.name for c in _fused_cases()]
    assert "d64_8f8b_512" in names and "d40_0f1b_2" in names, names


@pytest.mark.parametrize("case", LC.IN_CASES, ids=lambda c: c.name)
def test_fused_launch_on_limit_cones(case):
    """prepare_dense -> cone_op_prepared with the same cones attached as the following batch (both halves of the kernel
    in every call), all modes, both signs, vs the oracle.  A shape without a fused launch (d = 256 / 255) makes
    prepare_dense return the tensor; a batch whose dense entries exceed the step's non-zero budget (d = 193: 1850 entries
    against 4 (m_max + d) + 128) reports CAVE_ST_TOO_LARGE from the pack half, and the checked call falls back to the
    general operator: the answers are the oracle's either way."""
    import torch

    from cave_amd.qpsolver import PreparedCones, cone_op_dense, cone_op_prepared, prepare_dense

    bt = _batch(case.name, SEEDS[0])
    ctrs, pred = bt["ctrs"], bt["pred"]
    _fresh_shape_state(*ctrs.shape[1:])
    c = torch.tensor(ctrs, device="cuda")
    p = torch.tensor(pred, device="cuda")
    fused = _step_lds(ctrs.shape[1], case.d) > 0
    fits = 4 * (ctrs.shape[1] + case.d) + 128 >= LC.dense_nnz(ctrs)
    for sign in (-1.0, 1.0):
        for mode in MODES:
            ref = reference(case.name, SEEDS[0], mode, sign)
            prep = prepare_dense(c)
            assert isinstance(prep, PreparedCones) == (fused and (fits or (sign, mode) == (-1.0, MODES[0]))), (fused, fits)
            outs = _defined(mode)
            if isinstance(prep, PreparedCones):
                prep.then(c)
                o = cone_op_prepared(prep, p, mode, sign, RATIO, outputs=outs)
                if fits:
                    assert bool((prep.store.pack_status == 0).all())
                    o2 = cone_op_prepared(prep.next, p, mode, sign, RATIO, outputs=outs)
                    for k in outs:
                        assert torch.equal(o[k], o2[k]), k
            else:
                o = cone_op_dense(c, p, mode, sign, RATIO, outputs=outs)
            o = _np(o)
            assert (o["status"] == 0).all() and o["iters"].max() <= 40
            assert_matches(o, ref, mode, np.float32(sign) * pred, (case.name, mode, sign))


def _padded_fused_batch(n_free, n_bound, nnz, share, seed, d_from=256, d_only=None):
    """(case, unpadded batch, padded batch) at the largest d <= d_from at which the family, padded with zero rows until the
    step's budget of 4 (m_max + d) + 128 non-zeros per instance holds its dense entries, still has a fused launch
    (cave_hip_step_lds_bytes of the library); None if there is none down to d = 193"""
    for d in ([d_only] if d_only else range(d_from, 192, -1)):
        case = LC.Case(f"d{d}_{n_free}f{n_bound}b_{nnz}_padded", d, n_free, n_bound, nnz, unit_share=share)
        raw = LC.batch(case, seed)
        m_pad = LC.m_max_for_fused(raw["ctrs"], d)
        if _step_lds(m_pad, d) > 0:
            return case, raw, LC.batch(case, seed, m_max=m_pad)
    return None


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("fam", [(16, 8, 1032, 0.1, None), (19, 8, 1027, 0.5, 193)],
                         ids=["16f8b_1032_at_the_fused_limit", "d193_19f8b_1027_padded"])
def test_fused_launch_at_the_limits_on_padded_batches(fam, seed):
    """The FUSED launch on cones at the limits: the fourth coordinate slot of a lane (d >= 193), the third csr16 group
    (more than 1024 non-zeros, 24 entries per lane), 8 bound rows with a scratch block of their own -- through the pack
    half (run_pack_lite_instance / write_lite_slot) and a solve beside a pack, on the hardware.  As drawn such a batch
    exceeds the step's budget of 4 (m_max + d) + 128 dense non-zeros per instance (a free row arrives twice), so it is
    padded with zero rows until they fit; d is the largest at which the padded batch still has a fused launch, asked of
    cave_hip_step_lds_bytes downwards from 256 (the 24-row family), or 193 itself (the d193 'in' case, padded).
    Asserted: prepare_dense gives a PreparedCones, pack status 0 from the pack-only launch AND from the pack beside the
    solve, header words, all modes and both signs vs the certified oracle, the store packed beside a solve gives the same
    bits.  The SAME cones not padded: the pack half answers CAVE_ST_TOO_LARGE and the checked call falls back to the
    general operator (same oracle)."""
    import torch

    from cave_amd.qpsolver import PreparedCones, cone_op_prepared, prepare_dense
    from oracle import cave_oracle as O
    from certificate import kkt_certificate

    n_free, n_bound, nnz, share, d_only = fam
    found = _padded_fused_batch(n_free, n_bound, nnz, share, seed, d_only=d_only)
    assert found is not None, "no fused launch at d >= 193 for this family"
    case, raw, bt = found
    d = case.d
    assert d >= 193 and LC.scratch_fits(d, case.p, n_bound) and LC.scratch_doubles(case.p, n_bound) > d
    ctrs, pred = bt["ctrs"], bt["pred"]
    _fresh_shape_state(*ctrs.shape[1:])
    _fresh_shape_state(*raw["ctrs"].shape[1:])
    c, p = torch.tensor(ctrs, device="cuda"), torch.tensor(pred, device="cuda")
    refs = {}
    for sign in (-1.0, 1.0):
        y = np.float32(sign) * pred
        proj, rnorm = O.batch_project(y, ctrs)
        for b in range(len(y)):
            k = kkt_certificate(ctrs[b], y[b], proj[b], 4e-6)
            assert k["dual"] <= 4e-6 and k["comp"] <= 4e-6 and k["member"], (sign, b, k)
        refs[sign] = (proj, rnorm)
    for sign in (-1.0, 1.0):
        y = np.float32(sign) * pred
        proj, rnorm = refs[sign]
        avg = O.average_ctrs(ctrs)
        for mode in MODES:
            target = {MODE_EXACT: lambda: _with_projection(lambda: O.exact_target(y, ctrs)[0], proj, rnorm),
                      MODE_INNER: lambda: _with_projection(lambda: O.inner_target(y, ctrs, RATIO)[0], proj, rnorm),
                      MODE_HEURISTIC: lambda: O.heuristic_target(y, ctrs, RATIO), MODE_AVG: lambda: avg,
                      MODE_PROJECT: lambda: None}[mode]()
            ref = {"proj": proj, "rnorm": rnorm, "target": target}
            if mode in (MODE_EXACT, MODE_INNER, MODE_HEURISTIC):
                ref["loss"], ref["grad"] = O.cone_loss(pred, target, sign), O.cone_loss_grad(pred, target, sign)
            prep = prepare_dense(c)
            assert isinstance(prep, PreparedCones)
            prep.then(c)
            outs = _defined(mode)
            o = cone_op_prepared(prep, p, mode, sign, RATIO, outputs=outs)
            assert bool((prep.store.pack_status == 0).all()) and isinstance(prep.next, PreparedCones)
            o2 = cone_op_prepared(prep.next, p, mode, sign, RATIO, outputs=outs)
            assert bool((prep.next.store.pack_status == 0).all())
            for k in outs + ("iters",):
                assert torch.equal(o[k], o2[k]), (mode, sign, k)
            for st in (prep.store, prep.next.store):
                hdr = st.t["hdr"].cpu().numpy().reshape(len(ctrs), 8)
                for b in range(len(ctrs)):
                    assert hdr[b, 0] == 1 and (hdr[b, 1], hdr[b, 2], hdr[b, 3], hdr[b, 5], hdr[b, 6]) == LC.header_of(case, bt["rows"][b]), hdr[b]
                assert int(hdr[0, 6]) == 24
            o = _np(o)
            assert (o["status"] == 0).all() and o["iters"].max() <= 40
            assert_matches(o, ref, mode, y, (case.name, mode, sign))
    # the same cones, not padded: their dense entries exceed the budget -> pack status TOO_LARGE, checked call falls back
    rc = torch.tensor(raw["ctrs"], device="cuda")   # (the same cones; the predictions of the padded batch go with them)
    assert 4 * (raw["ctrs"].shape[1] + d) + 128 < LC.dense_nnz(raw["ctrs"]) and _step_lds(raw["ctrs"].shape[1], d) > 0
    prep = prepare_dense(rc)
    assert isinstance(prep, PreparedCones)
    torch.cuda.synchronize()
    assert bool((prep.store.pack_status == 2).all())
    assert all(np.array_equal(a, b) for a, b in zip(raw["rows"], bt["rows"]))
    o = _np(cone_op_prepared(prep, p, MODE_INNER, -1.0, RATIO, outputs=ALL))
    assert (o["status"] == 0).all()
    proj, rnorm = refs[-1.0]
    t = _with_projection(lambda: O.inner_target(-pred, ctrs, RATIO)[0], proj, rnorm)
    assert_matches(o, {"proj": proj, "rnorm": rnorm, "target": t, "loss": O.cone_loss(pred, t, -1.0),
                       "grad": O.cone_loss_grad(pred, t, -1.0)}, MODE_INNER, -pred, (case.name, "not padded"))
    assert prepare_dense(rc) is rc


def _with_projection(fn, proj, rnorm):
    """an oracle target function evaluated on an already computed (and certified) projection"""
    from unittest import mock

    from oracle import cave_oracle as O

    with mock.patch.object(O, "batch_project", lambda *_a: (proj, rnorm)):
        return fn()


def _store_checks(store, case, seed, warm):
    import torch

    bt = _batch(case.name, seed)
    pred = bt["pred"]
    B = len(pred)
    assert store.lite_slots is not None, "an 'in' batch must be served from the lite slots (solve-only launch)"
    hdr = store.lite_slots.t["hdr"].cpu().numpy().reshape(B, 8)
    for b in range(B):
        assert hdr[b, 0] == 1 and (hdr[b, 1], hdr[b, 2], hdr[b, 3], hdr[b, 5], hdr[b, 6]) == LC.header_of(case, bt["rows"][b]), hdr[b]
    perm = np.random.default_rng(seed).permutation(B)
    ids = torch.tensor(perm, device="cuda")
    if warm:
        store.enable_warm_start(True)
    for sign in (-1.0, 1.0):
        for mode in MODES:
            ref = reference(case.name, seed, mode, sign)
            outs = _defined(mode)
            pin = None if mode == MODE_AVG else torch.tensor(pred[perm], device="cuda")
            for rep in range(2 if warm and mode in SOLVE_MODES else 1):
                o = store.cone_op(ids, pin, mode, sign, RATIO, outputs=outs)
                hit = o.get("warm_hit")
                o = _np({k: v for k, v in o.items() if k != "zero_failed"})
                assert (o["status"] == 0).all() and o["iters"].max() <= 40, (mode, sign, o["status"])
                back = {k: np.empty_like(v) for k, v in o.items()}
                for k in back:
                    back[k][perm] = o[k]
                assert_matches(back, ref, mode, np.float32(sign) * pred, (case.name, mode, sign, rep))
                if warm and mode in SOLVE_MODES:
                    assert hit is not None and (rep == 0 or bool((hit == 1).all())), (mode, sign, rep)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", LC.IN_CASES, ids=lambda c: c.name)
def test_store_route_on_limit_cones(case, seed):
    """ConeStore.from_dense and .from_sparse: the lite slots exist, their header words show the case where it claims to
    be, cone_op with permuted ids equals the oracle in all modes and both signs -- through the SOLVE-ONLY launch, whose
    LDS is step_solve_lds_bytes(d) alone (a slot that says 1 must be solved there) -- cold and with warm start on (the
    second call of a mode hits for every instance)."""
    import torch

    from cave_amd.dataset import ConeStore
    from cave_amd.sparse import SparseCones

    bt = _batch(case.name, seed)
    c = torch.tensor(bt["ctrs"], device="cuda")
    _store_checks(ConeStore.from_dense(c), case, seed, warm=False)
    _store_checks(ConeStore.from_sparse(SparseCones.from_dense(c)), case, seed, warm=True)


@pytest.mark.parametrize("case", [c for c in LC.IN_CASES if c.d >= 193 or c.name == "d64_8f8b_512"], ids=lambda c: c.name)
def test_gpu_lite_slots_equal_the_emulation(case):
    """The lite store the GPU builds (cave_hip_lite_from_packed inside ConeStore) equals the emulation's word for word:
    header, sign bytes, row pointers, ell, csr16 up to the cone's own extent, rl exactly; avg to 2e-6."""
    import torch

    from cave_amd.dataset import ConeStore
    from emul_lib import Emul, Simt
    from test_step_emul import store_route

    bt = _batch(case.name, SEEDS[0])
    ctrs = bt["ctrs"]
    ls, la, status, keep = store_route(Emul(), Simt(), ctrs)
    store = ConeStore.from_dense(torch.tensor(ctrs, device="cuda"))
    assert store.lite_slots is not None and (status == 0).all()
    ga = {k: v.cpu().numpy() for k, v in store.lite_slots.t.items()}
    ga = {k: (v.view(np.uint32) if v.dtype == np.int32 and k != "hdr" else v) for k, v in ga.items()}
    for b in range(len(ctrs)):
        wa, wb = slot_words(la, b, case.d), slot_words(ga, b, case.d)
        for k in wa:
            if k == "avg":
                assert np.abs(wa[k] - wb[k]).max() <= TOL, (b, k)
            else:
                assert np.array_equal(wa[k], wb[k]), (b, k)


@pytest.mark.parametrize("seed", (21, 22))
@pytest.mark.parametrize("case", LC.OUT_CASES + LC.SCRATCH_CASES, ids=lambda c: c.name)
def test_cones_beyond_a_limit_fall_back_and_equal_the_oracle(case, seed):
    """A batch with a cone the lite solver does not take: the store keeps no lite slots and answers through the general
    operator; a checked prepared call falls back to the general operator and prepare_dense then returns the tensor for
    that shape; the answers are the oracle's."""
    import torch

    from cave_amd.dataset import ConeStore
    from cave_amd.qpsolver import PreparedCones, cone_op_prepared, prepare_dense

    bt = _batch(case.name, seed)
    ctrs, pred = bt["ctrs"], bt["pred"]
    _fresh_shape_state(*ctrs.shape[1:])
    c, p = torch.tensor(ctrs, device="cuda"), torch.tensor(pred, device="cuda")
    ref = reference(case.name, seed, MODE_INNER, -1.0)
    store = ConeStore.from_dense(c)
    assert store.lite_slots is None
    o = _np(store.cone_op(torch.arange(len(c), device="cuda"), p, MODE_INNER, -1.0, RATIO, outputs=ALL))
    assert (o["status"] == 0).all()
    assert_matches(o, ref, MODE_INNER, -pred, (case.name, "store"))
    prep = prepare_dense(c)
    if _step_lds(ctrs.shape[1], case.d) > 0:
        assert isinstance(prep, PreparedCones)
        o = _np(cone_op_prepared(prep, p, MODE_INNER, -1.0, RATIO, outputs=ALL))
        assert (o["status"] == 0).all()
        assert_matches(o, ref, MODE_INNER, -pred, (case.name, "prepared"))
        assert prepare_dense(c) is c          # the shape no longer qualifies
    else:
        assert prep is c


def test_d257_is_invalid_for_the_step_and_served_by_the_general_path():
    import torch

    from cave_amd.cave import innerConeAlignedCosine
    from cave_amd.qpsolver import prepare_dense
    from oracle import cave_oracle as O

    case = LC.Case("d257", 257, 10, 3, 600)
    bt = LC.batch(case, 5, B=4)
    _fresh_shape_state(*bt["ctrs"].shape[1:])
    c, p = torch.tensor(bt["ctrs"], device="cuda"), torch.tensor(bt["pred"], device="cuda", requires_grad=True)
    assert _step_lds(bt["ctrs"].shape[1], 257) == -1 and prepare_dense(c) is c
    mod = innerConeAlignedCosine(_M(), solver="hip", seed=0, solver_kwargs={"warm_start": True})
    loss = mod(p, c)
    loss.backward()
    ref_loss, ref_grad = O.ConeLossOracle(minimize=True, inner=True, seed=0)(bt["pred"], bt["ctrs"])
    assert abs(float(loss) - float(ref_loss)) <= TOL
    assert np.abs(p.grad.cpu().numpy() - ref_grad).max() <= 4 * TOL * max(1.0, float(np.abs(ref_grad).max()))


@pytest.mark.parametrize("name", [c.name for c in LC.IN_CASES])
def test_sparse_batches_through_a_loss_module(name):
    """collate_sparse batches (one-instance SparseCones per sample) through innerConeAlignedCosine with warm_start on, vs
    the oracle's loss and gradient."""
    import torch

    from cave_amd.cave import innerConeAlignedCosine
    from cave_amd.sparse import SparseCones, collate_sparse
    from oracle import cave_oracle as O

    bt = _batch(name, SEEDS[0])
    ctrs, pred = bt["ctrs"], bt["pred"]
    _fresh_shape_state(*ctrs.shape[1:])
    samples = [(torch.tensor(pred[b]), SparseCones.from_dense(torch.tensor(ctrs[b:b + 1]))) for b in range(len(ctrs))]
    y, cones = collate_sparse(samples)
    mod = innerConeAlignedCosine(_M(), solver="hip", seed=0, reduction="none", solver_kwargs={"warm_start": True})
    ref = reference(name, SEEDS[0], MODE_INNER, -1.0)
    for _ in range(2):
        p = y.clone().cuda().requires_grad_(True)
        loss = mod(p, cones.cuda())
        loss.sum().backward()
        assert np.abs(loss.detach().cpu().numpy() - ref["loss"]).max() <= TOL
        gs = max(1.0, float(np.abs(ref["grad"]).max()))
        assert np.abs(p.grad.cpu().numpy() - ref["grad"]).max() <= 4 * TOL * gs


def test_mixed_batch_of_1024_is_deterministic_and_certified():
    """Every d = 256 "in" case tiled to 1024 ids over one store: three launches bit-identical, 16 projections
    KKT-certified.  (A store -- and a dense batch -- has ONE d, so "all in cases tiled" can only mean those of one
    dimension; d = 256 is the one with the most cases, and the one with no fused launch.)"""
    import torch

    from cave_amd.dataset import ConeStore

    cases = [c for c in LC.IN_CASES if c.d == 256]
    bts = [_batch(c.name, SEEDS[0]) for c in cases]
    m = max(bt["ctrs"].shape[1] for bt in bts)
    ctrs = np.zeros((sum(len(bt["ctrs"]) for bt in bts), m, 256), np.float32)
    pred = np.concatenate([bt["pred"] for bt in bts])
    i = 0
    for bt in bts:
        ctrs[i:i + len(bt["ctrs"]), :bt["ctrs"].shape[1]] = bt["ctrs"]
        i += len(bt["ctrs"])
    store = ConeStore.from_dense(torch.tensor(ctrs, device="cuda"))
    assert store.lite_slots is not None
    n = len(ctrs)
    ids = torch.arange(1024, device="cuda") % n
    rng = np.random.default_rng(5)
    y = np.float32(rng.standard_normal((1024, 256)))
    p = torch.tensor(y, device="cuda")
    outs = [store.cone_op(ids, p, MODE_INNER, -1.0, RATIO, outputs=ALL) for _ in range(3)]
    assert bool((outs[0]["status"] == 0).all()) and int(outs[0]["iters"].max()) <= 40
    for o in outs[1:]:
        for k in ALL + ("iters",):
            assert torch.equal(o[k], outs[0][k]), k
    proj = outs[0]["proj"].cpu().numpy()
    for b in rng.choice(1024, 16, replace=False):
        assert_projection(ctrs[b % n], -y[b], proj[b], 4e-6, what=int(b))


def test_lazy_check_on_prefetched_batches_re_tiers_after_an_over_limit_cone():
    """check='lazy' on prefetch batches: a cone with 10 bound rows is reported CAVE_ST_TOO_LARGE by the step kernel, its
    loss and gradient zeroed on the device.  The verdict raises once (with a message that names the lite solver), marks
    the shape as not qualifying, and the call after the verdict -- a batch prepared BEFORE it included -- runs through the
    general path, status-checked, and equals the oracle.  (Before: forget_shape alone left the shape qualifying and every
    later batch raised again.)"""
    import torch

    from cave_amd import qpsolver
    from cave_amd.cave import flush_checks, innerConeAlignedCosine
    from cave_amd.dataset import prefetch
    from cave_amd.qpsolver import HipSolverError, PreparedCones, prepare_dense
    from oracle import cave_oracle as O

    case = LC.Case("d64_10bound", 64, 6, 10, 400, kind="out")
    bt = LC.batch(case, 31, B=6)   # instance 1: 10 bound rows; the others small qualifying cones
    ctrs, pred = bt["ctrs"], bt["pred"]
    _fresh_shape_state(*ctrs.shape[1:])
    shape = tuple(ctrs.shape[1:])
    assert _step_lds(*shape) > 0
    c = torch.tensor(ctrs, device="cuda")
    mod = innerConeAlignedCosine(_M(), solver="hip", seed=0, reduction="none", solver_kwargs={"check": "lazy"})
    ref_t = O.inner_target(-pred, ctrs, 0.2)[0]
    ref_loss, ref_grad = O.cone_loss(pred, ref_t, -1.0), O.cone_loss_grad(pred, ref_t, -1.0)
    batches = prefetch([(torch.tensor(pred), c) for _ in range(4)])
    seen = []
    raised = 0
    for step, (p, cones) in enumerate(batches):
        seen.append(type(cones).__name__)
        p = p.cuda().requires_grad_(True)
        try:
            loss = mod(p, cones)
        except HipSolverError as e:
            raised += 1
            assert "one-wave solver" in str(e), str(e)
            assert qpsolver._step_ok.get(shape) is False
            loss = mod(p, cones)          # the call after the verdict: general path, checked
        loss.sum().backward()
        torch.cuda.synchronize()
        lo, gr = loss.detach().cpu().numpy(), p.grad.cpu().numpy()
        if qpsolver._step_ok.get(shape) is False:
            assert np.abs(lo - ref_loss).max() <= TOL, step
            assert np.abs(gr - ref_grad).max() <= 4 * TOL * max(1.0, float(np.abs(ref_grad).max())), step
        else:   # lazy step-kernel launch: the over-limit instance is zeroed, the others are right
            assert lo[1] == 0 and not gr[1].any() and np.abs(np.delete(lo - ref_loss, 1)).max() <= TOL, step
        if step == 0:
            torch.cuda.synchronize()   # let the verdict of the first launch arrive before the next call polls
    try:
        flush_checks()
    except HipSolverError:
        raised += 1
    assert raised == 1 and seen[0] == "PreparedCones", (raised, seen)
    assert prepare_dense(c) is c
