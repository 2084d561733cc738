"""GPU tier: the fused step in the interior-point mode (cave_hip_cone_step_ipm / cave_hip_cone_step_sparse_ipm, kernels
cone_step_kernel<.., IPM> of k_step_ipm.hip / k_step_sparse_ipm.hip), through cave_amd._lib and the host routes built on
it: the prepared chain (qpsolver.cone_op_prepared, dataset.prefetch), the lite slots of a ConeStore, the loss module.

At max_iter 1 and 3 the new kernel is compared with the EXISTING general kernel on the same inputs,
cone_op_dense(..., MODE_IPM, waves=1), at the tolerances of tests/golden_cases.py, and the general kernel's own spread
between waves=1 and waves=4 is measured beside it (tests/step_ipm_cases.py says what "agree" means); the properties of
tests/test_ipm_mode.py are checked with that file's own functions (at 40 steps against the oracle, not the general
kernel).  Inputs as in tests/test_step_ipm_emul.py."""

import os

import numpy as np
import pytest

import limit_cones as LC
import step_ipm_cases as SC
from test_ipm_mode import MODE_IPM, check_ipm_properties

pytestmark = pytest.mark.gpu

ALL = ("proj", "rnorm", "target", "loss", "grad")
OUT = ALL + ("status", "iters")
ST_TOO_LARGE, ST_BAD_INPUT = 2, 3
RECORD = {}   # figures of this run (tools/diag/ipm_margins.py writes them to profiles/step_ipm_margins.json)


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    """after the last test of this file: the figures the comparisons recorded, written where CAVE_IPM_MARGINS_OUT says"""
    yield
    SC.write_record(RECORD)


class _M:
    from cave_amd.abcmodule import EPO

    modelSense = EPO.MINIMIZE


def _fresh(m, d):
    import torch

    from cave_amd import cave, qpsolver

    torch.cuda.synchronize()
    cave._pending_checks.clear()
    qpsolver.forget_shape(int(m), int(d))
    qpsolver._step_pool.clear()


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items() if hasattr(v, "cpu")}


def _dev(a):
    import torch

    return torch.tensor(a, device="cuda")


def _sparse(ctrs):
    from cave_amd.sparse import SparseCones

    return SparseCones.from_dense(ctrs).cuda()


def _general(ctrs, pred, k, waves, big=False):
    """the existing general kernel at `waves` waves per instance; unchecked, so that nothing re-launches it elsewhere"""
    from cave_amd.qpsolver import cone_op_dense

    kw = {"nnz_cap": LC.dense_nnz(ctrs) + 64, "lds_bytes": 160 * 1024} if big else {}
    o = _np(cone_op_dense(_dev(ctrs), _dev(pred), MODE_IPM, SC.SIGN, 0.0, max_iter=k, waves=waves, check=False, outputs=ALL, **kw))
    assert (o["status"] == 0).all(), o["status"]
    return o


def _no_general_operator(monkeypatch):
    from cave_amd import cave, qpsolver as Q

    def refuse(*a, **k):
        raise AssertionError("the general operator ran")

    for mod in (Q, cave):   # (cave.py binds the two names at import)
        monkeypatch.setattr(mod, "cone_op_dense", refuse)
        monkeypatch.setattr(mod, "cone_op_sparse", refuse)


def _chain(pieces, preds, k, **kw):
    """pieces: dense tensors / SparseCones on the device, chained through prepare(...).then(...): a pack-only launch,
    then solve launches in the interior-point mode that pack the next piece -> outputs per piece"""
    from cave_amd.qpsolver import PreparedCones, cone_op_prepared, prepare_cones

    prep = prepare_cones(pieces[0])
    outs = []
    for i, pred in enumerate(preds):
        assert isinstance(prep, PreparedCones), i
        if i + 1 < len(pieces):
            prep.then(pieces[i + 1])
        outs.append(cone_op_prepared(prep, pred, MODE_IPM, SC.SIGN, 0.0, max_iter=k, outputs=ALL, **kw))
        prep = prep.next
    return {f: np.concatenate([o[f].cpu().numpy() for o in outs]) for f in OUT}


def _same_bits(a, b, what):
    for f in OUT:
        assert np.array_equal(a[f].view(np.uint8), b[f].view(np.uint8)), (what, f)


# ------------------------------------------------------------------ 1. pack-only launch, then fused launches
@pytest.mark.parametrize("name,split", [("tsp20", (6, 5, 5)), ("sp5", (3, 4, 1))])
def test_fused_chains_agree_with_the_general_kernel(golden, monkeypatch, name, split):
    """dense next, sparse next and mixed, halves of different sizes; two runs are bit-identical; the general operators
    are patched to raise, so what answers is the new kernel"""
    ctrs, costs = SC.fixture_inputs(golden)[name]
    m, d = ctrs.shape[1:]
    _fresh(m, d)
    cuts = np.cumsum((0,) + split)
    assert cuts[-1] == len(ctrs)
    parts = [ctrs[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    preds = [_dev(costs[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    forms = {"dense": [_dev(p) for p in parts], "sparse": [_sparse(p) for p in parts],
             "mixed": [_dev(p) if i % 2 else _sparse(p) for i, p in enumerate(parts)]}
    gen = {k: (_general(ctrs, costs, k, 1), _general(ctrs, costs, k, 4)) for k in (1, 3)}
    _no_general_operator(monkeypatch)
    outs = {}
    for k in (1, 3):
        g1, g4 = gen[k]
        for form, pieces in forms.items():
            o = _chain(pieces, preds, k)
            assert (o["status"] == 0).all() and (o["iters"] == k).all(), (name, k, form, o["status"], o["iters"])
            SC.compare(o, g1, g1, g4, SC.SIGN * costs, f"gpu/{name}/max_iter={k}/{form}", RECORD)
            _same_bits(o, _chain(pieces, preds, k), (name, k, form, "second run"))
            if form != "dense":
                _same_bits(o, outs[k], (name, k, form, "the solve half does not care which route packed its store"))
            outs[k] = o
    assert np.abs(outs[1]["loss"] - outs[3]["loss"]).max() > 1e-4   # max_iter is honoured
    _same_bits(_chain(forms["dense"], preds, 0), outs[3], (name, "max_iter <= 0 means 3"))


# ------------------------------------------------------------------ 2. solve-only launch from a store's lite slots
def _store_inputs(golden):
    for name, (ctrs, costs) in SC.fixture_inputs(golden).items():
        yield name, ctrs, costs, False
    for name in SC.LIMIT_NAMES:
        bt = SC.limit_batch(name)
        yield name, bt["ctrs"], bt["pred"], True
    ctrs, pred, _ = SC.edge_batch()
    yield "edge", ctrs, pred, False


def test_store_solve_only_launch_agrees_with_the_general_kernel(golden, monkeypatch):
    """ConeStore.cone_op serves the mode from its lite slots (every d <= 256: the limit cones, a zero prediction, the
    empty cone, unit rows only); ids permuted, repeated, one out of range; a batch of one"""
    import torch

    from cave_amd import qpsolver as Q
    from cave_amd.dataset import ConeStore

    seen = 0
    for name, ctrs, pred, big in _store_inputs(golden):
        B, m, d = ctrs.shape
        gen = {k: (_general(ctrs, pred, k, 1, big), _general(ctrs, pred, k, 4, big)) for k in (1, 3)}
        store = ConeStore.from_dense(_dev(ctrs))
        assert store.lite_slots is not None, name
        p_rows = store.lite_slots.t["hdr"].cpu().numpy()[1::8]
        with monkeypatch.context() as mp:
            # (the general packed kernel is a C entry of its own: refuse it too)
            mp.setattr(store, "_waves_for", lambda *_a: (_ for _ in ()).throw(AssertionError("the general packed kernel ran")))
            ids = torch.arange(B, device="cuda")
            for k in (1, 3):
                o = _np(store.cone_op(ids, _dev(pred), MODE_IPM, SC.SIGN, 0.0, max_iter=k, outputs=ALL))
                assert (o["status"] == 0).all() and np.array_equal(o["iters"], np.where(p_rows > 0, k, 0)), (name, k, o["iters"])
                SC.compare(o, gen[k][0], gen[k][0], gen[k][1], SC.SIGN * pred, f"gpu/{name}/max_iter={k}/store", RECORD)
                o2 = _np(store.cone_op(ids, _dev(pred), MODE_IPM, SC.SIGN, 0.0, max_iter=k, outputs=ALL))
                _same_bits(o, o2, (name, k, "second launch"))
            # warm start asked for: the mode still runs cold, from the same kernel
            store.enable_warm_start(True)
            ow = _np(store.cone_op(ids, _dev(pred), MODE_IPM, SC.SIGN, 0.0, max_iter=3, outputs=ALL))
            store.enable_warm_start(False)
            _same_bits(o, ow, (name, "warm_start"))
            assert "warm_hit" not in ow
            # ... also while the store has no multiplier cache yet: the mode does not wait for one
            keep_cache, store.lite_warm, store.warm_start = store.lite_warm, None, True
            ow = _np(store.cone_op(ids, _dev(pred), MODE_IPM, SC.SIGN, 0.0, max_iter=3, outputs=ALL))
            store.lite_warm, store.warm_start = keep_cache, False
            _same_bits(o, ow, (name, "warm_start without a cache"))
            # permuted, repeated and one out-of-range id, through the launch function (the store's own call checks ids)
            pick = np.array([B - 1, 0, 0, B + 5, B // 2], np.int64)
            inr = pick < B
            pp = _dev(pred[np.minimum(pick, B - 1)])
            for zero_failed in (False, True):
                out = {f: torch.full((5,) if f in ("rnorm", "loss") else (5, d), 77.0, device="cuda") for f in ALL}
                status, iters = torch.full((5,), -7, dtype=torch.int32, device="cuda"), torch.full((5,), -7, dtype=torch.int32, device="cuda")
                Q._launch_step(store.lite_slots, pp, 5, MODE_IPM, SC.SIGN, 0.0, 3, out, status, iters, None, None,
                               ids=_dev(pick), zero_failed=zero_failed)
                got = _np(dict(out, status=status, iters=iters))
                assert np.array_equal(got["status"], np.where(inr, 0, ST_BAD_INPUT))
                for f in OUT:
                    assert np.array_equal(got[f][inr], o[f][pick[inr]]), (name, f)
                assert np.isnan(got["proj"][~inr]).all() and np.isnan(got["target"][~inr]).all()
                if zero_failed:
                    assert (got["loss"][~inr] == 0).all() and (got["grad"][~inr] == 0).all()
                else:
                    assert np.isnan(got["loss"][~inr]).all() and np.isnan(got["grad"][~inr]).all()
            one = _np(store.cone_op(ids[B - 1:], _dev(pred[B - 1:]), MODE_IPM, SC.SIGN, 0.0, max_iter=3, outputs=ALL))
            for f in OUT:
                assert np.array_equal(one[f][0], o[f][B - 1]), (name, "batch of one", f)
        seen += 1
    assert seen == 2 + len(SC.LIMIT_NAMES) + 1 == 9


def test_never_packed_store_reports_too_large(golden):
    import torch

    from cave_amd import qpsolver as Q

    ctrs, costs = SC.fixture_inputs(golden)["sp5"]
    B, m, d = ctrs.shape
    blank = Q._LiteSlots(torch.device("cuda", torch.cuda.current_device()), B, d)
    for zero_failed in (False, True):
        out = {f: torch.full((B,) if f in ("rnorm", "loss") else (B, d), 77.0, device="cuda") for f in ALL}
        status, iters = torch.full((B,), -7, dtype=torch.int32, device="cuda"), torch.full((B,), -7, dtype=torch.int32, device="cuda")
        Q._launch_step(blank, _dev(costs), B, MODE_IPM, SC.SIGN, 0.0, 3, out, status, iters, None, None, zero_failed=zero_failed)
        assert bool((status == ST_TOO_LARGE).all()) and bool((iters == 0).all()) and bool(torch.isnan(out["proj"]).all())
        if zero_failed:
            assert not bool(out["loss"].any()) and not bool(out["grad"].any())
        else:
            assert bool(torch.isnan(out["loss"]).all()) and bool(torch.isnan(out["grad"]).all())


# ------------------------------------------------------------------ 3. fallback of a batch the lite form does not take
def test_cones_that_are_not_pm1_fall_back_to_the_general_operator(golden):
    """the `generic` fixture's Gaussian rows: the pack half refuses them, the checked host call falls back"""
    from cave_amd import qpsolver as Q

    g = golden["generic"]
    ctrs, costs = g["generic_ctrs"], g["generic_costs"]
    m, d = ctrs.shape[1:]
    _fresh(m, d)
    prep = Q.prepare_dense(_dev(ctrs))
    assert isinstance(prep, Q.PreparedCones)
    o = Q.cone_op_prepared(prep, _dev(costs), MODE_IPM, SC.SIGN, 0.0, max_iter=3, outputs=ALL)
    assert Q._step_ok[(m, d)] is False and bool((o["status"] == 0).all()) and bool((o["iters"] == 3).all())
    ref = Q.cone_op_dense(_dev(ctrs), _dev(costs), MODE_IPM, SC.SIGN, 0.0, max_iter=3, outputs=ALL)
    # both sides are the general operator on the same inputs: the per-output tolerances of tests/step_ipm_cases.py
    diff = SC.normalised(_np(o), _np(ref), SC.SIGN * costs)
    for f in ALL:
        assert diff[f] <= SC.TOL, (f, diff[f])
    # unchecked: the verdict is in `status`
    _fresh(m, d)
    o = Q.cone_op_prepared(Q.prepare_dense(_dev(ctrs)), _dev(costs), MODE_IPM, SC.SIGN, 0.0, max_iter=3, check=False, outputs=ALL)
    assert bool((o["status"] == ST_TOO_LARGE).all())
    _fresh(m, d)


# ------------------------------------------------------------------ 4. the loss module
def test_module_on_a_prefetch_chain_runs_the_new_kernel(golden, monkeypatch):
    import torch
    from torch.utils.data import DataLoader

    from cave_amd.cave import innerConeAlignedCosine
    from cave_amd.dataset import ConeStore, PackedBatch, prefetch
    from cave_amd.qpsolver import PreparedCones

    g = golden["structured"]
    ctrs, costs = g["tsp20_ctrs"], g["tsp20_costs"]
    m, d = ctrs.shape[1:]
    _fresh(m, d)
    dc, dy = _dev(ctrs), _dev(costs)

    def module(k, **kw):
        return innerConeAlignedCosine(_M(), solver="hip", solver_kwargs=dict({"inner": "ipm"}, **kw), max_iter=k, reduction="none")

    plain = {}
    for k in (1, 3):
        p = dy.clone().requires_grad_(True)
        loss = module(k)(p, dc)            # the plain call: the general operator
        loss.sum().backward()
        plain[k] = (loss.detach(), p.grad)
    store = ConeStore.from_dense(dc)
    loader = DataLoader([(torch.tensor(costs[b]), torch.tensor(ctrs[b])) for b in range(len(ctrs))], batch_size=6)
    _no_general_operator(monkeypatch)      # from here on only the step kernels can answer
    monkeypatch.setattr(store, "_waves_for", lambda *_a: (_ for _ in ()).throw(AssertionError("the general packed kernel ran")))
    got = {}
    for k, kw in ((1, {}), (3, {}), (3, {"warm_start": True}), (3, {"check": "lazy"})):
        mod = module(k, **kw)
        losses, grads, n = [], [], 0
        for pred, cones in prefetch(loader):
            assert isinstance(cones, PreparedCones), n
            p = pred.cuda().requires_grad_(True)
            loss = mod(p, cones.cuda())
            loss.sum().backward()
            losses.append(loss.detach())
            grads.append(p.grad)
            n += 1
        assert n == 3
        loss, grad = torch.cat(losses), torch.cat(grads)
        assert float((loss - plain[k][0]).abs().max()) <= 2e-6, (k, kw)
        assert float((grad - plain[k][1]).abs().max()) <= 2e-6 * max(1.0, float(np.abs(costs).max())), (k, kw)
        if kw:
            assert torch.equal(loss, got[k][0]) and torch.equal(grad, got[k][1]), kw   # warm_start means "runs cold"
        got[k] = (loss, grad)
        p = dy.clone().requires_grad_(True)
        lp = mod(p, PackedBatch(store, torch.arange(len(ctrs), device="cuda")))
        lp.sum().backward()
        assert float((lp.detach() - plain[k][0]).abs().max()) <= 2e-6, (k, kw, "PackedBatch")
        assert float((p.grad - plain[k][1]).abs().max()) <= 2e-6 * max(1.0, float(np.abs(costs).max())), (k, kw, "PackedBatch")
    from cave_amd.cave import flush_checks

    flush_checks()
    assert float((got[1][0] - got[3][0]).abs().max()) > 1e-4


# ------------------------------------------------------------------ 5. properties
def test_properties_of_the_interior_point_mode(golden, monkeypatch):
    from cave_amd import qpsolver as Q

    _no_general_operator(monkeypatch)

    def run(c, y, k):
        prep = Q.prepare_dense(_dev(c))
        assert isinstance(prep, Q.PreparedCones)
        return _np(Q.cone_op_prepared(prep, _dev(y), MODE_IPM, SC.SIGN, 0.0, max_iter=k, outputs=ALL))
    _fresh(235, 190)
    _fresh(90, 40)
    check_ipm_properties(run, SC.property_golden(golden))

