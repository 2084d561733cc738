"""GPU tier: the fused step for batches on the sparse wire format (cave_hip_cone_step_sparse, qpsolver.prepare_sparse,
dataset.prefetch over a collate_sparse loader, warm start).

The sparse pack half builds the lite store from the same non-zeros in the same arena as the dense pack half, and the
solve half is the same source reading that store: stores, losses, gradients, statuses and iteration counts are compared
BIT FOR BIT between the two routes, and against the reference's own outputs at the tolerances of tests/golden_cases.py
(loss 2e-6, gradient 8e-6 max(1, |grad|_inf)).  Shapes are the small ones of tests/test_step_sparse_emul.py."""

import collections
import os
import sys

import numpy as np
import pytest

import limit_cones as LC
from golden_cases import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("hdr", "usign", "avg", "rowptr", "ell", "csr16", "rl")
OUTS = ("loss", "grad")
LIMIT_CASES = [c for c in LC.IN_CASES + LC.OUT_CASES + LC.SCRATCH_CASES if c.d <= 228]
MODE_INNER = 2


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


def _sparse(ctrs):
    from cave_amd.sparse import SparseCones

    return SparseCones.from_dense(ctrs).cuda()


def _limit_batch(case, seed=11):
    bt0 = LC.batch(case, seed, B=6)
    return LC.batch(case, seed, B=6, m_max=LC.m_max_for_fused(bt0["ctrs"], case.d))


def _pack_only(x):
    """a pack-only launch into a freshly zeroed store: -> ({array: host copy}, pack status)"""
    import torch

    from cave_amd import qpsolver as Q

    sparse = not isinstance(x, torch.Tensor)
    B, d = (len(x), x.d) if sparse else (x.shape[0], x.shape[2])
    ss = Q._LiteSlots(x.device, B, d)
    ss.pack_status.fill_(-7)
    (Q._launch_step_sparse if sparse else Q._launch_step)(None, None, 0, 0, 1.0, 0.0, 0, {}, None, None, x, ss)
    torch.cuda.synchronize()
    return {k: ss.t[k].cpu().numpy() for k in ARRAYS}, ss.pack_status.cpu().numpy()


def _assert_same_store(a, b, what):
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------ 1. pack-only launch
def _pack_inputs(golden):
    g = golden["structured"]
    yield "tsp20", g["tsp20_ctrs"], "in"
    yield "sp5", g["sp5_ctrs"], "in"
    for case in LIMIT_CASES:
        yield case.name, _limit_batch(case)["ctrs"], case.kind


def test_pack_only_launch_writes_the_dense_routes_store(golden):
    import torch

    from cave_amd.qpsolver import step_lds_bytes

    seen = 0
    for name, ctrs, kind in _pack_inputs(golden):
        B, m, d = ctrs.shape
        assert step_lds_bytes(m, d) > 0, (name, m, d)
        da, ds = _pack_only(torch.tensor(ctrs, device="cuda"))
        sa, ss = _pack_only(_sparse(ctrs))
        assert np.array_equal(ds, ss), (name, ds, ss)
        _assert_same_store(da, sa, name)
        state = sa["hdr"][0::8]
        if kind == "in":
            assert (ss == 0).all() and (state == 1).all(), name
        elif kind == "out":
            assert ss[1] == 2 and state[1] == -1 and (np.delete(ss, 1) == 0).all(), name
        else:
            assert (ss == 2).all() and (state == -1).all(), name
        seen += 1
    assert seen == 2 + len(LIMIT_CASES) == 12


# ------------------------------------------------------------------ 2. / 3. chains
def _chain(pieces, preds, warm=None):
    """pieces: dense tensors / SparseCones on the device, chained through prepare(...).then(...): -> outputs per batch"""
    from cave_amd.qpsolver import PreparedCones, cone_op_prepared, prepare_cones

    prep = prepare_cones(pieces[0])
    outs = []
    for i, pred in enumerate(preds):
        assert isinstance(prep, PreparedCones), i
        if i + 1 < len(pieces):
            prep.then(pieces[i + 1])
        outs.append(cone_op_prepared(prep, pred, MODE_INNER, -1.0, 0.2, outputs=OUTS, warm=warm))
        prep = prep.next
    return outs


def _cat(outs, k):
    import torch

    return torch.cat([o[k] for o in outs]).cpu().numpy()


@pytest.mark.parametrize("tag,split", [("tsp20", (6, 5, 5)), ("sp5", (11, 11, 10))])
def test_fused_chain_sparse_equals_dense_and_the_reference(golden, tag, split):
    import torch

    g = golden["structured"]
    ctrs, costs = g[f"{tag}_ctrs"], g[f"{tag}_costs"]
    _fresh(*ctrs.shape[1:])
    cuts = np.cumsum((0,) + split)
    assert cuts[-1] == len(ctrs)
    parts = [ctrs[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    preds = [torch.tensor(costs[a:b], device="cuda") for a, b in zip(cuts[:-1], cuts[1:])]
    dense = _chain([torch.tensor(p, device="cuda") for p in parts], preds)
    sparse = _chain([_sparse(p) for p in parts], preds)
    for k in OUTS + ("status", "iters"):
        assert np.array_equal(_cat(dense, k), _cat(sparse, k)), (tag, k)
    assert (_cat(sparse, "status") == 0).all()
    ok = g[f"{tag}_min_consistent"]
    assert np.all(np.abs(_cat(sparse, "loss") - g[f"{tag}_min_inner_loss"])[ok] <= TOL)
    rg = g[f"{tag}_min_inner_grad"]
    assert np.all(np.abs(_cat(sparse, "grad") - rg)[ok] <= 4 * TOL * max(1.0, float(np.abs(rg).max())))


def test_mixed_chain_gives_the_same_bits(golden):
    import torch

    g = golden["structured"]
    ctrs, costs = g["tsp20_ctrs"], g["tsp20_costs"]
    _fresh(*ctrs.shape[1:])
    parts = [ctrs[i:i + 4] for i in range(0, 16, 4)]
    preds = [torch.tensor(costs[i:i + 4], device="cuda") for i in range(0, 16, 4)]
    dense = _chain([torch.tensor(p, device="cuda") for p in parts], preds)
    mixed = _chain([torch.tensor(p, device="cuda") if i % 2 == 0 else _sparse(p) for i, p in enumerate(parts)], preds)
    for k in OUTS + ("status", "iters"):
        assert np.array_equal(_cat(dense, k), _cat(mixed, k)), k


# ------------------------------------------------------------------ 4. loader alignment on the device
def test_loader_alignment_on_the_device(golden):
    import torch

    from cave_amd.sparse import SparseCones

    ctrs = golden["structured"]["tsp20_ctrs"]
    sc = SparseCones.from_dense(ctrs)
    Z = sc.nnz
    base, bstatus = _pack_only(sc.cuda())
    assert (bstatus == 0).all()
    off = sc.ent_off.cuda()
    starts = set()
    for ok in range(4):
        for ov in (ok, (ok + 1) % 4):
            kb, vb = torch.zeros(Z + 8, dtype=torch.int32, device="cuda"), torch.zeros(Z + 8, dtype=torch.float32, device="cuda")
            assert kb.data_ptr() % 16 == 0 and vb.data_ptr() % 16 == 0
            k, v = kb[ok:ok + Z], vb[ov:ov + Z]
            k.copy_(sc.key)
            v.copy_(sc.val)
            x = SparseCones(sc.m_max, sc.d, off, k, v)
            assert x.key.data_ptr() % 16 == 4 * ok and x.val.data_ptr() % 16 == 4 * ov
            starts |= {((x.key.data_ptr() + 4 * int(o)) % 16) // 4 for o in sc.ent_off[:-1]}
            arrs, status = _pack_only(x)
            assert np.array_equal(status, bstatus), (ok, ov)
            _assert_same_store(base, arrs, (ok, ov))
    assert starts == {0, 1, 2, 3}


# ------------------------------------------------------------------ 5. malformed entries
def _malformed():
    import torch

    from cave_amd import synth
    from cave_amd.sparse import SparseCones
    from test_sparse_cpu import malformed_batch

    ctrs, costs, _ = synth.tsp_batch(20, 14, seed=8)
    off, key, val, bad = malformed_batch(ctrs)
    sc = SparseCones(ctrs.shape[1], ctrs.shape[2], torch.from_numpy(off.copy()), torch.from_numpy(key.view(np.int32).copy()),
                     torch.from_numpy(val.copy()))
    return ctrs, costs, sc.cuda(), bad


def test_malformed_instances_on_the_prepared_route():
    import torch

    from cave_amd.cave import exactConeAlignedCosine, flush_checks
    from cave_amd.qpsolver import PreparedCones, cone_op_prepared, prepare_sparse

    ctrs, costs, sc, bad = _malformed()
    _fresh(sc.m_max, sc.d)
    B = len(costs)
    good = [i for i in range(B) if i not in bad]
    pred = torch.tensor(costs, device="cuda")
    prep = prepare_sparse(sc)
    assert isinstance(prep, PreparedCones) and prep.sparse
    assert np.array_equal(np.flatnonzero(prep.store.pack_status.cpu().numpy() == 3), bad)
    with pytest.raises(ValueError, match=r"malformed sparse cone.*6 instance\(s\), first index 1\."):
        cone_op_prepared(prep, pred, MODE_INNER, -1.0, 0.2, outputs=OUTS)
    # check=False: status 3 and NaN there, the neighbours are the clean batch's bit for bit
    o = cone_op_prepared(prepare_sparse(sc), pred, MODE_INNER, -1.0, 0.2, check=False, outputs=OUTS)
    st = o["status"].cpu().numpy()
    assert np.all(st[bad] == 3) and np.all(st[good] == 0)
    ref = cone_op_prepared(prepare_sparse(_sparse(ctrs[good])), pred[good], MODE_INNER, -1.0, 0.2, outputs=OUTS)
    for k in OUTS:
        assert bool(torch.isnan(o[k][bad]).all()) and torch.equal(o[k][good], ref[k]), k
    # check='lazy': zero loss and gradient for the rejected instances, the verdict a call later
    clean = exactConeAlignedCosine(_M(), solver="hip", reduction="none")(pred[good], prepare_sparse(_sparse(ctrs[good])))
    mod = exactConeAlignedCosine(_M(), solver="hip", reduction="none", solver_kwargs={"check": "lazy"})
    p = pred.clone().requires_grad_(True)
    loss = mod(p, prepare_sparse(sc))
    loss.sum().backward()
    assert not bool(loss.detach()[bad].any()) and not bool(p.grad[bad].any()) and bool(torch.isfinite(p.grad).all())
    assert torch.equal(loss.detach()[good], clean)
    with pytest.raises(ValueError, match="malformed sparse cone.*first index 1"):
        flush_checks()


# ------------------------------------------------------------------ 6. TOO_LARGE fallback
def test_too_large_falls_back_to_the_sparse_operator():
    import torch

    from cave_amd import qpsolver as Q
    from cave_amd.cave import innerConeAlignedCosine

    case = [c for c in LC.OUT_CASES if c.name == "d200_20f9b"][0]
    bt = _limit_batch(case)
    ctrs, costs = bt["ctrs"], bt["pred"]
    m, d = ctrs.shape[1:]
    _fresh(m, d)
    Q._sparse_split_ok.pop((m, d), None)
    sc = _sparse(ctrs)
    pred = torch.tensor(costs, device="cuda")
    early = Q.prepare_sparse(sc)            # prepared before the verdict
    prep = Q.prepare_sparse(sc)
    assert isinstance(prep, Q.PreparedCones) and isinstance(early, Q.PreparedCones)
    o = Q.cone_op_prepared(prep, pred, MODE_INNER, -1.0, 0.2, outputs=OUTS)
    assert Q._step_ok[(m, d)] is False and (o["status"] == 0).all()
    ref = Q.cone_op_dense(torch.tensor(ctrs, device="cuda"), pred, MODE_INNER, -1.0, 0.2, outputs=OUTS)
    assert float((o["loss"] - ref["loss"]).abs().max()) <= TOL
    assert float((o["grad"] - ref["grad"]).abs().max()) <= 4 * TOL * max(1.0, float(ref["grad"].abs().max()))
    assert Q.prepare_sparse(sc) is sc       # the shape is remembered: no fused step for it any more
    mod = innerConeAlignedCosine(_M(), solver="hip", seed=0, reduction="none")
    loss = mod(pred, early)                 # unwrapped to its SparseCones, not failed
    assert float((loss - ref["loss"]).abs().max()) <= TOL
    _fresh(m, d)


# ------------------------------------------------------------------ 7. prefetch
Sample = collections.namedtuple("Sample", "pred cones")


def _loaders(ctrs, costs, bs, named=False):
    import torch
    from torch.utils.data import DataLoader

    from cave_amd.sparse import SparseCones, collate_sparse

    ds_sparse = [(torch.tensor(costs[b]), SparseCones.from_dense(ctrs[b:b + 1])) for b in range(len(ctrs))]
    ds_dense = [(torch.tensor(costs[b]), torch.tensor(ctrs[b])) for b in range(len(ctrs))]
    coll = (lambda batch: Sample(*collate_sparse(batch))) if named else collate_sparse
    return DataLoader(ds_sparse, batch_size=bs, collate_fn=coll), DataLoader(ds_dense, batch_size=bs)


def test_prefetch_over_a_sparse_loader():
    import torch

    from cave_amd import synth
    from cave_amd.cave import innerConeAlignedCosine
    from cave_amd.dataset import prefetch
    from cave_amd.qpsolver import PreparedCones

    ctrs, costs, _ = synth.tsp_batch(20, 32, seed=5)
    _fresh(*ctrs.shape[1:])
    mod = innerConeAlignedCosine(_M(), solver="hip", seed=0, reduction="none")
    runs = {}
    for name, named in (("sparse", False), ("named", True), ("dense", False), ("plain", False)):
        sp, de = _loaders(ctrs, costs, 8, named=named)
        it = {"sparse": lambda: prefetch(sp), "named": lambda: prefetch(sp), "dense": lambda: prefetch(de), "plain": lambda: sp}[name]()
        losses, n = [], 0
        for batch in it:
            if name == "named":
                assert type(batch) is Sample
            pred, cones = batch
            if name != "plain":
                assert isinstance(cones, PreparedCones) and cones.sparse == (name != "dense"), (name, n)
            losses.append(mod(pred.cuda(), cones.cuda()).detach())
            n += 1
        assert n == 4
        runs[name] = torch.cat(losses)
    assert torch.equal(runs["sparse"], runs["dense"]) and torch.equal(runs["named"], runs["dense"])
    assert float((runs["sparse"] - runs["plain"]).abs().max()) <= TOL


# ------------------------------------------------------------------ 8. warm start
def test_warm_start_on_sparse_batches():
    import torch

    from cave_amd import synth
    from cave_amd.cave import innerConeAlignedCosine
    from cave_amd.dataset import prefetch

    ctrs, costs, _ = synth.tsp_batch(20, 32, seed=9)
    _fresh(*ctrs.shape[1:])
    rng = np.random.default_rng(3)
    epochs = [costs.astype(np.float32), (costs + rng.normal(0, 0.01, costs.shape)).astype(np.float32)]

    def run(kw, use_prefetch):
        mod = innerConeAlignedCosine(_M(), solver="hip", seed=0, reduction="none", solver_kwargs=kw)
        res = []
        for pred in epochs:
            sp, _ = _loaders(ctrs, pred, 8)
            ep = {"loss": [], "grad": [], "iters": [], "hit": []}
            for p, cones in (prefetch(sp) if use_prefetch else sp):
                p = p.cuda().requires_grad_(True)
                loss = mod(p, cones.cuda())
                loss.sum().backward()
                ep["loss"].append(loss.detach())
                ep["grad"].append(p.grad)
                cache = getattr(mod, "_warm", None)
                if cache is not None:
                    assert cache.last_hit is not None and bool((cache.last_status == 0).all())
                    ep["iters"].append(cache.last_iters.clone())
                    ep["hit"].append(cache.last_hit.clone())
            res.append({k: torch.cat(v) for k, v in ep.items() if v})
        return res

    cold = run(None, True)
    warm = run({"warm_start": True}, True)
    plain = run({"warm_start": True}, False)
    assert "hit" not in cold[0]
    # the cold run's iteration counts: the same solve kernel without the cache
    from cave_amd.qpsolver import cone_op_prepared, prepare_sparse

    cold_iters = [cone_op_prepared(prepare_sparse(_sparse(ctrs)), torch.tensor(p, device="cuda"), MODE_INNER, -1.0, 0.2,
                                   outputs=("loss",))["iters"] for p in epochs]
    for w in (warm, plain):
        assert not bool(w[0]["hit"].any())                       # epoch 1: every instance misses ...
        assert torch.equal(w[0]["loss"], cold[0]["loss"]) and torch.equal(w[0]["grad"], cold[0]["grad"])   # ... and is the cold run
        nonempty = torch.tensor((ctrs != 0).any(axis=(1, 2)), device="cuda")
        assert bool((w[1]["hit"][nonempty] == 1).all())          # epoch 2: every non-empty instance hits
        assert float(w[1]["iters"].float().mean()) < float(cold_iters[1].float().mean())
        assert float((w[1]["loss"] - cold[1]["loss"]).abs().max()) <= 4e-6
        assert float((w[1]["grad"] - cold[1]["grad"]).abs().max()) <= 4e-6
    assert torch.equal(warm[1]["hit"], plain[1]["hit"])


# ------------------------------------------------------------------ 9. more prepared batches than pool stores
def test_stale_sparse_prepared_batch_falls_back(golden):
    import torch

    from cave_amd import qpsolver as Q

    g = golden["structured"]
    ctrs, costs = g["sp5_ctrs"], g["sp5_costs"]
    _fresh(*ctrs.shape[1:])
    sc = _sparse(ctrs)
    pred = torch.tensor(costs, device="cuda")
    preps = [Q.prepare_sparse(sc) for _ in range(Q.STEP_POOL + 1)]
    assert preps[0].stale() and not preps[-1].stale()
    a = Q.cone_op_prepared(preps[0], pred, MODE_INNER, -1.0, 0.2, outputs=OUTS)    # cone_op_sparse on the batch it keeps
    b = Q.cone_op_prepared(preps[-1], pred, MODE_INNER, -1.0, 0.2, outputs=OUTS)
    ok = g["sp5_min_consistent"]
    for o in (a, b):
        assert (o["status"] == 0).all()
        assert np.all(np.abs(o["loss"].cpu().numpy() - g["sp5_min_inner_loss"])[ok] <= TOL)
        rg = g["sp5_min_inner_grad"]
        assert np.all(np.abs(o["grad"].cpu().numpy() - rg)[ok] <= 4 * TOL * max(1.0, float(np.abs(rg).max())))


# ------------------------------------------------------------------ 10. _get_projection
def test_get_projection_unwraps_prepared_batches(golden):
    import torch

    from cave_amd import qpsolver as Q
    from cave_amd.cave import innerConeAlignedCosine

    g = golden["structured"]
    ctrs, costs = g["tsp20_ctrs"], g["tsp20_costs"]
    _fresh(*ctrs.shape[1:])
    c = torch.tensor(ctrs, device="cuda")
    y = -torch.tensor(costs, device="cuda")
    mod = innerConeAlignedCosine(_M(), solver="hip", seed=0)
    want = mod._get_projection(y, c)
    ok = g["tsp20_min_consistent"]
    assert np.all(np.abs(want.cpu().numpy() - g["tsp20_min_inner_target"])[ok] <= 4 * TOL)
    for prep in (Q.prepare_dense(c), Q.prepare_sparse(_sparse(ctrs))):
        assert isinstance(prep, Q.PreparedCones)
        assert torch.equal(mod._get_projection(y, prep), want)


# ------------------------------------------------------------------ 11. the training example
def test_example_sparse_prefetch_equals_dense_prefetch():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_sp_cave

    base = ["--problem", "tsp", "--nodes", "10", "--num-data", "64", "--batch", "32", "--epochs", "3", "--prefetch"]
    dense = train_sp_cave.main(base)
    sparse = train_sp_cave.main(base + ["--sparse"])
    assert len(dense) == len(sparse) == 4
    for (e1, l1, r1), (e2, l2, r2) in zip(dense[1:], sparse[1:]):
        assert e1 == e2 and l1 == l2 and r1 == r2, (dense, sparse)
    train_sp_cave.main(base + ["--sparse", "--warm-start"])
    log, hits = train_sp_cave.main.iters_log, train_sp_cave.main.hit_log
    assert len(log) == 3 and len(hits) == 3
    assert all(log[e][0] < log[0][0] for e in (1, 2)), log   # fewer mean Newton iterations from epoch 2 on
    assert hits[0] < hits[1] and hits[1] > 0.5, hits
