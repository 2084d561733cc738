"""GPU tier: warm start of the fused small-cone step (cave_hip_cone_step_warm, cave_amd/warm.py).

The solve half of the step kernel starts each instance from the multipliers its cone ended with last time -- dense
batches keyed by the content of the reduced cone, a device-resident store by slot.  A miss computes exactly what the
cold kernel computes; a hit converges to the same projection in fewer Newton iterations; nothing in the cache can
change a result."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = ("proj", "rnorm", "target", "loss", "grad")


class _M:
    from cave_amd.abcmodule import EPO

    modelSense = EPO.MINIMIZE


def _tol(k, sc):
    return 4e-6 * (sc if k in ("proj", "rnorm") else 4.0)


def _sources(golden):
    from cave_amd import synth

    ctrs, costs, _ = synth.tsp_batch(20, 1024, seed=21)
    g = golden["structured"]
    return [("synth", ctrs, costs), ("structured", g["tsp20_ctrs"], g["tsp20_costs"])]


@pytest.mark.parametrize("leg", ["dense", "prefetch"])
def test_module_warm_start_matches_cold_and_saves_iterations(golden, leg):
    import torch

    from cave_amd.cave import innerConeAlignedCosine
    from cave_amd.dataset import prefetch
    from cave_amd.qpsolver import MODE_INNER, cone_op_dense, prepare_dense

    for name, ctrs, costs in _sources(golden):
        B = len(ctrs)
        c = torch.tensor(ctrs, device="cuda")
        sc = float(np.abs(costs).max())
        warm = innerConeAlignedCosine(_M(), solver="hip", solver_kwargs={"warm_start": True}, seed=0, reduction="none")
        cold = innerConeAlignedCosine(_M(), solver="hip", seed=0, reduction="none")
        rng = np.random.default_rng(7)
        preds = [costs.astype(np.float32)]
        for _ in range(4):
            preds.append(preds[-1] + rng.normal(0, 0.01, costs.shape).astype(np.float32))
        batches = prefetch([(torch.tensor(p), c) for p in preds]) if leg == "prefetch" else [(torch.tensor(p), c) for p in preds]
        its = []
        for step, (p, cones) in enumerate(batches):
            p = p.cuda()
            pw = p.clone().requires_grad_(True)
            lw = warm(pw, cones)
            lw.sum().backward()
            cache = warm._warm
            assert cache is not None and cache.last_hit is not None, (name, leg, step)  # the warm kernel served it
            assert bool((cache.last_status == 0).all()), (name, leg, step)
            # cold twin through the same kernel (bit-identical on a miss) and through the general operator
            pc = p.clone().requires_grad_(True)
            lc = cold(pc, prepare_dense(c))
            lc.sum().backward()
            ref = cone_op_dense(c, p, MODE_INNER, -1.0, 0.2, outputs=ALL)
            for k, a, b in (("loss", lw, lc), ("grad", pw.grad, pc.grad), ("loss", lw, ref["loss"]), ("grad", pw.grad, ref["grad"])):
                assert float((a.detach() - b).abs().max()) <= _tol(k, sc), (name, leg, step, k)
            if step == 0:  # every instance misses: exactly the cold kernel
                assert not bool(cache.last_hit.any())
                assert torch.equal(lw.detach(), lc.detach()) and torch.equal(pw.grad, pc.grad), (name, leg)
                assert torch.equal(cache.last_iters, ref["iters"]), (name, leg)
            if step >= 2:
                assert bool((cache.last_hit == 1).all()), (name, leg, step)
            its.append((float(ref["iters"].float().mean()), float(cache.last_iters.float().mean())))
        assert its[-1][1] <= 3.0 and its[-1][1] <= its[-1][0] - 1.5, (name, leg, its)
        # the target (a projection with the same cache) matches the cold target too
        from cave_amd.qpsolver import cone_op_prepared

        pt = torch.tensor(preds[-1], device="cuda")
        got = cone_op_prepared(prepare_dense(c), pt, MODE_INNER, -1.0, 0.2, outputs=ALL, warm=warm._warm)
        for k in ALL:
            assert float((got[k] - ref[k]).abs().max()) <= _tol(k, sc), (name, k)
        assert B == len(ctrs)


def _prepared(c, p, warm=None, **kw):
    from cave_amd.qpsolver import MODE_INNER, cone_op_prepared, prepare_dense

    return cone_op_prepared(prepare_dense(c), p, MODE_INNER, -1.0, 0.2, outputs=ALL, warm=warm, **kw)


def test_cache_contents_never_change_results():
    import torch

    from cave_amd import synth
    from cave_amd.warm import WarmCache

    ctrs, costs, _ = synth.tsp_batch(20, 256, seed=22)
    c = torch.tensor(ctrs, device="cuda")
    sc = float(np.abs(costs).max())
    rng = np.random.default_rng(8)
    p0 = torch.tensor(costs, device="cuda")
    p1 = p0 + torch.tensor(rng.normal(0, 0.01, costs.shape).astype(np.float32), device="cuda")
    cold = _prepared(c, p1)
    cache = WarmCache(device="cuda")
    assert _prepared(c, p0, cache)["status"].eq(0).all()
    for fill in ("nan", "big", "-big", "random"):
        th = {"nan": torch.full_like(cache.theta, float("nan")), "big": torch.full_like(cache.theta, 1e30),
              "-big": torch.full_like(cache.theta, -1e30),
              "random": torch.randn(cache.theta.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(3)) * 5}[fill]
        cache.theta.copy_(th)
        o = _prepared(c, p1, cache)
        assert bool((o["warm_hit"] == 1).all()) and bool((o["status"] == 0).all()), fill
        for k in ALL:
            assert float((o[k] - cold[k]).abs().max()) <= _tol(k, sc), (fill, k)
        _prepared(c, p0, cache)  # (good multipliers again for the next round)
    tiny = WarmCache(4, device="cuda")  # one set of four ways: 256 cones thrash it
    assert tiny.n == 4
    for _ in range(3):
        o = _prepared(c, p1, tiny)
        assert bool((o["status"] == 0).all())
        for k in ALL:
            assert float((o[k] - cold[k]).abs().max()) <= _tol(k, sc), k


def test_nan_prediction_invalidates_only_its_entry():
    import torch

    from cave_amd.cave import flush_checks, innerConeAlignedCosine
    from cave_amd.qpsolver import prepare_dense

    from cave_amd import synth

    ctrs, costs, _ = synth.tsp_batch(20, 128, seed=23)
    c = torch.tensor(ctrs, device="cuda")
    mod = innerConeAlignedCosine(_M(), solver="hip", seed=0, reduction="none",
                                 solver_kwargs={"warm_start": True, "check": "lazy"})
    p = torch.tensor(costs, device="cuda")
    for _ in range(2):
        mod(p.clone().requires_grad_(True), c)  # (the first call of a shape runs strict; both populate the cache)
    flush_checks()
    bad = p.clone()
    bad[5, 3] = float("nan")
    pb = bad.requires_grad_(True)
    loss = mod(pb, prepare_dense(c))
    loss.sum().backward()
    cache = mod._warm
    torch.cuda.synchronize()
    ls = cache.last_status.cpu()
    assert int(ls[5]) == 3 and bool((ls[torch.arange(128) != 5] == 0).all())
    assert float(loss[5]) == 0.0 and bool((pb.grad[5] == 0).all()) and bool(torch.isfinite(pb.grad).all())
    with pytest.raises(ValueError):
        flush_checks()
    mod(p.clone().requires_grad_(True), c)
    flush_checks()
    hit = cache.last_hit.cpu()
    assert int(hit[5]) == 0 and bool((hit[torch.arange(128) != 5] == 1).all())


def test_repeated_cones_in_one_batch_and_repeated_ids():
    import torch

    from cave_amd import synth
    from cave_amd.dataset import ConeStore
    from cave_amd.qpsolver import MODE_INNER, cone_op_dense
    from cave_amd.warm import WarmCache

    ctrs, costs, _ = synth.tsp_batch(20, 6, seed=24)
    idx = np.arange(96) % 6
    c = torch.tensor(ctrs[idx], device="cuda")
    rng = np.random.default_rng(9)
    base = costs[idx] + rng.normal(0, 0.05, (96, costs.shape[1])).astype(np.float32)
    sc = float(np.abs(base).max())
    cache = WarmCache(device="cuda")
    for step in range(3):
        p = torch.tensor(base + rng.normal(0, 0.01, base.shape).astype(np.float32), device="cuda")
        o = _prepared(c, p, cache)
        ref = cone_op_dense(c, p, MODE_INNER, -1.0, 0.2, outputs=ALL)
        assert bool((o["status"] == 0).all()), step
        assert bool((o["warm_hit"] == (1 if step >= 1 else 0)).all()), step  # 16 copies of each cone share one entry
        for k in ALL:
            assert float((o[k] - ref[k]).abs().max()) <= _tol(k, sc), (step, k)
    # a device-resident store: repeated ids in one batch
    warm, cold = ConeStore.from_dense(torch.tensor(ctrs, device="cuda")), ConeStore.from_dense(torch.tensor(ctrs, device="cuda"))
    warm.enable_warm_start()
    ids = torch.tensor(idx, device="cuda")
    for step in range(3):
        p = torch.tensor(base + rng.normal(0, 0.01, base.shape).astype(np.float32), device="cuda")
        a = cold.cone_op(ids, p, MODE_INNER, -1.0, 0.2, outputs=ALL)
        b = warm.cone_op(ids, p, MODE_INNER, -1.0, 0.2, outputs=ALL)
        assert "warm_hit" in b and bool((b["status"] == 0).all())
        assert bool((b["warm_hit"] == (1 if step >= 1 else 0)).all()), step
        for k in ALL:
            assert float((a[k] - b[k]).abs().max()) <= _tol(k, sc), (step, k)


def test_content_key_ignores_batch_position_and_padding():
    """The same cones in another order, padded to another m_max, hit the entries an earlier batch left; cones that
    share their reduced rows but not their unit rows do not hit each other's entries."""
    import torch

    from cave_amd import synth
    from cave_amd.qpsolver import PreparedCones, prepare_dense
    from cave_amd.warm import WarmCache

    ctrs, costs, _ = synth.tsp_batch(20, 256, seed=27)
    rows = (ctrs != 0).any(axis=2).sum(axis=1)
    rng = np.random.default_rng(11)
    sub = rng.permutation(np.argsort(rows, kind="stable")[:128])   # the smaller half, shuffled
    m2 = int(rows[sub].max())
    assert m2 < ctrs.shape[1]
    c, c2 = torch.tensor(ctrs, device="cuda"), torch.tensor(np.ascontiguousarray(ctrs[sub][:, :m2]), device="cuda")
    assert isinstance(prepare_dense(c2), PreparedCones)
    p = torch.tensor(costs, device="cuda")
    cache = WarmCache(device="cuda")
    assert not bool(_prepared(c, p, cache)["warm_hit"].any())
    p2 = p[torch.tensor(sub, device="cuda")] + 0.01 * torch.randn(128, p.shape[1], device="cuda",
                                                                  generator=torch.Generator("cuda").manual_seed(5))
    o, cold = _prepared(c2, p2, cache), _prepared(c2, p2)
    assert bool((o["warm_hit"] == 1).all()) and bool((o["status"] == 0).all())
    assert float(o["iters"].float().mean()) <= float(cold["iters"].float().mean()) - 1.0
    sc = float(np.abs(costs).max())
    for k in ALL:
        assert float((o[k] - cold[k]).abs().max()) <= _tol(k, sc), k
    # one cone with a unit row dropped: same reduced rows, another cone -- it must not take the entry of the original
    u = ctrs[:1].copy()
    unit = np.nonzero((u[0] != 0).sum(axis=1) == 1)[0]
    assert unit.size > 0
    u[0, unit[0]] = 0.0
    o = _prepared(torch.tensor(u, device="cuda"), p[:1], cache)
    assert int(o["warm_hit"][0]) == 0 and int(o["status"][0]) == 0


def test_same_cache_contents_same_outputs():
    import torch

    from cave_amd import synth
    from cave_amd.warm import WarmCache

    ctrs, costs, _ = synth.tsp_batch(20, 256, seed=25)
    c = torch.tensor(ctrs, device="cuda")
    rng = np.random.default_rng(10)
    p0 = torch.tensor(costs, device="cuda")
    p1 = p0 + torch.tensor(rng.normal(0, 0.01, costs.shape).astype(np.float32), device="cuda")
    cache = WarmCache(device="cuda")
    _prepared(c, p0, cache)
    key, theta = cache.key.clone(), cache.theta.clone()
    a = _prepared(c, p1, cache)
    cache.key.copy_(key)
    cache.theta.copy_(theta)
    b = _prepared(c, p1, cache)
    assert bool((a["warm_hit"] == 1).all())
    for k in ALL + ("status", "iters", "warm_hit"):
        assert torch.equal(a[k], b[k]), k


def test_abi_warm_null_is_the_cold_step():
    """cave_hip_cone_step_warm with warm = NULL: bit-identical to cave_hip_cone_step; a bad cache is refused."""
    import ctypes as C

    import torch

    from cave_amd import _lib, synth
    from cave_amd.qpsolver import _tickets_for, prepare_dense

    lib = _lib.load()
    ctrs, costs, _ = synth.tsp_batch(20, 128, seed=26)
    c = torch.tensor(ctrs, device="cuda")
    p = torch.tensor(costs, device="cuda")
    B, d = p.shape
    outs = []
    for fn in ("cave_hip_cone_step", "cave_hip_cone_step_warm"):
        prep = prepare_dense(c)
        o = {k: torch.empty((B,) if k in ("rnorm", "loss") else (B, d), device="cuda") for k in ALL}
        st = torch.empty(B, dtype=torch.int32, device="cuda")
        it = torch.empty(B, dtype=torch.int32, device="cuda")
        args = [prep.store.ref, None, _lib.ptr(p), B, 2, -1.0, 0.2, 0, 0] + [_lib.ptr(o[k]) for k in ALL] + \
            [_lib.ptr(st), _lib.ptr(it), None, 0, 0, d, None, None]
        if fn.endswith("warm"):
            args += [None, None, None]
        rc = getattr(lib, fn)(*args, _lib.ptr(_tickets_for(c.device)), _lib.current_stream())
        assert rc == 0, lib.cave_hip_last_error()
        outs.append((o, st, it))
    (o1, s1, i1), (o2, s2, i2) = outs
    assert torch.equal(s1, s2) and torch.equal(i1, i2) and bool((s1 == 0).all())
    for k in ALL:
        assert torch.equal(o1[k], o2[k]), k
    key = torch.zeros(8, dtype=torch.int64, device="cuda")
    theta = torch.zeros(8 * 32 + 4, dtype=torch.float32, device="cuda")
    for n, kp, tp in ((6, key.data_ptr(), theta.data_ptr()), (8, None, theta.data_ptr()), (8, key.data_ptr(), theta.data_ptr() + 4)):
        w = _lib.WarmCacheC(n_entries=n, key=kp, theta=tp)
        args = [prep.store.ref, None, _lib.ptr(p), B, 2, -1.0, 0.2, 0, 0] + [None] * 7 + [None, 0, 0, d, None, None]
        assert lib.cave_hip_cone_step_warm(*args, C.byref(w), None, None, _lib.ptr(_tickets_for(c.device)),
                                           _lib.current_stream()) == -1


def test_cone_store_warm_start_uses_the_lite_slots(golden):
    import torch

    from cave_amd.dataset import ConeStore
    from cave_amd.qpsolver import MODE_INNER

    g = golden["structured"]
    ctrs, costs = g["tsp20_ctrs"], g["tsp20_costs"]
    s = ConeStore.from_dense(torch.tensor(ctrs, device="cuda"))
    assert s.lite_slots is not None
    n0 = s.nbytes()
    s.enable_warm_start()
    assert s.nbytes() >= n0 + s.lite_warm.nbytes
    ids = torch.arange(len(ctrs), device="cuda")
    p = torch.tensor(costs, device="cuda")
    a = s.cone_op(ids, p, MODE_INNER, -1.0, 0.2, outputs=ALL)
    b = s.cone_op(ids, p, MODE_INNER, -1.0, 0.2, outputs=ALL)
    assert "warm_hit" in a and not bool(a["warm_hit"].any()) and bool((b["warm_hit"] == 1).all())
    assert float(b["iters"].float().mean()) < float(a["iters"].float().mean())
    s.reset_warm_start()
    c = s.cone_op(ids, p, MODE_INNER, -1.0, 0.2, outputs=ALL)
    assert not bool(c["warm_hit"].any()) and torch.equal(c["iters"], a["iters"])


def test_training_example_dense_prefetch_warm_start():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_sp_cave

    # shuffled batches of 32 out of 64, each padded to its own m_max: the cones come back at other batch positions and
    # paddings every epoch, so hits from epoch 2 on show that the content key depends on the cone only
    hist = train_sp_cave.main(["--problem", "tsp", "--nodes", "9", "--num-data", "64", "--batch", "32", "--epochs", "6",
                               "--prefetch", "--warm-start"])
    assert hist[-1][2] < hist[0][2], hist
    log, hits = train_sp_cave.main.iters_log, train_sp_cave.main.hit_log   # (from the loss module's multiplier cache)
    assert len(log) == 6 and len(hits) == 6, (log, hits)
    assert all(h == 1.0 for h in hits[1:]), hits
    assert all(m <= 3.0 for m, _ in log[1:]), log
