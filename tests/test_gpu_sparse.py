"""GPU tier of the sparse wire format: cave_hip_pack_*_sparse, ConeStore.from_sparse, cone_op_sparse, the loss modules
with a SparseCones batch.

The correctness argument is bit identity with the dense route (same build_cone, same entries, different producer):
stores compared tensor by tensor with torch.equal, operator outputs with torch.equal.  Reference parity is checked on
top of that with the tolerances of tests/golden_cases.py, unchanged.
"""

import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from golden_cases import (CASES, MODE_AVG, MODE_EXACT, MODE_HEURISTIC, MODE_INNER, MODE_PROJECT, check_case, check_regress)

ALL = ("proj", "rnorm", "target", "loss", "grad")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE_ATTRS = ("n", "max_rows", "max_nnz", "lite", "large", "all_pm1", "band_entries", "max_bw", "lds_bytes", "lds_bytes_big",
               "lds_bytes_diet", "large_lds", "fits4")


def _op_impl():
    import torch

    from cave_amd.qpsolver import cone_op_sparse
    from cave_amd.sparse import SparseCones

    def impl(ctrs, costs, mode, sign, inner_ratio):
        sc = SparseCones.from_dense(np.asarray(ctrs))
        p = None if costs is None else torch.tensor(np.asarray(costs), device="cuda")
        o = cone_op_sparse(sc, p, mode, sign, inner_ratio, outputs=ALL)
        return {k: v.cpu().numpy() for k, v in o.items()}
    return impl


def _store_impl():
    import torch

    from cave_amd.dataset import ConeStore
    from cave_amd.sparse import SparseCones

    cache = {}

    def impl(ctrs, costs, mode, sign, inner_ratio):
        ctrs = np.asarray(ctrs)
        key = (ctrs.shape, ctrs.tobytes()[:4096], float(ctrs.sum()))
        if key not in cache:
            cache.clear()
            cache[key] = ConeStore.from_sparse(SparseCones.from_dense(ctrs), chunk=7)
        store = cache[key]
        ids = torch.arange(len(ctrs), device="cuda")
        p = None if costs is None else torch.tensor(np.asarray(costs), device="cuda")
        o = store.cone_op(ids, p, mode, sign, inner_ratio, outputs=ALL)
        return {k: v.cpu().numpy() for k, v in o.items()}
    return impl


# ------------------------------------------------------------------ 5. reference fixtures
@pytest.mark.parametrize("route", ["op", "store"])
@pytest.mark.parametrize("file,tag", CASES)
def test_sparse_routes_match_reference_outputs(golden, file, tag, route):
    check_case(_op_impl() if route == "op" else _store_impl(), golden, file, tag)


@pytest.mark.parametrize("route", ["op", "store"])
def test_sparse_routes_regression_fixtures(golden, route):
    check_regress(_op_impl() if route == "op" else _store_impl(), golden["regress"])


@pytest.mark.parametrize("route", ["op", "store"])
def test_sparse_routes_large_and_tsp50_fixtures(golden, route):
    """tests/golden/large.npz and tsp50.npz at the tolerances of tests/test_gpu_parity.py (4e-6 * max(1, |y|))."""
    from cave_amd import synth

    impl = _op_impl() if route == "op" else _store_impl()
    g = golden["large"]
    for tag, (h, n) in (("sp12", (12, 4)), ("sp30", (30, 1)), ("tsp100", (100, 1))):
        c, y, _ = synth.tsp_batch(h, n, seed=0) if tag == "tsp100" else synth.sp_batch(h, h, n, seed=0)
        o = impl(c, y, MODE_PROJECT, -1.0, 0.0)
        assert (o["status"] == 0).all() and o["iters"].max() <= 20
        ok = g[f"{tag}_consistent"]
        assert ok.any()
        sc = max(1.0, np.abs(y).max())
        assert np.abs(o["proj"] - g[f"{tag}_proj"])[ok].max() <= 4e-6 * sc
        assert np.abs(o["rnorm"] - g[f"{tag}_rnorm"])[ok].max() <= 4e-6 * sc
    g = golden["tsp50"]
    c, y, _ = synth.tsp_batch(int(g["n"]), int(g["batch"]), seed=int(g["seed"]))
    o = impl(c, -y, MODE_PROJECT, 1.0, 0.0)
    assert (o["status"] == 0).all()
    assert np.abs(o["proj"] - g["proj"]).max() <= 4e-6 and np.abs(o["rnorm"] - g["rnorm"]).max() <= 4e-6


# ------------------------------------------------------------------ 6. store identity on the device
@pytest.mark.parametrize("kind,size,B,chunk", [("tsp", 20, 256, 32), ("tsp", 50, 64, 16), ("tsp", 100, 16, 8), ("sp", (30, 30), 32, 16)])
def test_store_from_sparse_equals_store_from_dense(kind, size, B, chunk):
    """Every tensor and every derived figure of ConeStore.from_sparse equals that of from_chunks_lazy(densify_on), and
    so do the outputs of cone_op.  Both routes are given the same chunk size: the tier ladder is walked per chunk, so
    each cone is then packed by the same kernel shape on both routes (a chunk whose cones all fit the default limits
    is packed by two waves, another by the wide shape), and no tolerance is needed for `avg`."""
    import torch

    from cave_amd import synth
    from cave_amd.dataset import ConeStore
    from cave_amd.sparse import SparseCones

    dev = torch.device("cuda")
    items, costs, _ = synth.coo_batch(kind, size, B, seed=0)
    d = costs.shape[1]
    m_max = max(it[3] for it in items)
    dense = ConeStore.from_chunks_lazy(lambda i: synth.densify_on(items[i:i + chunk], d, dev, m_max), list(range(0, B, chunk)))
    sparse = ConeStore.from_sparse(SparseCones.from_coo(items, d), chunk=chunk)
    assert set(dense.t) == set(sparse.t)
    for k in dense.t:
        assert dense.t[k].dtype == sparse.t[k].dtype and torch.equal(dense.t[k], sparse.t[k]), k
    for a in STORE_ATTRS:
        assert getattr(dense, a) == getattr(sparse, a), a
    assert (dense.rb_cache is None) == (sparse.rb_cache is None) and (dense.lite_slots is None) == (sparse.lite_slots is None)
    if dense.lite_slots is not None:
        for k in dense.lite_slots.t:
            assert torch.equal(dense.lite_slots.t[k], sparse.lite_slots.t[k]), k
    ids = torch.arange(B, device=dev)
    pred = torch.tensor(costs, device=dev)
    for mode in (MODE_EXACT, MODE_INNER):
        a = dense.cone_op(ids, pred, mode, -1.0, 0.2, outputs=ALL)
        b = sparse.cone_op(ids, pred, mode, -1.0, 0.2, outputs=ALL)
        assert bool((a["status"] == 0).all())
        for k in ALL + ("status", "iters"):
            assert torch.equal(a[k], b[k]), (mode, k)


def test_from_sparse_shard_partitions_by_entry_counts():
    import torch

    from cave_amd import synth
    from cave_amd.dataset import ConeStore
    from cave_amd.dist import weighted_shards
    from cave_amd.sparse import SparseCones

    items, costs, _ = synth.coo_batch("tsp", 20, 24, seed=4)
    sc = SparseCones.from_coo(items, 190)
    full = ConeStore.from_sparse(sc)
    shards = weighted_shards([len(it[0]) for it in items], 3)
    pred = torch.tensor(costs, device="cuda")
    seen = []
    for rank in range(3):
        st = ConeStore.from_sparse_shard(sc, rank, 3)
        assert st.global_ids.tolist() == [int(i) for i in shards[rank]] and st.shard == (rank, 3)
        gi = st.global_ids.cuda()
        a = st.cone_op(st.local_ids(st.global_ids).cuda(), pred[gi], MODE_EXACT, -1.0, outputs=("loss", "grad"))
        b = full.cone_op(gi, pred[gi], MODE_EXACT, -1.0, outputs=("loss", "grad"))
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["grad"], b["grad"])
        seen += st.global_ids.tolist()
    assert sorted(seen) == list(range(24))


# ------------------------------------------------------------------ 7. split form
def _slot_fill_both(ctrs_dev, sc_dev):
    """The two slot-mode fills, four waves each, into separate slot stores: (dense store, sparse store)."""
    from cave_amd import _lib
    from cave_amd.qpsolver import _SlotStore

    lib = _lib.load()
    B, m, d = ctrs_dev.shape
    sd, ss = _SlotStore(ctrs_dev.device, B, d), _SlotStore(ctrs_dev.device, B, d)
    _lib.check(lib.cave_hip_pack_fill(_lib.ptr(ctrs_dev), B, m, d, 0, 0, 4, sd.ref, 0, _lib.ptr(sd.pack_status),
                                      _lib.current_stream()), "cave_hip_pack_fill")
    _lib.check(lib.cave_hip_pack_fill_sparse(sc_dev.c_ref(), 0, 0, 4, ss.ref, 0, _lib.ptr(ss.pack_status),
                                             _lib.current_stream()), "cave_hip_pack_fill_sparse")
    return sd, ss


def _assert_same_live_slots(sd, ss, B, d):
    import torch

    from cave_amd.qpsolver import SPLIT_NNZ, SPLIT_ROWS

    assert bool((sd.pack_status == 0).all()) and torch.equal(sd.pack_status, ss.pack_status)
    for k in ("n_rows", "n_nnz", "n_valid", "flags", "usign", "avg", "cptr"):
        assert torch.equal(sd.t[k], ss.t[k]), k
    rows = torch.arange(SPLIT_ROWS, device=sd.t["n_rows"].device)[None, :] < sd.t["n_rows"][:, None]
    nnz = torch.arange(SPLIT_NNZ, device=rows.device)[None, :] < sd.t["n_nnz"][:, None]
    for k in ("vkind", "rlo", "rhi"):
        assert torch.equal(sd.t[k].view(B, SPLIT_ROWS)[rows], ss.t[k].view(B, SPLIT_ROWS)[rows]), k
    for k in ("ccol", "cval", "cvar", "cvalc"):
        assert torch.equal(sd.t[k].view(B, SPLIT_NNZ)[nnz], ss.t[k].view(B, SPLIT_NNZ)[nnz]), k


@pytest.mark.parametrize("what", ["tsp20", "sp5"])
def test_split_form_sparse_equals_dense(what):
    import torch

    from cave_amd import qpsolver, synth
    from cave_amd.qpsolver import cone_op_dense, cone_op_sparse
    from cave_amd.sparse import SparseCones

    if what == "tsp20":
        B = 1024
        items, costs, _ = synth.coo_batch("tsp", 20, B, seed=0)
        d = 190
    else:
        B = 100
        items, costs, _ = synth.coo_batch("sp", (5, 5), B, seed=0)
        d = 40
    sc = SparseCones.from_coo(items, d).cuda()
    ctrs = sc.densify()
    m = sc.m_max
    sd, ss = _slot_fill_both(ctrs, sc)
    _assert_same_live_slots(sd, ss, B, d)
    pred = torch.tensor(costs, device="cuda")
    qpsolver.forget_shape(m, d)
    for mode in (MODE_PROJECT, MODE_EXACT, MODE_INNER, MODE_HEURISTIC, MODE_AVG):
        sign = 1.0 if mode in (MODE_PROJECT, MODE_AVG) else -1.0
        # (the outputs a mode defines: PROJECT leaves target / loss / grad unwritten, AVG writes the target only)
        outs = {MODE_PROJECT: ("proj", "rnorm"), MODE_AVG: ("target",), MODE_HEURISTIC: ("target", "loss", "grad")}.get(mode, ALL)
        a = cone_op_dense(ctrs, None if mode == MODE_AVG else pred, mode, sign, 0.2, outputs=outs)
        assert qpsolver._split_ok[(m, d)] is True   # the dense call took the split form: the same solve launch
        b = cone_op_sparse(sc, None if mode == MODE_AVG else pred, mode, sign, 0.2, outputs=outs)
        assert qpsolver._sparse_split_ok[(m, d)] is True
        assert bool((a["status"] == 0).all())
        for k in outs + ("status", "iters"):
            assert torch.equal(a[k], b[k]), (mode, k)
    # a host batch is moved by the call; project_hip_sparse is cone_op_sparse in PROJECT mode
    from cave_amd.qpsolver import project_hip, project_hip_sparse

    p1, r1 = project_hip(ctrs, -pred)
    p2, r2 = project_hip_sparse(SparseCones.from_coo(items, d), -pred)
    assert torch.equal(p1, p2) and torch.equal(r1, r2)


# ------------------------------------------------------------------ 8. loss modules
class _Model:
    def __init__(self, sense):
        self.modelSense = sense


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_loss_modules_with_sparse_batches(reduction):
    import torch

    from cave_amd import synth
    from cave_amd.cave import EPO, exactConeAlignedCosine, innerConeAlignedCosine
    from cave_amd.sparse import SparseCones

    items, costs, _ = synth.coo_batch("tsp", 20, 48, seed=2)
    sc = SparseCones.from_coo(items, 190)
    ctrs = sc.densify("cuda")
    for sense in (EPO.MINIMIZE, EPO.MAXIMIZE):
        for make in (lambda: exactConeAlignedCosine(_Model(sense), solver="hip", reduction=reduction),
                     lambda: innerConeAlignedCosine(_Model(sense), solver="hip", reduction=reduction, seed=3)):
            out = []
            for cones in (ctrs, sc, sc.cuda()):
                mod = make()
                pred = torch.tensor(costs, device="cuda", requires_grad=True)
                loss = mod(pred, cones)
                loss.sum().backward()
                out.append((loss.detach().clone(), pred.grad.clone()))
            for loss, grad in out[1:]:
                assert torch.equal(loss, out[0][0]) and torch.equal(grad, out[0][1])
            # _get_projection: the constant target for a sense-flipped cost
            mod = make()
            t1 = mod._get_projection(torch.tensor(-costs, device="cuda"), ctrs)
            mod = make()
            t2 = mod._get_projection(torch.tensor(-costs, device="cuda"), sc)
            assert torch.equal(t1, t2)


def test_hybrid_branch_sequence_is_unchanged():
    import torch

    from cave_amd import _lib, synth
    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.sparse import SparseCones

    items, costs, _ = synth.coo_batch("tsp", 20, 16, seed=5)
    sc = SparseCones.from_coo(items, 190).cuda()
    ctrs = sc.densify()
    pred = torch.tensor(costs, device="cuda")
    a = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", solve_ratio=0.5, seed=7)
    b = innerConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", solve_ratio=0.5, seed=7)
    ref = np.random.RandomState(7)
    modes = []
    for _ in range(8):
        la, lb = a(pred, ctrs), b(pred, sc)
        assert torch.equal(la, lb)
        modes.append(_lib.MODE_HEURISTIC if ref.uniform() > 0.5 else _lib.MODE_INNER)
    assert len(set(modes)) == 2   # both branches were drawn
    # the modules drew the same numbers as the reference stream: their next draw is the stream's ninth
    nxt = ref.uniform()
    assert a._branch_rng.uniform() == nxt and b._branch_rng.uniform() == nxt


def test_lazy_check_masks_a_rejected_instance():
    import torch

    from cave_amd import synth
    from cave_amd.cave import EPO, exactConeAlignedCosine, flush_checks
    from cave_amd.sparse import SparseCones

    items, costs, _ = synth.coo_batch("tsp", 20, 8, seed=6)
    sc = SparseCones.from_coo(items, 190)
    good = exactConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none")(torch.tensor(costs, device="cuda"), sc)
    val = sc.val.clone()
    val[int(sc.ent_off[2]) + 5] = float("inf")
    bad = SparseCones(sc.m_max, sc.d, sc.ent_off, sc.key, val)
    mod = exactConeAlignedCosine(_Model(EPO.MINIMIZE), solver="hip", reduction="none", solver_kwargs={"check": "lazy"})
    pred = torch.tensor(costs, device="cuda", requires_grad=True)
    loss = mod(pred, bad)
    loss.sum().backward()
    keep = torch.arange(8, device="cuda") != 2
    assert float(loss[2].detach()) == 0.0 and not bool(pred.grad[2].any()) and bool(torch.isfinite(pred.grad).all())
    assert torch.equal(loss[keep], good[keep])
    with pytest.raises(ValueError, match="malformed sparse cone.*first index 2"):
        flush_checks()


# ------------------------------------------------------------------ 9. malformed input through the public API
def _malformed(B0=14):
    import torch

    from cave_amd import synth
    from cave_amd.sparse import SparseCones
    from test_sparse_cpu import malformed_batch

    ctrs, costs, _ = synth.tsp_batch(20, B0, seed=8)
    off, key, val, bad = malformed_batch(ctrs)
    sc = SparseCones(ctrs.shape[1], ctrs.shape[2], torch.from_numpy(off.copy()), torch.from_numpy(key.view(np.int32).copy()),
                     torch.from_numpy(val.copy()))
    return ctrs, costs, sc, bad


def test_malformed_instances_raise_value_error():
    import torch

    from cave_amd.dataset import ConeStore
    from cave_amd.qpsolver import cone_op_sparse

    ctrs, costs, sc, bad = _malformed()
    pred = torch.tensor(costs, device="cuda")
    with pytest.raises(ValueError, match=r"malformed sparse cone.*6 instance\(s\), first index 1\."):
        cone_op_sparse(sc, pred, MODE_PROJECT)
    with pytest.raises(ValueError, match="malformed sparse cone.*first index 1"):
        ConeStore.from_sparse(sc)
    with pytest.raises(ValueError, match="malformed sparse cone.*first index 11"):
        ConeStore.from_sparse(sc[[0, 2, 4, 6, 8, 10, 12, 13, 0, 2, 4, 11]], chunk=8)   # index in the batch, not in its chunk


@pytest.mark.parametrize("route", ["split", "store"])
def test_malformed_instance_unchecked_leaves_status_and_neighbours(route):
    """check=False: status 3 and NaN outputs at the rejected instances, the others bit-equal to the dense call on the
    good cones.  The inputs are rejected by value checks in the loader; nothing here relies on a memory fault."""
    import torch

    from cave_amd import qpsolver
    from cave_amd.qpsolver import cone_op_dense, cone_op_sparse

    ctrs, costs, sc, bad = _malformed()
    B = len(costs)
    good = [i for i in range(B) if i not in bad]
    pred = torch.tensor(costs, device="cuda")
    if route == "store":
        qpsolver._sparse_split_ok[(sc.m_max, sc.d)] = False   # as after a batch that did not fit the split form
    try:
        o = cone_op_sparse(sc, pred, MODE_INNER, -1.0, 0.2, check=False, outputs=ALL)
    finally:
        qpsolver._sparse_split_ok.pop((sc.m_max, sc.d), None)
    st = o["status"].cpu().numpy()
    assert np.all(st[bad] == 3) and np.all(st[good] == 0)
    for k in ALL:
        assert bool(torch.isnan(o[k][bad]).all()), k
    if route == "split":
        ref = cone_op_dense(torch.tensor(ctrs[good], device="cuda"), pred[good], MODE_INNER, -1.0, 0.2, outputs=ALL)
        for k in ALL:
            assert torch.equal(o[k][good], ref[k]), k
    else:
        # The transient store holds empty slots for the rejected instances, so it is not an all-+-1 store and its batch
        # is served by the general solver, where the dense call on the good cones alone takes the one-wave solver for
        # small +-1 cones: two fp64 solves of the same (unique) projection, rounded to fp32.  Compared at the
        # tolerances tests/golden_cases.py states for such outputs.
        ref = cone_op_dense(torch.tensor(ctrs[good], device="cuda"), pred[good], MODE_INNER, -1.0, 0.2, outputs=ALL)
        sc_y = max(1.0, float(np.abs(costs).max()))
        for k, tol in (("proj", 2e-6 * sc_y), ("rnorm", 2e-6 * sc_y), ("loss", 2e-6), ("target", 8e-6), ("grad", 8e-6)):
            scale = max(1.0, float(ref[k].abs().max())) if k == "grad" else 1.0
            assert float((o[k][good] - ref[k]).abs().max()) <= tol * scale, k


# ------------------------------------------------------------------ 10. no dense staging
def test_tsp100_store_build_peak_memory_is_below_the_dense_route():
    import torch

    from cave_amd import synth
    from cave_amd.dataset import ConeStore
    from cave_amd.sparse import SparseCones

    dev = torch.device("cuda")
    B, chunk = 32, 8
    items, costs, _ = synth.coo_batch("tsp", 100, B, seed=1)
    d = costs.shape[1]
    m_max = max(it[3] for it in items)
    sc = SparseCones.from_coo(items, d)
    peaks = {}
    for route in ("sparse", "dense"):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if route == "sparse":
            store = ConeStore.from_sparse(sc)
        else:
            store = ConeStore.from_chunks_lazy(lambda i: synth.densify_on(items[i:i + chunk], d, dev, m_max), list(range(0, B, chunk)))
        torch.cuda.synchronize()
        peaks[route] = torch.cuda.max_memory_allocated() - base
        assert store.n == B and store.large
        del store
    print(f"peak device memory of the TSP-100 B = {B} store build: sparse {peaks['sparse'] / 2**20:.1f} MiB, "
          f"dense (chunks of {chunk}) {peaks['dense'] / 2**20:.1f} MiB")
    assert peaks["sparse"] < peaks["dense"], peaks


# ------------------------------------------------------------------ 11. the example
@pytest.mark.parametrize("packed", [False, True])
def test_example_sparse_run_equals_dense_run(packed):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_sp_cave

    base = ["--grid", "5", "5", "--num-data", "40", "--batch", "16", "--epochs", "3"] + (["--packed"] if packed else [])
    dense = train_sp_cave.main(base)
    sparse = train_sp_cave.main(base + ["--sparse"])
    assert len(dense) == len(sparse) == 4
    for (e1, l1, r1), (e2, l2, r2) in zip(dense[1:], sparse[1:]):
        assert e1 == e2 and l1 == l2 and r1 == r2, (dense, sparse)
