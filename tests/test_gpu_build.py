"""GPU tier: the cone build ALONE on the MI355X, against the plain restatement of the reduction (tests/build_ref.py).

The cases, the restatement and the comparisons are those of tests/test_build_emul.py (tests/build_cases.py,
tests/build_check.py): every pack route of the C ABI writes its store on the device, the store is copied back and
decoded on the host, and p, vkind, usign, n_valid, flag bit 0, every reduced row and every CSC column must equal the
restated rules EXACTLY, avg within the bound derived in build_ref.  Family C (colliding 12-entry signatures) is held to
build_ref.is_valid_reduction and to the oracle's projection instead: the build may leave such twins unpaired.

Routes: cave_hip_pack_count + cave_hip_pack_fill at waves 1, 2, 4, 8 (exact-fit stores) and at waves 4 into a slot-mode
store, cave_hip_pack_large, cave_hip_pack_count_sparse + cave_hip_pack_fill_sparse at waves 2, 4, 8,
cave_hip_pack_large_sparse, the pack-only launch of cave_hip_cone_step and of cave_hip_cone_step_sparse, and
cave_hip_lite_from_packed.  The worst |avg - ref| / bound per route goes into profiles/build_margins.json (tier
"mi355x"; the environment variable CAVE_BUILD_MARGINS names another file)."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

import build_cases as BC
import build_ref as BR
import limit_cones as LC
from build_check import FULL_LDS, ST_TOO_LARGE, cases_of, check_lite, check_store, lite_must_pack, nnz_cap, refs_of
from golden_cases import MODE_PROJECT, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STORE_KEYS = ("row_off", "nnz_off", "n_valid", "flags", "usign", "avg", "vkind", "rlo", "rhi", "ccol", "cval", "cptr", "cvar",
              "cvalc", "n_rows", "n_nnz")
LITE_KEYS = ("hdr", "usign", "avg", "rowptr", "ell", "csr16", "rl")


@pytest.fixture(scope="module")
def gpu():
    import torch

    from cave_amd import _lib

    lib = _lib.load()
    yield lib, _lib, torch
    BR.dump_margins("mi355x", default=os.path.join(ROOT, "profiles", "build_margins.json"))


def host(t):
    return {k: v.cpu().numpy() for k, v in t.items() if k in STORE_KEYS + LITE_KEYS}


def on_device(torch, ctrs):
    """the batch on the device and the pointer the C ABI takes (a batch without rows has no bytes: the ABI wants a
    non-null pointer, which the kernels then never read)"""
    x = torch.tensor(ctrs, device="cuda")
    return x, (x if x.numel() else torch.zeros(4, device="cuda"))


def exact_store(gpu, B, d, count):
    """count pass -> exact-fit store -> (tensors, struct, status tensor)"""
    lib, _lib, torch = gpu
    n_rows = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    n_nnz = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    count(n_rows, n_nnz, status)
    assert bool((status == 0).all()), status
    z = torch.zeros(1, dtype=torch.int64, device="cuda")
    row_off = torch.cat([z, torch.cumsum(n_rows.to(torch.int64), 0)])
    nnz_off = torch.cat([z, torch.cumsum(n_nnz.to(torch.int64), 0)])
    t, c = _lib.alloc_store("cuda", d, row_off, nnz_off, int(row_off[-1]), int(nnz_off[-1]))
    status.fill_(-7)
    return t, c, status


def sparse_on_device(ctrs):
    from cave_amd.sparse import SparseCones

    sc = SparseCones.from_dense(ctrs)
    return sc.cuda() if sc.nnz else None   # (no entry at all: no key array to hand to the ABI)


# ------------------------------------------------------------------------------------------------ packed stores
@pytest.mark.parametrize("waves", [1, 2, 4, 8])
@pytest.mark.parametrize("fam", "ABCD")
def test_pack_count_and_fill(gpu, fam, waves):
    lib, _lib, torch = gpu
    stream = _lib.current_stream()
    for c in cases_of(fam):
        B, m, d = c["ctrs"].shape
        x, xp = on_device(torch, c["ctrs"])
        lim = (nnz_cap(c["ctrs"]), FULL_LDS, waves)
        t, cs, status = exact_store(gpu, B, d, lambda nr, nz, st: _lib.check(lib.cave_hip_pack_count(
            _lib.ptr(xp), B, m, d, *lim, _lib.ptr(nr), _lib.ptr(nz), _lib.ptr(st), stream), "cave_hip_pack_count"))
        _lib.check(lib.cave_hip_pack_fill(_lib.ptr(xp), B, m, d, *lim, C.byref(cs), 0, _lib.ptr(status), stream), "cave_hip_pack_fill")
        assert bool((status == 0).all()), (c["name"], status)
        check_store(c, host(t), f"pack_fill w{waves}")


@pytest.mark.parametrize("fam", "ABCD")
def test_pack_fill_slot_mode(gpu, fam):
    """the slot-mode store of the split form (32 rows / 1536 non-zeros per slot): an instance beyond a slot says
    CAVE_ST_TOO_LARGE and n_rows = -1, every other slot holds the restated reduction"""
    lib, _lib, torch = gpu
    from cave_amd.qpsolver import SPLIT_NNZ, SPLIT_ROWS, _SlotStore

    for c in cases_of(fam):
        B, m, d = c["ctrs"].shape
        x, xp = on_device(torch, c["ctrs"])
        ss = _SlotStore(x.device, B, d)
        ss.pack_status.fill_(-7)
        _lib.check(lib.cave_hip_pack_fill(_lib.ptr(xp), B, m, d, nnz_cap(c["ctrs"]), FULL_LDS, 4, ss.ref, 0, _lib.ptr(ss.pack_status),
                                          _lib.current_stream()), "cave_hip_pack_fill")
        arrs, status = host(ss.t), ss.pack_status.cpu().numpy()
        for b, ref in enumerate(refs_of(c)):
            if arrs["n_rows"][b] < 0:
                assert status[b] == ST_TOO_LARGE and c["family"] != "C", (c["name"], b)
                assert ref["p"] > SPLIT_ROWS or int((ref["M"] != 0).sum()) > SPLIT_NNZ, (c["name"], b, ref["p"])
                continue
            assert status[b] == 0, (c["name"], b, status[b])
            dec = BR.decode_store(arrs, b)
            if c["family"] == "C":
                ok, why = BR.is_valid_reduction(c["ctrs"][b], dec, ref)
                assert ok and BR.no_false_pairs(c["ctrs"][b], dec), (c["name"], b, why)
            else:
                BR.record("pack_fill slots w4", BR.assert_same(dec, ref, ("slot mode", c["name"], b)))


def large_ws(gpu, B, m, d, cap):
    lib, _lib, torch = gpu
    dev = torch.device("cuda", torch.cuda.current_device())
    slice_bytes = int(lib.cave_hip_large_slice_bytes(m, d, cap, 1))
    slots = _lib.large_slots(dev, B, slice_bytes)
    return _lib.workspace(dev, slots * slice_bytes), slice_bytes, slots


@pytest.mark.parametrize("fam", "ABCD")
def test_pack_large(gpu, fam):
    lib, _lib, torch = gpu
    stream = _lib.current_stream()
    for c in cases_of(fam):
        B, m, d = c["ctrs"].shape
        x, xp = on_device(torch, c["ctrs"])
        cap = nnz_cap(c["ctrs"])
        ws, slice_bytes, slots = large_ws(gpu, B, m, d, cap)
        call = lambda nr, nz, store, st: _lib.check(lib.cave_hip_pack_large(
            _lib.ptr(xp), B, m, d, cap, _lib.ptr(ws), slice_bytes, slots, _lib.ptr(nr), _lib.ptr(nz), store, 0, _lib.ptr(st), stream),
            "cave_hip_pack_large")
        t, cs, status = exact_store(gpu, B, d, lambda nr, nz, st: call(nr, nz, None, st))
        call(None, None, C.byref(cs), status)
        assert bool((status == 0).all()), (c["name"], status)
        check_store(c, host(t), "pack_large")


@pytest.mark.parametrize("waves", [2, 4, 8])
@pytest.mark.parametrize("fam", "ABCD")
def test_pack_count_and_fill_sparse(gpu, fam, waves):
    lib, _lib, torch = gpu
    stream = _lib.current_stream()
    seen = 0
    for c in cases_of(fam):
        B, m, d = c["ctrs"].shape
        sc = sparse_on_device(c["ctrs"])
        if sc is None:
            continue
        seen += 1
        lim = (nnz_cap(c["ctrs"]), FULL_LDS, waves)
        t, cs, status = exact_store(gpu, B, d, lambda nr, nz, st: _lib.check(lib.cave_hip_pack_count_sparse(
            sc.c_ref(), *lim, _lib.ptr(nr), _lib.ptr(nz), _lib.ptr(st), stream), "cave_hip_pack_count_sparse"))
        _lib.check(lib.cave_hip_pack_fill_sparse(sc.c_ref(), *lim, C.byref(cs), 0, _lib.ptr(status), stream),
                   "cave_hip_pack_fill_sparse")
        assert bool((status == 0).all()), (c["name"], status)
        check_store(c, host(t), f"pack_fill_sparse w{waves}")
    assert seen, fam   # (only batches without a single entry are left out)


@pytest.mark.parametrize("fam", "ABCD")
def test_pack_large_sparse(gpu, fam):
    lib, _lib, torch = gpu
    stream = _lib.current_stream()
    for c in cases_of(fam):
        B, m, d = c["ctrs"].shape
        sc = sparse_on_device(c["ctrs"])
        if sc is None:
            continue
        cap = nnz_cap(c["ctrs"])
        ws, slice_bytes, slots = large_ws(gpu, B, m, d, cap)
        call = lambda nr, nz, store, st: _lib.check(lib.cave_hip_pack_large_sparse(
            sc.c_ref(), cap, _lib.ptr(ws), slice_bytes, slots, _lib.ptr(nr), _lib.ptr(nz), store, 0, _lib.ptr(st), stream),
            "cave_hip_pack_large_sparse")
        t, cs, status = exact_store(gpu, B, d, lambda nr, nz, st: call(nr, nz, None, st))
        call(None, None, C.byref(cs), status)
        assert bool((status == 0).all()), (c["name"], status)
        check_store(c, host(t), "pack_large_sparse")


# ------------------------------------------------------------------------------------------------ lite slots
def pack_only(gpu, x):
    """a pack-only launch of the step kernel (dense tensor: cave_hip_cone_step, SparseCones: cave_hip_cone_step_sparse)
    into a freshly zeroed lite store -> (host arrays, pack status)"""
    lib, _lib, torch = gpu
    from cave_amd import qpsolver as Q

    sparse = not isinstance(x, torch.Tensor)
    B, d = (len(x), x.d) if sparse else (x.shape[0], x.shape[2])
    ss = Q._LiteSlots(x.device, B, d)
    ss.pack_status.fill_(-7)
    Q._launch_step(None, None, 0, 0, 1.0, 0.0, 0, {}, None, None, x, ss)
    torch.cuda.synchronize()
    return host(ss.t), ss.pack_status.cpu().numpy()


@pytest.mark.parametrize("fam", "ABCD")
def test_pack_only_step_launches(gpu, fam):
    lib, _lib, torch = gpu
    from cave_amd.qpsolver import step_lds_bytes

    seen = 0
    for c in cases_of(fam):
        B, m, d = c["ctrs"].shape
        if m == 0 or step_lds_bytes(m, d) <= 0:   # no pack half / the shape has no fused launch
            continue
        seen += 1
        must = [lite_must_pack(r, c["ctrs"][b], m, d) for b, r in enumerate(refs_of(c))]
        arrs, status = pack_only(gpu, torch.tensor(c["ctrs"], device="cuda"))
        check_lite(c, arrs, status, "cone_step pack", must)
        sc = sparse_on_device(c["ctrs"])
        if sc is not None:
            arrs, status = pack_only(gpu, sc)
            check_lite(c, arrs, status, "cone_step_sparse pack", must)
    assert seen, fam


def lite_from_packed(gpu, ctrs):
    """exact-fit store by pack_count / pack_fill (two waves), then cave_hip_lite_from_packed -> (packed arrays, lite arrays, status)"""
    lib, _lib, torch = gpu
    from cave_amd import qpsolver as Q

    stream = _lib.current_stream()
    B, m, d = ctrs.shape
    x, xp = on_device(torch, ctrs)
    lim = (nnz_cap(ctrs), FULL_LDS, 2)
    t, cs, status = exact_store(gpu, B, d, lambda nr, nz, st: _lib.check(lib.cave_hip_pack_count(
        _lib.ptr(xp), B, m, d, *lim, _lib.ptr(nr), _lib.ptr(nz), _lib.ptr(st), stream), "cave_hip_pack_count"))
    _lib.check(lib.cave_hip_pack_fill(_lib.ptr(xp), B, m, d, *lim, C.byref(cs), 0, _lib.ptr(status), stream), "cave_hip_pack_fill")
    ls = Q._LiteSlots(x.device, B, d)
    ls.pack_status.fill_(-7)
    _lib.check(lib.cave_hip_lite_from_packed(C.byref(cs), ls.ref, _lib.ptr(ls.pack_status), stream), "cave_hip_lite_from_packed")
    torch.cuda.synchronize()
    return host(t), host(ls.t), ls.pack_status.cpu().numpy()


@pytest.mark.parametrize("fam", "ABCD")
def test_lite_from_packed(gpu, fam):
    for c in cases_of(fam):
        _, arrs, status = lite_from_packed(gpu, c["ctrs"])
        check_lite(c, arrs, status, "lite_from_packed")


# ------------------------------------------------------------------------------------------------ E: the lite limits
def test_lite_limit_cones_decode_to_the_restated_reduction(gpu):
    lib, _lib, torch = gpu
    from cave_amd.qpsolver import step_lds_bytes

    for case in BC.family_e():
        ctrs = case["ctrs"]
        d = ctrs.shape[2]
        lc = case["limit_case"]
        assert all(r["p"] == lc.p and int(r["vkind"].sum()) == lc.n_free and BR.lite_takes(r, d, LC.scratch_fits) for r in refs_of(case))
        parrs, arrs, status = lite_from_packed(gpu, ctrs)
        check_store(case, parrs, "pack_fill w2")
        check_lite(case, arrs, status, "lite_from_packed")
        if d <= 228:   # the shapes with a fused launch
            mm = LC.m_max_for_fused(ctrs, d)
            padded = dict(case, name=case["name"] + "_padded", ctrs=LC.batch(lc, 11, B=2, m_max=mm)["ctrs"])
            assert step_lds_bytes(mm, d) > 0
            for route, x in (("cone_step pack", torch.tensor(padded["ctrs"], device="cuda")),
                             ("cone_step_sparse pack", sparse_on_device(padded["ctrs"]))):
                arrs, status = pack_only(gpu, x)
                assert (status == 0).all(), (case["name"], route, status)
                check_lite(padded, arrs, status, route)


def assert_projection_is_the_oracles(torch, ctrs, seed):
    from cave_amd.qpsolver import cone_op_dense
    from oracle import cave_oracle as O

    B, m, d = ctrs.shape
    y = np.random.default_rng(seed).standard_normal((B, d)).astype(np.float32)
    o = cone_op_dense(torch.tensor(ctrs, device="cuda"), torch.tensor(y, device="cuda"), MODE_PROJECT, 1.0, 0.2,
                      outputs=("proj", "rnorm"))
    po, ro = O.batch_project(y, ctrs)
    assert bool((o["status"] == 0).all()), o["status"]
    sc = np.maximum(1.0, np.abs(y).max(axis=1))
    proj, rnorm = o["proj"].cpu().numpy(), o["rnorm"].cpu().numpy()
    assert np.all(np.abs(proj - po) <= TOL * sc[:, None]), float(np.abs(proj - po).max())
    assert np.all(np.abs(rnorm - ro) <= TOL * np.maximum(1.0, ro)), float(np.abs(rnorm - ro).max())


def test_collisions_project_as_the_oracle_does(gpu):
    for i, c in enumerate(cases_of("C")):
        assert_projection_is_the_oracles(gpu[2], c["ctrs"], 100 + i)


def test_missed_pairs_beyond_the_lite_limit(gpu):
    """tests/test_build_emul.py test_missed_pairs_beyond_the_lite_limit, on the device"""
    lib, _lib, torch = gpu
    from cave_amd.qpsolver import step_lds_bytes

    case = BC.e_missed_pairs()
    ctrs = case["ctrs"]
    B, m, d = ctrs.shape
    ref = refs_of(case)
    assert ref[1]["p"] == 5 and ref[1]["vkind"].all() and BR.lite_takes(ref[1], d, LC.scratch_fits)
    assert step_lds_bytes(m, d) > 0
    parrs, larrs, lstatus = lite_from_packed(gpu, ctrs)
    dec = BR.decode_store(parrs, 1)
    ok, why = BR.is_valid_reduction(ctrs[1], dec, ref[1])
    assert ok and BR.no_false_pairs(ctrs[1], dec), why
    assert dec["p"] == 10 and not dec["vkind"].any()       # the measured deviation: every pair missed
    BR.assert_same(BR.decode_store(parrs, 0), ref[0], "the neighbour")
    for name, (arrs, status) in {
        "cone_step pack": pack_only(gpu, torch.tensor(ctrs, device="cuda")),
        "cone_step_sparse pack": pack_only(gpu, sparse_on_device(ctrs)),
        "lite_from_packed": (larrs, lstatus),
    }.items():
        assert status.tolist() == [0, ST_TOO_LARGE], (name, status)
        assert BR.decode_lite(arrs, 1, d)["state"] == -1, name
        BR.assert_same(BR.decode_lite(arrs, 0, d), ref[0], name)
    assert_projection_is_the_oracles(torch, ctrs, 7)
