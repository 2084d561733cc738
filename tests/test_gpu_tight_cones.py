"""GPU tier: the tight-cone kernels (cave_amd/csrc/tight_cones.h, k_tight_cones.hip) through the C ABI
(cave_hip_tight_cones_count / cave_hip_tight_cones_fill) and through the Python layer (tight.tight_cones_hip,
TSPConeDataset(device=), VRPConeDataset(device=, cones="sparse"), the example's --device-cones).

The cases and the oracle are those of the CPU tier (tests/tight_cones_cases.py): host code only, exact comparisons."""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import tight_cones_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_system(s):
    from cave_amd import _lib

    if s is None:
        return None
    return _lib.LinSystemC(R=s.R, Z=s.Z, d=s.d, reserved=0, **{k: (getattr(s, k).data_ptr() if getattr(s, k) is not None else None)
                                                                 for k in ("row_off", "col", "coef", "sense", "rhs")})


def _run(case, slack=0):
    """both passes of a case through the C ABI on device tensors -> (rc, outputs as TC.check takes them)"""
    import torch

    from cave_amd import _lib

    lib = _lib.load()
    p, ref = _lib.ptr, lambda c: None if c is None else C.byref(c)

    def count(s, lz, off, sol, N, tol, n_rows, n_ent, st):
        return lib.cave_hip_tight_cones_count(ref(_c_system(s)), ref(_c_system(lz)), p(off), p(sol), N, tol, p(n_rows), p(n_ent), p(st),
                                              _lib.current_stream())

    def fill(s, lz, off, sol, N, tol, ent_off, cap, key, val, st):
        return lib.cave_hip_tight_cones_fill(ref(_c_system(s)), ref(_c_system(lz)), p(off), p(sol), N, tol, p(ent_off), cap, p(key),
                                             p(val), p(st), _lib.current_stream())

    return TC.two_passes(case, count, fill, lambda a: torch.from_numpy(a).cuda(), lambda t: t.cpu().numpy(), slack=slack)


def _lin(s):
    """the LinSystem of a well-formed RawSys"""
    from cave_amd import tight

    return tight.LinSystem(sp.csr_matrix((s.coef, s.col, s.row_off), shape=(s.R, s.d)), s.sense, s.rhs)


def _hip(case):
    import torch

    from cave_amd import tight

    lazy = None if case.lazy is None else (_lin(case.lazy), case.lazy_off)
    return tight.tight_cones_hip(_lin(case.sys), torch.from_numpy(case.sol).cuda(), lazy, case.tol)


def _same(a, e, what=None):
    assert a.m_max == e.m_max and a.d == e.d and a.B == e.B, what
    for k in ("ent_off", "key", "val"):
        assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(e, k).cpu().numpy()), (what, k)


@pytest.mark.parametrize("case", TC.good_cases(), ids=lambda c: c.name)
def test_cones_equal_the_host(case):
    rc, o = _run(case)
    TC.check(case, rc, o)
    rc2, o2 = _run(case)  # two launches of the same batch give identical bytes
    assert rc2 == 0 and all(np.array_equal(o[k].view(np.uint8), o2[k].view(np.uint8)) for k in o)
    cones = _hip(case)
    assert cones.is_cuda
    _same(cones, case.expect, case.name)


@pytest.mark.parametrize("case", TC.bad_cases(), ids=lambda c: c.name)
def test_a_failed_instance_counts_nothing_and_writes_nothing(case):
    rc, o = _run(case, slack=16)
    TC.check(case, rc, o)
    N = len(case.sol)
    assert (o["n_rows"][:N][case.status != 0] == 0).all() and (o["n_ent"][:N][case.status != 0] == 0).all()
    if case.name in ("nan_sol", "too_large"):  # (the Python layer canonicalises a system: the other two cannot reach it)
        first = int(np.flatnonzero(case.status)[0])
        with pytest.raises(ValueError, match=f"instance {first} "):
            _hip(case)


def test_invalid_arguments_and_an_empty_batch():
    import torch

    from cave_amd import _lib, tight

    lib = _lib.load()
    case = TC.d1_case()
    s = case.sys._replace(**{k: torch.from_numpy(getattr(case.sys, k)).cuda() for k in ("row_off", "col", "coef", "sense", "rhs")})
    sol = torch.from_numpy(case.sol).cuda()
    n_rows, n_ent = torch.full((3,), -7, dtype=torch.int32, device="cuda"), torch.full((3,), -7, dtype=torch.int64, device="cuda")
    p = _lib.ptr

    def count(sys=s, sol=sol, N=3, tol=1e-5, n_rows=n_rows):
        c = _c_system(sys)
        return lib.cave_hip_tight_cones_count(C.byref(c), None, None, p(sol), N, tol, p(n_rows), p(n_ent), None, _lib.current_stream())

    for kw in (dict(sol=None), dict(n_rows=None), dict(sys=s._replace(d=0)), dict(sys=s._replace(d=65536)), dict(N=-1), dict(tol=-1.0),
               dict(tol=float("nan")), dict(sys=s._replace(rhs=None)), dict(sys=s._replace(col=None))):
        assert count(**kw) == TC.E_INVALID, kw
        assert b"tight_cones_count" in lib.cave_hip_last_error()
    torch.cuda.synchronize()
    assert bool((n_rows == -7).all()) and bool((n_ent == -7).all())
    assert count(N=0, sol=None, n_rows=None) == 0
    empty = tight.tight_cones_hip(_lin(case.sys), sol[:0])
    assert empty.B == 0 and empty.nnz == 0 and empty.m_max == 0
    with pytest.raises(ValueError, match="columns"):
        tight.tight_cones_hip(tight.tsp_system(5), sol)
    with pytest.raises(ValueError, match="float32"):
        tight.tight_cones_hip(_lin(case.sys), sol.cpu())
    with pytest.raises(ValueError, match="tol"):
        tight.tight_cones_hip(_lin(case.sys), sol, tol=-1.0)


@pytest.mark.parametrize("shape", [(3, 3), (5, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shortest_path_cones_are_those_of_the_solve_kernel(shape):
    import torch

    from cave_amd import tight

    h, w = shape
    costs = torch.from_numpy(tight.sp_gen_data(4, 5, h, w, seed=135)[1]).cuda()
    cones, sols, _ = tight.sp_cones_hip(costs, h, w)
    mine = tight.tight_cones_hip(tight.sp_system(h, w), sols)
    _same(mine, cones, shape)
    _same(mine, TC.sp_case(h, w).expect, shape)


def _items_equal(ds, ctrs):
    from cave_amd.sparse import SparseCones

    for i, a in enumerate(ctrs):
        x, c, s, z, cone = ds[i]
        e = SparseCones.from_ragged([a], m_max=ds.cones.m_max)
        assert cone.is_cuda and cone.B == 1 and x.is_cuda and c.is_cuda and s.is_cuda and z.is_cuda
        _same(cone, e, i)
        assert cone.key.data_ptr() == ds.cones.key.data_ptr() + 4 * int(ds.cones.ent_off[i])  # a view, no copy


@pytest.fixture(scope="module")
def tsp_sets():
    from cave_amd import tight

    feats, costs, _, _ = TC.tsp_data(8)
    return tight.TSPConeDataset(feats, costs, 8), tight.TSPConeDataset(feats, costs, 8, device="cuda")


def test_tsp_dataset_on_the_device(tsp_sets):
    import torch

    from cave_amd.sparse import SparseCones

    host, dev = tsp_sets
    assert not hasattr(dev, "ctrs") and len(dev) == len(host) == 12 and dev.tight_cuts == host.tight_cuts
    _same(dev.cones, SparseCones.from_ragged(host.ctrs))
    _items_equal(dev, host.ctrs)
    for k in ("feats", "costs", "sols", "objs"):
        assert torch.equal(getattr(dev, k).cpu(), getattr(host, k)), k


def test_vrp_dataset_on_the_device():
    import torch

    from cave_amd import tight
    from cave_amd.sparse import SparseCones

    feats, costs, demands, capacity, _, _ = TC.vrp_data()
    host = tight.VRPConeDataset(feats, costs, TC.VRP_N, demands, capacity, TC.VRP_K)
    default = tight.VRPConeDataset(feats, costs, TC.VRP_N, demands, capacity, TC.VRP_K, device="cuda")
    assert default.cones is None and all(torch.equal(a, b) for a, b in zip(default.ctrs, host.ctrs))  # the default: the dense list
    dev = tight.VRPConeDataset(feats, costs, TC.VRP_N, demands, capacity, TC.VRP_K, device="cuda", cones="sparse")
    assert not hasattr(dev, "ctrs") and dev.tight_cuts == host.tight_cuts
    _same(dev.cones, SparseCones.from_ragged(host.ctrs))
    _items_equal(dev, host.ctrs)
    assert torch.equal(dev.sols.cpu(), host.sols) and torch.equal(dev.objs.cpu(), host.objs)
    with pytest.raises(ValueError, match="device"):
        tight.VRPConeDataset(feats, costs, TC.VRP_N, demands, capacity, TC.VRP_K, cones="sparse")


def test_a_store_from_device_cones_steps_like_the_host_built_dense_batch(tsp_sets):
    import torch

    from cave_amd.cave import EPO, innerConeAlignedCosine
    from cave_amd.dataset import ConeStore, PackedBatch

    host, dev = tsp_sets

    class _Model:
        modelSense = EPO.MINIMIZE

    out = []
    for store in (ConeStore.from_ragged(host.ctrs), ConeStore.from_sparse(dev.cones)):
        mod = innerConeAlignedCosine(_Model(), solver="hip", seed=0)
        pred = (host.costs * 1.25 + 0.5).cuda().requires_grad_(True)
        loss = mod(pred, PackedBatch(store, torch.arange(len(host))))
        loss.backward()
        out.append((loss.detach().clone(), pred.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert bool(torch.isfinite(out[0][1]).all()) and float(out[0][1].abs().max()) > 0


def test_integration_doc_stub_for_the_reference_side():
    """its fenced stub is executed as written on a small scipy.sparse system standing in for getA()"""
    import torch

    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 16. "):]
    blocks = re.findall(r"^```py\n(.*?)^```", sec, flags=re.S | re.M)
    assert len(blocks) == 1, "INTEGRATION.md §16 must hold one python stub"
    ns = {}
    exec(compile(blocks[0], "INTEGRATION.md", "exec"), ns)  # noqa: S102 - the document is the test subject
    sys_, lazy, off, sol = TC.synth_parts()
    A = sp.csr_matrix((sys_.coef, sys_.col, sys_.row_off), shape=(sys_.R, sys_.d))
    L = TC.dense(lazy)
    chars = np.array(["<", ">", "="])
    parsed = [[(L[i], float(lazy.rhs[i]), str(chars[lazy.sense[i]])) for i in range(off[b], off[b + 1])] for b in range(len(sol))]
    cones = ns["extract_tight_cones"](A, chars[sys_.sense], sys_.rhs, parsed, sol)
    assert cones.is_cuda
    _same(cones, TC.synth_case().expect)
    assert isinstance(cones.key, torch.Tensor)


def test_example_with_device_cones(capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_sp_cave

    hist = train_sp_cave.main(["--problem", "tsp", "--nodes", "8", "--num-data", "12", "--epochs", "2", "--sparse", "--device-cones"])
    printed = capsys.readouterr().out
    assert len(hist) == 3 and all(np.isfinite(r) for _, _, r in hist) and re.search(r"epoch 2: loss \S+\s+regret \S+%", printed)
    host = train_sp_cave.main(["--problem", "tsp", "--nodes", "8", "--num-data", "12", "--epochs", "2", "--sparse"])
    assert [(e, l, r) for e, l, r in hist[1:]] == [(e, l, r) for e, l, r in host[1:]]  # the same cones: the same run
