"""GPU tier: the grid shortest-path kernel (cave_amd/csrc/sp_grid.h, k_sp_grid.hip) through the C ABI
(cave_hip_sp_grid_solve) and through the Python layer (tight.sp_solve_hip, sp_cones_hip, sp_regret(device=),
SPConeDataset(device=), examples/train_sp_cave.py --device-data).

Oracle: the project's host code (tight.sp_solve, tight.sp_tight_normals, SparseCones.from_ragged); cases and bounds are
those of the CPU tier (tests/sp_grid_cases.py):
  1. sols and objs equal the host's exactly           2. evals within (h + w) 2^-52 sum |c_k| sol_k of the fp64 product
  3. sp_regret(device=) within (h + w) 2^-23 sum_i sum_k |c_ik| sol_ik / sum_i |z_i| of the host's (the rounding of the
     host's float32 c @ s)                             4. cones equal SparseCones.from_ragged(...) as tensors
  5. ConeStore.from_sparse(device cones) and ConeStore.from_ragged(host ctrs): the same bits in MODE_INNER
  6. a non-finite cost fails its instance alone        7. two launches: the same bits
  8. / 9. the training example with --device-data."""

import os
import sys

import numpy as np
import pytest

import sp_grid_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SOL, F_OBJ, F_EVAL, F_STATUS, F_CONES = 2, 4, 8, 16, 32
F_ALL = 62


@pytest.fixture(scope="module")
def lib():
    from cave_amd import _lib

    return _lib.load()


def abi_solve(lib, costs, h, w, eval_costs=None, flags=F_ALL):
    """cave_hip_sp_grid_solve on numpy inputs -> (rc, dict of numpy outputs; None where `flags` gives no buffer)"""
    import torch

    from cave_amd import _lib

    N, d = costs.shape[0], SC.n_arcs(h, w)
    c = torch.tensor(costs, device="cuda")
    ev = None if eval_costs is None else torch.tensor(eval_costs, device="cuda")
    t = {"sol": torch.full((N, d), 77.0, device="cuda") if flags & F_SOL else None,
         "obj": torch.full((N,), 77.0, dtype=torch.float64, device="cuda") if flags & F_OBJ else None,
         "eval": torch.full((N,), 77.0, dtype=torch.float64, device="cuda") if flags & F_EVAL else None,
         "status": torch.full((N,), -7, dtype=torch.int32, device="cuda") if flags & F_STATUS else None,
         "key": torch.full((N * 5 * d,), -7, dtype=torch.int32, device="cuda") if flags & F_CONES else None,
         "val": torch.full((N * 5 * d,), 77.0, device="cuda") if flags & F_CONES else None}
    rc = lib.cave_hip_sp_grid_solve(_lib.ptr(c), _lib.ptr(ev), N, h, w, _lib.ptr(t["sol"]), _lib.ptr(t["obj"]), _lib.ptr(t["eval"]),
                                    _lib.ptr(t["status"]), _lib.ptr(t["key"]), _lib.ptr(t["val"]), _lib.current_stream())
    torch.cuda.synchronize()
    return int(rc), {k: None if v is None else v.cpu().numpy() for k, v in t.items()}


def test_lds_query_and_rejected_shapes(lib):
    for (h, w) in list(SC.SHAPES) + [(1, 1), (128, 128), (134, 134), (135, 135), (0, 5)]:
        assert lib.cave_hip_sp_grid_lds_bytes(h, w) == SC.lds_bytes(h, w), (h, w)
    at, above = SC.lds_limit_shapes()
    assert lib.cave_hip_sp_grid_lds_bytes(*at) > 0 and lib.cave_hip_sp_grid_lds_bytes(*above) == SC.E_INVALID
    assert abi_solve(lib, np.ones((1, 0), np.float32), 1, 1)[0] == SC.E_INVALID
    assert abi_solve(lib, np.ones((1, SC.n_arcs(*above)), np.float32), *above, flags=F_SOL)[0] == SC.E_INVALID
    assert abi_solve(lib, np.ones((1, 1), np.float32), 1, 2, flags=F_EVAL)[0] == SC.E_INVALID
    assert abi_solve(lib, np.zeros((0, 1), np.float32), 1, 2, flags=F_SOL)[0] == 0
    c = np.ones((1, SC.n_arcs(128, 129)), np.float32)
    assert abi_solve(lib, c, 128, 129, flags=F_CONES)[0] == SC.E_INVALID
    assert abi_solve(lib, c, 128, 129, flags=F_SOL)[0] == 0


@pytest.mark.parametrize("shape", list(SC.SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", SC.KINDS)
def test_abi_solve_eval_and_cones_equal_the_host(lib, kind, shape):
    h, w = shape
    costs, sols, objs = SC.host(kind, h, w)
    ev = SC.costs_of("signed", len(costs), h, w, seed=3)
    rc, o = abi_solve(lib, costs, h, w, eval_costs=ev)
    assert rc == 0
    SC.check_solve(o, costs, sols, objs, h, w, eval_costs=ev, what=(kind, shape))
    SC.check_cones(o["key"], o["val"], SC.host_cones(kind, h, w), len(costs), h, w, what=(kind, shape))
    rc, o2 = abi_solve(lib, costs, h, w, eval_costs=ev)   # condition 7
    assert rc == 0
    for k in o:
        assert np.array_equal(o[k].view(np.uint8), o2[k].view(np.uint8)), (kind, shape, k)


def test_limit_shapes(lib):
    from cave_amd.sparse import SparseCones

    (h, w), _ = SC.lds_limit_shapes()
    costs, sols, objs = SC.host("ties", h, w, N=2)
    rc, o = abi_solve(lib, costs, h, w, eval_costs=costs, flags=F_ALL & ~F_CONES)
    assert rc == 0
    SC.check_solve(o, costs, sols, objs, h, w, eval_costs=costs, what="lds limit")
    assert abi_solve(lib, costs, h, w, eval_costs=costs)[0] == SC.E_INVALID   # its cone is beyond the key's 16 bits
    h = w = 128
    costs, sols, objs = SC.host("gen", h, w, N=1)
    rc, o = abi_solve(lib, costs, h, w, flags=F_ALL & ~F_EVAL)
    assert rc == 0
    SC.check_solve(o, costs, sols, objs, h, w, what="cone limit")
    SC.check_cones(o["key"], o["val"], SparseCones.from_coo([SC.cone_coo(sols[0], h, w)], SC.n_arcs(h, w)), 1, h, w, what="cone limit")


def test_batch_variants(lib):
    h, w = 5, 5
    for N in (1, 1000):   # 1000: 250 workgroups
        costs, sols, objs = SC.host("gen", h, w, N=N)
        rc, o = abi_solve(lib, costs, h, w, eval_costs=costs, flags=F_ALL & ~F_CONES)
        assert rc == 0
        SC.check_solve(o, costs, sols, objs, h, w, eval_costs=costs, what=N)
    costs, sols, objs = SC.host("ties", h, w)
    ref = SC.host_cones("ties", h, w)
    for drop in (F_SOL, F_OBJ, F_EVAL, F_STATUS, F_CONES):   # each output pointer null in turn, eval_costs present and absent
        for ev in (costs, None):
            rc, o = abi_solve(lib, costs, h, w, eval_costs=ev, flags=F_ALL & ~drop & ~(0 if ev is not None else F_EVAL))
            assert rc == 0
            SC.check_solve(o, costs, sols, objs, h, w, eval_costs=ev, what=(drop, ev is None))
            if o["key"] is not None:
                SC.check_cones(o["key"], o["val"], ref, len(costs), h, w)


@pytest.mark.parametrize("poison", [np.nan, np.inf])
@pytest.mark.parametrize("shape", [(5, 5), (3, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_non_finite_cost_fails_its_instance_alone(lib, shape, poison):
    import torch

    from cave_amd import tight

    h, w = shape
    costs, sols, objs = SC.host("gen", h, w)
    d = SC.n_arcs(h, w)
    bad = costs.copy()
    bad[9, d // 2] = poison
    rc, o = abi_solve(lib, bad, h, w, eval_costs=costs)
    assert rc == 0
    ok = np.arange(len(costs)) != 9
    assert o["status"][9] == SC.ST_BAD_INPUT and (o["status"][ok] == SC.ST_OK).all()
    assert (o["sol"][9] == 0).all() and np.isnan(o["obj"][9]) and np.isnan(o["eval"][9])
    assert np.array_equal(o["sol"][ok], sols[ok]) and np.array_equal(o["obj"][ok], objs[ok])
    ref = SC.host_cones("gen", h, w)
    key, rk = o["key"].reshape(len(costs), -1), ref.key.numpy().reshape(len(costs), -1)
    assert np.array_equal(key[ok], rk[ok])
    with pytest.raises(ValueError, match="instance 9"):   # the Python layer refuses the batch
        tight.sp_solve_hip(torch.tensor(bad, device="cuda"), h, w)


@pytest.mark.parametrize("shape", [(5, 5), (30, 30), (3, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_python_layer(shape):
    import torch

    from cave_amd import tight

    h, w = shape
    costs, sols, objs = SC.host("gen", h, w)
    ev = SC.costs_of("signed", len(costs), h, w, seed=3)
    c, e = torch.tensor(costs, device="cuda"), torch.tensor(ev, device="cuda")
    s, z = tight.sp_solve_hip(c, h, w)
    s2, z2, v = tight.sp_solve_hip(c, h, w, eval_costs=e)
    assert s.dtype == torch.float32 and z.dtype == torch.float64 and torch.equal(s, s2) and torch.equal(z, z2)
    SC.check_solve({"sol": s.cpu().numpy(), "obj": z.cpu().numpy(), "eval": v.cpu().numpy()}, costs, sols, objs, h, w, eval_costs=ev)
    cones, s3, z3 = tight.sp_cones_hip(c, h, w)
    ref = SC.host_cones("gen", h, w)
    assert cones.is_cuda and torch.equal(s3, s) and torch.equal(z3, z)
    assert cones.m_max == ref.m_max and cones.d == ref.d and cones.B == ref.B   # condition 4
    for k in ("ent_off", "key", "val"):
        assert torch.equal(getattr(cones, k).cpu(), getattr(ref, k)), k
    with pytest.raises(ValueError):
        tight.sp_solve_hip(c.cpu(), h, w)
    with pytest.raises(ValueError):
        tight.sp_solve_hip(c[:, :-1], h, w)


@pytest.mark.parametrize("shape,kind", [((5, 5), "gen"), ((12, 12), "signed"), ((30, 30), "gen"), ((3, 70), "spread")],
                         ids=lambda s: str(s))
def test_device_regret_matches_the_host(shape, kind):
    """condition 3"""
    import torch

    from cave_amd import tight

    h, w = shape
    true, tsols, z = SC.host("gen" if kind != "signed" else "signed", h, w)
    pred = SC.costs_of(kind, len(true), h, w, seed=5)
    z32 = z.astype(np.float32)
    host = tight.sp_regret(pred, true, z32, h, w)
    psols = np.stack([tight.sp_solve(p, h, w)[0] for p in pred])
    bound = (h + w) * 2.0 ** -23 * (np.abs(true.astype(np.float64)) * psols).sum() / np.abs(z32.astype(np.float64)).sum()
    dev = tight.sp_regret(pred, true, z32, h, w, device="cuda")
    print(f"regret {shape} {kind}: host {host!r} device {dev!r} |diff| {abs(dev - host):.3e} bound {bound:.3e}")
    assert abs(dev - host) <= bound
    on_dev = tight.sp_regret(torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda"), torch.tensor(z32, device="cuda"),
                             h, w, device="cuda")
    assert on_dev == dev


@pytest.mark.parametrize("shape", [(5, 5), (12, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_store_from_device_cones_equals_store_from_host_ctrs(shape):
    """condition 5, and the dataset with a device: no dense list, sparse slices, collate_sparse"""
    import torch

    from cave_amd import _lib, tight
    from cave_amd.dataset import ConeStore
    from cave_amd.sparse import SparseCones, collate_sparse

    h, w = shape
    feats, costs = tight.sp_gen_data(48, 5, h, w, seed=135)
    hd = tight.SPConeDataset(feats, costs, h, w)
    dd = tight.SPConeDataset(feats, costs, h, w, device="cuda")
    assert not hasattr(dd, "ctrs") and isinstance(dd.cones, SparseCones) and dd.cones.is_cuda and len(dd) == len(hd)
    assert torch.equal(dd.sols.cpu(), hd.sols) and torch.equal(dd.objs.cpu(), hd.objs) and torch.equal(dd.costs.cpu(), hd.costs)
    ref = SparseCones.from_ragged(hd.ctrs)
    batch = collate_sparse([dd[i] for i in (3, 0, 47)])
    want = ref[[3, 0, 47]]
    assert torch.equal(batch[0].cpu(), hd.feats[[3, 0, 47]]) and batch[-1].is_cuda
    for k in ("ent_off", "key", "val"):
        assert torch.equal(getattr(batch[-1], k).cpu(), getattr(want, k)), k
    a, b = ConeStore.from_ragged(hd.ctrs), ConeStore.from_sparse(dd.cones)
    ids = torch.arange(len(hd), device="cuda")
    pred = torch.tensor(SC.costs_of("gen", len(hd), h, w, seed=9), device="cuda")
    oa = a.cone_op(ids, pred, _lib.MODE_INNER, -1.0, 0.2, outputs=("proj", "rnorm", "loss", "grad"))
    ob = b.cone_op(ids, pred, _lib.MODE_INNER, -1.0, 0.2, outputs=("proj", "rnorm", "loss", "grad"))
    assert bool((oa["status"] == 0).all())
    for k in ("proj", "rnorm", "loss", "grad"):
        assert torch.equal(oa[k], ob[k]), k


def _example(argv):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_sp_cave

    return train_sp_cave.main(argv)


def test_training_example_device_data_matches_host_data():
    """condition 8: the same losses; regrets within condition 3's bound -- sp_gen_data costs are positive, so
    sum_i c_i . w(c_hat_i) / sum_i z_i = 1 + regret"""
    base = ["--grid", "5", "5", "--num-data", "64", "--batch", "32", "--epochs", "3", "--packed"]
    host, dev = _example(base), _example(base + ["--device-data"])
    assert len(host) == len(dev) == 4
    for (e0, l0, r0), (e1, l1, r1) in zip(host, dev):
        print(f"epoch {e0}: loss {l0!r} / {l1!r}  regret {r0!r} / {r1!r}")
        assert e0 == e1 and (l0 == l1 or e0 == 0)
        assert abs(r0 - r1) <= 10 * 2.0 ** -23 * (1.0 + r0), (e0, r0, r1)
    sparse = _example(base[:-1] + ["--device-data", "--sparse", "--prefetch"])   # the other routes the flag combines with
    assert len(sparse) == 4 and all(np.isfinite(x[2]) for x in sparse)


def test_training_example_30x30_on_device_data():
    """condition 9"""
    hist = _example(["--grid", "30", "30", "--num-data", "64", "--device-data", "--packed", "--inner", "ipm", "--epochs", "2"])
    assert len(hist) == 3 and all(np.isfinite(x[2]) for x in hist) and all(np.isfinite(x[1]) for x in hist[1:])
