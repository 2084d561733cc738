"""GPU tier: the CVRP dynamic-program kernels (cave_amd/csrc/vrp_dp.h, k_vrp_dp.hip) through the C ABI
(cave_hip_vrp_dp_solve, bound by the ctypes stub of INTEGRATION.md section 13 as printed) and through the Python layer
(tight.vrp_solve_hip, vrp_regret(device=), VRPConeDataset(device=), examples/train_sp_cave.py --problem vrp).

Oracle: tight.vrp_solve; cases and bounds are those of the CPU tier (tests/vrp_dp_cases.py):
  1. objs, routes and sols equal the host's bit for bit, ties, negative costs and loads equal to the capacity included
  2. evals equal the fp64 sum of the routes' edges under eval_costs in route order, bit for bit
  3. a non-finite cost fails its instance alone, a bad demand every instance; infeasible instances report
     CAVE_ST_INFEASIBLE                                 4. absent outputs leave the others unchanged; nothing is written
     beyond an output                                   5. rejected arguments (outputs untouched), size queries
  6. two launches, a two-slot and the default workspace, another batch order: the same bytes per instance
  7. vrp_regret(device=) within (n + K) 2^-23 sum_i sum_k |c_ik| sol_ik / sum_i |z_i| of the host's (the rounding of the
     host's float32 c @ s)                              8. the training example with --problem vrp --device-regret
  9. CVRP cones through exactConeAlignedCosine(solver='hip') against the CPU oracle at the tolerances of
     tests/golden_cases.py (loss 2e-6 absolute, gradient 8e-6 max(1, |grad|_inf))."""

import itertools
import os
import re
import sys

import numpy as np
import pytest

import vrp_dp_cases as VC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SOL, F_OBJ, F_EVAL, F_ROUTES, F_STATUS = 2, 4, 8, 16, 32
F_ALL = 62
EACH = (("sol", F_SOL), ("obj", F_OBJ), ("eval", F_EVAL), ("routes", F_ROUTES), ("status", F_STATUS))
GUARD = 8


@pytest.fixture(scope="module")
def stub():
    """a fresh handle of the library bound by INTEGRATION.md section 13's stub, and the stub's functions"""
    import ctypes as C

    from cave_amd import _lib

    _lib.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 13. CVRP on the device"):]
    ns = {}
    exec(re.search(r"^```py\n(.*?)^```", sec, flags=re.S | re.M).group(1), ns)
    lib = C.CDLL(_lib.LIB_PATH)
    lib.cave_hip_last_error.restype = C.c_char_p
    ns["bind_vrp_dp"](lib)
    norm = lambda t: re.sub(r"\s+", " ", t).strip()
    hdr = norm(open(os.path.join(ROOT, "include", "cave_hip.h")).read())
    protos = re.findall(r"int\d\d_t cave_hip_\w+\([^;]*\);", re.search(r"^```c\n(.*?)^```", sec, flags=re.S | re.M).group(1))
    assert len(protos) == 3 and all(norm(p) in hdr for p in protos)
    assert "#define CAVE_ST_INFEASIBLE 4" in hdr and "#define CAVE_HIP_ABI_VERSION 10" in hdr
    return lib, ns


def abi_solve(stub, costs, n, demands, capacity, K, eval_costs=None, flags=F_ALL, workspace_bytes=None, null=()):
    """cave_hip_vrp_dp_solve on numpy inputs -> (rc, dict of numpy outputs; None where `flags` gives no buffer).  Outputs
    are sentinel-filled with GUARD extra elements, which are checked and cut off; a rejected call must leave them as they
    were.  `workspace_bytes`: None = the size query's default.  `null`: inputs handed over as null pointers."""
    import torch

    from cave_amd import _lib

    lib, ns = stub
    N, d = costs.shape[0], VC.n_edges(n)
    c = torch.tensor(np.ascontiguousarray(costs), device="cuda")
    ev = None if eval_costs is None else torch.tensor(np.ascontiguousarray(eval_costs), device="cuda")
    q = torch.tensor(np.ascontiguousarray(demands, dtype=np.float32), device="cuda")
    size = {"sol": N * d, "obj": N, "eval": N, "routes": N * (n + K), "status": N}
    fill = {"sol": (77.0, torch.float32), "obj": (77.0, torch.float64), "eval": (77.0, torch.float64), "routes": (-7, torch.int32),
            "status": (-7, torch.int32)}
    t = {k: torch.full((max(size[k], 0) + GUARD,), fill[k][0], dtype=fill[k][1], device="cuda") if flags & f else None for k, f in EACH}
    if workspace_bytes is None:
        workspace_bytes = max(int(lib.cave_hip_vrp_dp_workspace_bytes(n, K, N)), 0)
    ws = torch.full((workspace_bytes // 8,), -1, dtype=torch.int64, device="cuda") if workspace_bytes >= 8 else None
    rc = lib.cave_hip_vrp_dp_solve(_lib.ptr(None if "costs" in null else c), _lib.ptr(ev), _lib.ptr(None if "demands" in null else q),
                                   float(capacity), K, N, n, _lib.ptr(t["sol"]), _lib.ptr(t["obj"]), _lib.ptr(t["eval"]),
                                   _lib.ptr(t["routes"]), _lib.ptr(t["status"]), _lib.ptr(ws), workspace_bytes if ws is not None else 0,
                                   _lib.current_stream())
    torch.cuda.synchronize()
    o = {}
    shape = {"sol": (N, d), "obj": (N,), "eval": (N,), "routes": (N, n + K), "status": (N,)}
    for k, v in t.items():
        if v is None:
            o[k] = None
            continue
        a = v.cpu().numpy()
        assert (a[max(size[k], 0):] == fill[k][0]).all(), (k, "written beyond its end")
        if rc != 0:
            assert (a == fill[k][0]).all(), (k, "written by a rejected call")
            o[k] = a
        else:
            o[k] = a[:size[k]].reshape(shape[k])
    return int(rc), o


def test_size_queries_and_rejected_arguments(stub):
    lib, _ = stub
    for n in range(0, 17):
        for K in range(0, 10):
            assert lib.cave_hip_vrp_dp_slot_bytes(n, K) == VC.slot_bytes(n, K), (n, K)
            for N in (0, 1, 5, 512, 513, 100000, -1):
                assert lib.cave_hip_vrp_dp_workspace_bytes(n, K, N) == VC.workspace_bytes(n, K, N), (n, K, N)
    c, q, cap = VC.host("gen", 5, 2)[:3]
    for n, K in ((2, 1), (15, 1), (5, 0), (5, 9)):
        assert abi_solve(stub, np.ones((1, VC.n_edges(max(n, 2))), np.float32), n, np.ones(max(n - 1, 1)), 10.0, K, flags=F_SOL,
                         workspace_bytes=0)[0] == VC.E_INVALID
    assert b"3 <= n <= 14" in lib.cave_hip_last_error()
    assert abi_solve(stub, c, 5, q, cap, 2, flags=F_EVAL)[0] == VC.E_INVALID                       # eval without eval_costs
    for bad_cap in (0.0, -1.0, np.inf, np.nan):
        assert abi_solve(stub, c, 5, q, bad_cap, 2, eval_costs=c)[0] == VC.E_INVALID, bad_cap
    assert b"capacity" in lib.cave_hip_last_error()
    assert abi_solve(stub, c, 5, q, cap, 2, eval_costs=c, null=("demands",))[0] == VC.E_INVALID
    assert abi_solve(stub, c, 5, q, cap, 2, eval_costs=c, null=("costs",))[0] == VC.E_INVALID
    assert abi_solve(stub, np.zeros((0, 10), np.float32), 5, q, cap, 2, flags=F_SOL)[0] == 0       # N == 0
    assert abi_solve(stub, np.zeros((0, VC.n_edges(13)), np.float32), 13, np.ones(12), 9.0, 3, flags=F_SOL, workspace_bytes=0)[0] == 0
    for n, K in ((VC.WS_MIN_N, 3), (13, 6)):                                                       # a slot is needed
        c, q, cap = VC.host("ties", n, K)[:3]
        for wsb in (0, 8, VC.slot_bytes(n, K) - 8):
            assert abi_solve(stub, c, n, q, cap, K, eval_costs=c, workspace_bytes=wsb)[0] == VC.E_INVALID, (n, K, wsb)
    c, q, cap = VC.host("ties", VC.LDS_MAX_N, 3)[:3]
    assert abi_solve(stub, c, VC.LDS_MAX_N, q, cap, 3, flags=F_SOL, workspace_bytes=0)[0] == 0     # tier 0 needs none


@pytest.mark.parametrize("shape", list(VC.SHAPES), ids=lambda s: f"n{s[0]}-K{s[1]}")
@pytest.mark.parametrize("kind", VC.KINDS)
def test_abi_routes_objectives_and_evals_equal_the_host(stub, kind, shape):
    n, K = shape
    costs, q, cap, sols, objs, routes = VC.host(kind, n, K)
    ev = VC.instance_of("signed", len(costs), n, K, seed=3)[0]
    rc, o = abi_solve(stub, costs, n, q, cap, K, eval_costs=ev)
    assert rc == 0
    VC.check_solve(o, sols, objs, routes, n, eval_costs=ev, what=(kind, n, K))
    rc, o2 = abi_solve(stub, costs, n, q, cap, K, eval_costs=ev)   # two launches: the same bytes
    assert rc == 0
    for k in o:
        assert np.array_equal(VC.bits(o[k]), VC.bits(o2[k])), (kind, n, K, k)
    perm = np.roll(np.arange(len(costs)), 1)[::-1].copy()   # the same instances in another batch order
    rc, o3 = abi_solve(stub, costs[perm], n, q, cap, K, eval_costs=ev[perm])
    assert rc == 0
    for k in o:
        assert np.array_equal(VC.bits(o3[k]), VC.bits(o[k][perm])), (kind, n, K, k, "batch order")


@pytest.mark.parametrize("shape", [(VC.WS_MIN_N, 3), (13, 6)], ids=["tier1", "tier2"])
def test_two_slots_five_instances_and_a_batch_of_one(stub, shape):
    """slot reuse and a tail: workgroup 0 takes instances 0, 2, 4 and workgroup 1 instances 1, 3; the default workspace
    (five slots) gives the same bytes; N = 1 in every tier"""
    n, K = shape
    costs, q, cap, sols, objs, routes = VC.host("ties", n, K, N=5, seed=1)
    rc, o = abi_solve(stub, costs, n, q, cap, K, eval_costs=costs, workspace_bytes=2 * VC.slot_bytes(n, K))
    assert rc == 0
    VC.check_solve(o, sols, objs, routes, n, eval_costs=costs, what="two slots")
    rc, od = abi_solve(stub, costs, n, q, cap, K, eval_costs=costs)
    assert rc == 0
    for k in o:
        assert np.array_equal(VC.bits(o[k]), VC.bits(od[k])), k
    rc, o = abi_solve(stub, costs[:1], n, q, cap, K, eval_costs=costs[:1])
    assert rc == 0
    VC.check_solve(o, sols[:1], objs[:1], routes[:1], n, eval_costs=costs[:1], what="N=1")
    c8, q8, cap8, s8, z8, r8 = VC.host("gen", 8, 3)
    rc, o = abi_solve(stub, c8[:1], 8, q8, cap8, 3, eval_costs=c8[:1])
    assert rc == 0
    VC.check_solve(o, s8[:1], z8[:1], r8[:1], 8, eval_costs=c8[:1], what="N=1, LDS")


def test_one_vehicle_and_a_loose_capacity_is_held_karp(stub):
    n = 8
    costs = VC.instance_of("ties", 4, n, 1)[0]
    ref = [VC.tight.tsp_solve(c, n) for c in costs]
    rc, o = abi_solve(stub, costs, n, np.ones(n - 1), 1e30, 1, eval_costs=costs)
    assert rc == 0
    assert np.array_equal(o["sol"], np.stack([s for s, _, _ in ref])) and np.array_equal(VC.bits(o["obj"]), VC.bits(np.asarray([z for _, z, _ in ref])))
    assert np.array_equal(o["routes"][:, :n], np.asarray([t for _, _, t in ref], np.int32)) and (o["routes"][:, n] == 0).all()


@pytest.mark.parametrize("shape", [(8, 3), (VC.WS_MIN_N, 3)], ids=["lds", "slot"])
def test_failed_instances(stub, shape):
    import torch

    from cave_amd import tight

    n, K = shape
    bad, hit, case = VC.bad_batch(n, K)
    q, cap = case[1], case[2]
    for wsb in (None, 2 * VC.slot_bytes(n, K)) if VC.slot_bytes(n, K) else (None,):   # the bad instance's slot is reused
        rc, o = abi_solve(stub, bad, n, q, cap, K, eval_costs=case[0], workspace_bytes=wsb)
        assert rc == 0
        VC.check_bad(o, hit, case, what=(n, K, wsb))
    for v in (-1.0, np.nan, np.inf):
        qb = q.copy()
        qb[n - 2] = v
        rc, o = abi_solve(stub, case[0], n, qb, cap, K, eval_costs=case[0])
        assert rc == 0
        VC.check_failed(o, VC.ST_BAD_INPUT, what=(n, K, v))
    with pytest.raises(ValueError, match="instance 1"):   # the Python layer refuses the batch
        tight.vrp_solve_hip(torch.tensor(bad, device="cuda"), n, q, cap, K)


def test_infeasible_instances(stub):
    import torch

    from cave_amd import tight

    n = 8
    for costs, q, cap, K, want in VC.infeasible_calls(n):
        rc, o = abi_solve(stub, costs, n, q, cap, K, eval_costs=costs)
        assert rc == 0
        if want is None:
            VC.check_failed(o, VC.ST_INFEASIBLE, what=(cap, K))
            with pytest.raises(ValueError, match="infeasible"):
                tight.vrp_solve_hip(torch.tensor(costs, device="cuda"), n, q, cap, K)
        else:
            VC.check_solve(o, *want, n, eval_costs=costs, what=(cap, K))


@pytest.mark.parametrize("shape", [(5, 2), (VC.WS_MIN_N, 3)], ids=["lds", "slot"])
def test_every_null_output_combination_leaves_the_others_unchanged(stub, shape):
    n, K = shape
    N = 3
    costs, q, cap, sols, objs, routes = VC.host("ties", n, K, N=N, seed=2)
    ev = VC.instance_of("signed", N, n, K, seed=4)[0]
    rc, full = abi_solve(stub, costs, n, q, cap, K, eval_costs=ev)
    assert rc == 0
    VC.check_solve(full, sols, objs, routes, n, eval_costs=ev)
    combos = list(itertools.product((0, 1), repeat=5)) if n == 5 else [(1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 0, 0, 0)]
    for keep in combos:
        flags = sum(f for (_, f), k in zip(EACH, keep) if k)
        for with_ev in (True, False):
            if not with_ev and flags & F_EVAL:
                continue
            rc, o = abi_solve(stub, costs, n, q, cap, K, eval_costs=ev if with_ev else None, flags=flags)
            assert rc == 0, (keep, with_ev)
            for k, f in EACH:
                assert (o[k] is None) == (not flags & f)
                if o[k] is not None:
                    assert np.array_equal(VC.bits(o[k]), VC.bits(full[k])), (keep, with_ev, k)


def test_the_integration_stub_prices_routes(stub):
    """INTEGRATION.md section 13's second function as printed: only eval and status are written"""
    import torch

    from cave_amd import _lib

    lib, ns = stub
    n, K = 8, 3
    pred, q, cap, _, _, routes = VC.host("gen", n, K)
    true = VC.instance_of("signed", len(pred), n, K, seed=3)[0]
    p, t, dq = torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda"), torch.tensor(q, device="cuda")
    ev = torch.zeros(len(pred), dtype=torch.float64, device="cuda")
    st = torch.full((len(pred),), -7, dtype=torch.int32, device="cuda")
    ns["vrp_regret_numerators"](lib, p.data_ptr(), t.data_ptr(), dq.data_ptr(), cap, K, len(pred), n, ev.data_ptr(), st.data_ptr(), None, 0,
                                _lib.current_stream())
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and np.array_equal(VC.bits(ev.cpu().numpy()), VC.bits(VC.routes_eval(true, routes, n)))
    with pytest.raises(RuntimeError, match="workspace"):
        ns["vrp_regret_numerators"](lib, p.data_ptr(), t.data_ptr(), dq.data_ptr(), cap, K, 1, 13, ev.data_ptr(), st.data_ptr(), None, 0,
                                    _lib.current_stream())


@pytest.mark.parametrize("shape", [(8, 3), (VC.LDS_MAX_N, 3), (VC.WS_MIN_N, 3)], ids=lambda s: f"n{s[0]}-K{s[1]}")
def test_python_layer(shape):
    import torch

    from cave_amd import tight

    n, K = shape
    costs, q, cap, sols, objs, routes = VC.host("gen", n, K)
    ev = VC.instance_of("signed", len(costs), n, K, seed=3)[0]
    c, e = torch.tensor(costs, device="cuda"), torch.tensor(ev, device="cuda")
    s, z, t = tight.vrp_solve_hip(c, n, q, cap, K)
    s2, z2, t2, v = tight.vrp_solve_hip(c, n, torch.tensor(q), cap, K, eval_costs=e)
    assert s.dtype == torch.float32 and z.dtype == torch.float64 and t.dtype == torch.int32 and t.shape == (len(costs), n + K)
    assert torch.equal(s, s2) and torch.equal(z, z2) and torch.equal(t, t2)
    VC.check_solve({"sol": s.cpu().numpy(), "obj": z.cpu().numpy(), "routes": t.cpu().numpy(), "eval": v.cpu().numpy()}, sols, objs, routes, n,
                   eval_costs=ev)
    empty = tight.vrp_solve_hip(c[:0], n, q, cap, K)
    assert empty[0].shape == (0, VC.n_edges(n)) and empty[2].shape == (0, n + K)
    with pytest.raises(ValueError):
        tight.vrp_solve_hip(c.cpu(), n, q, cap, K)                    # device
    with pytest.raises(ValueError):
        tight.vrp_solve_hip(c.double(), n, q, cap, K)                 # dtype
    with pytest.raises(ValueError):
        tight.vrp_solve_hip(c[:, :-1], n, q, cap, K)                  # shape
    with pytest.raises(ValueError):
        tight.vrp_solve_hip(c, n, q, cap, K, eval_costs=e[:-1])       # eval_costs shape
    with pytest.raises(ValueError):
        tight.vrp_solve_hip(c, n, q[:-1], cap, K)                     # demands
    for bad_cap in (0.0, float("inf")):
        with pytest.raises(ValueError):
            tight.vrp_solve_hip(c, n, q, bad_cap, K)
    for bad_n, bad_K in ((2, 1), (15, 1), (n, 0), (n, 9)):
        with pytest.raises(ValueError):
            tight.vrp_solve_hip(torch.ones(1, VC.n_edges(bad_n), device="cuda"), bad_n, np.ones(bad_n - 1), 10.0, bad_K)


def test_device_regret_matches_the_host():
    """condition 7, at n = 8, K = 3, N = 32: random predictions against true costs and their true objectives"""
    import torch

    from cave_amd import tight

    n, K, N = 8, 3, 32
    true, q, cap, _, z, _ = (np.array(a) if isinstance(a, np.ndarray) else a for a in VC.host("gen", n, K, N=N, seed=6))
    pred = (true * np.random.default_rng(5).uniform(0.3, 3.0, true.shape)).astype(np.float32)
    z32 = z.astype(np.float32)
    host = tight.vrp_regret(pred, true, z32, n, q, cap, K)
    psols = np.stack([tight.vrp_solve(p, n, q, cap, K)[0] for p in pred])
    bound = VC.regret_bound(true, psols, z32, n, K)
    dev = tight.vrp_regret(pred, true, z32, n, q, cap, K, device="cuda")
    print(f"regret n={n} K={K} N={N}: host {host!r} device {dev!r} |diff| {abs(dev - host):.3e} bound {bound:.3e}")
    assert abs(dev - host) <= bound
    on_dev = tight.vrp_regret(torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda"), torch.tensor(z32, device="cuda"),
                              n, torch.tensor(q, device="cuda"), cap, K, device="cuda")
    assert on_dev == dev


def _example(argv):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_sp_cave

    return train_sp_cave.main(argv)


def test_training_example_device_regret_matches_host_regret():
    """condition 8: the same losses; regrets within condition 7's bound -- tsp_gen_data costs are positive, so
    sum_i c_i . w(c_hat_i) / sum_i |z_i| = 1 + regret and the bound is (n + K) 2^-23 (1 + regret).  The third run solves
    the data set on the device as well: the same bits, so the same history as the second"""
    n, K = 8, 3
    base = ["--problem", "vrp", "--nodes", str(n), "--capacity", "20", "--vehicles", str(K), "--num-data", "24", "--epochs", "2", "--packed"]
    host, dev = _example(base), _example(base + ["--device-regret"])
    both = _example(base + ["--device-regret", "--device-data"])
    assert len(host) == len(dev) == len(both) == 3
    for (e0, l0, r0), (e1, l1, r1), (e2, l2, r2) in zip(host, dev, both):
        print(f"epoch {e0}: loss {l0!r} / {l1!r}  regret {r0!r} / {r1!r}")
        assert e0 == e1 == e2 and (l0 == l1 == l2 or e0 == 0)
        assert abs(r0 - r1) <= (n + K) * 2.0 ** -23 * (1.0 + r0), (e0, r0, r1)
        assert r1 == r2


def test_cvrp_cones_through_the_exact_loss_match_the_cpu_oracle():
    """condition 9: n = 8, B = 8.  The cones carry the depot's `<=` row ahead of the equality rows when all vehicles are
    used, and tight rounded-capacity cuts: the general kernels, not the lite solver"""
    import torch

    from cave_amd import tight
    from cave_amd.cave import EPO, exactConeAlignedCosine
    from oracle import cave_oracle as O
    from torch.nn.utils.rnn import pad_sequence

    n, K, B = 8, 3, 8
    feats, costs, q = tight.vrp_gen_data(B, 5, n, seed=9)
    ds = tight.VRPConeDataset(feats, costs, n, q, 20.0, K, device="cuda")
    host = tight.VRPConeDataset(feats, costs, n, q, 20.0, K)
    assert torch.equal(ds.sols, host.sols) and torch.equal(ds.objs, host.objs) and all(torch.equal(a, b) for a, b in zip(ds.ctrs, host.ctrs))
    ctrs = pad_sequence(ds.ctrs, batch_first=True, padding_value=0.0).numpy()
    pred = (costs * np.random.default_rng(2).uniform(0.5, 2.0, costs.shape)).astype(np.float32)

    class _Model:
        modelSense = EPO.MINIMIZE

    mod = exactConeAlignedCosine(_Model(), solver="hip")
    p = torch.tensor(pred, device="cuda", requires_grad=True)
    loss = mod(p, torch.tensor(ctrs, device="cuda"))
    loss.backward()
    torch.cuda.synchronize()
    ref_loss, ref_grad = O.ConeLossOracle(minimize=True, inner=False)(pred, ctrs)
    dl, dg = abs(float(loss.detach()) - float(ref_loss)), float(np.abs(p.grad.cpu().numpy() - ref_grad).max())
    print(f"CVRP cones n={n} B={B}: rows {ctrs.shape[1]}, tight cuts {ds.tight_cuts}, |dloss| {dl:.2e}, |dgrad| {dg:.2e}")
    assert dl <= 2e-6 and dg <= 8e-6 * max(1.0, float(np.abs(ref_grad).max()))
