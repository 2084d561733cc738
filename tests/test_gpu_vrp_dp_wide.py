"""GPU tier: the wide CVRP tier (cave_amd/csrc/vrp_dp_wide.h, k_vrp_dp_wide.hip) through the C ABI
(cave_hip_vrp_dp_wide_solve, bound by the ctypes stub of INTEGRATION.md section 15 as printed) and through the Python
layer (tight.vrp_solve_hip_wide, vrp_regret(device=), VRPConeDataset(device=)).

Oracles: tight.vrp_solve up to n = 14 (and the first entry's bytes there), the numpy restatement and its committed
fixture beyond; cases and bounds are those of the CPU tier (tests/vrp_dp_wide_cases.py):
  1. objs, routes and sols equal the oracle's bit for bit, ties, negative costs and loads equal to the capacity included
  2. evals equal the fp64 sum of the routes' edges under eval_costs in route order, bit for bit
  3. a non-finite cost fails its instance alone, a bad demand every instance; infeasible instances report
     CAVE_ST_INFEASIBLE                                 4. absent outputs leave the others unchanged; nothing is written
     beyond an output                                   5. rejected arguments (outputs untouched), size queries
  6. one slot for three instances, fewer slots than instances, the default workspace: the same bytes per instance
  7. 104 slots at n = 20: slot offsets beyond 4 GiB
  8. vrp_regret(device=) within vrp_dp_cases.regret_bound of the sum formed from the reference results, through the
     first entry at n = 12 and through this one at n = 15
  9. VRPConeDataset(device=) at n = 15: the reference's sols and objs, rows that are vrp_tight_normals of them."""

import os
import re

import numpy as np
import pytest

import vrp_dp_cases as VC
import vrp_dp_wide_cases as WC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SOL, F_OBJ, F_EVAL, F_ROUTES, F_STATUS = 2, 4, 8, 16, 32
F_ALL = 62
EACH = (("sol", F_SOL), ("obj", F_OBJ), ("eval", F_EVAL), ("routes", F_ROUTES), ("status", F_STATUS))
GUARD = 8


@pytest.fixture(scope="module")
def stub():
    """a fresh handle of the library bound by INTEGRATION.md section 15's stub (and section 13's, for the first entry)"""
    import ctypes as C

    from cave_amd import _lib

    _lib.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.cave_hip_last_error.restype = C.c_char_p
    ns = {}
    for title in ("## 13. CVRP on the device", "## 15. CVRP on the device up to 20 nodes"):
        sec = doc[doc.index(title):]
        exec(re.search(r"^```py\n(.*?)^```", sec, flags=re.S | re.M).group(1), ns)
    ns["bind_vrp_dp"](lib)
    ns["bind_vrp_dp_wide"](lib)
    norm = lambda t: re.sub(r"\s+", " ", t).strip()
    hdr = norm(open(os.path.join(ROOT, "include", "cave_hip.h")).read())
    protos = re.findall(r"int\d\d_t cave_hip_\w+\([^;]*\);", re.search(r"^```c\n(.*?)^```", sec, flags=re.S | re.M).group(1))
    assert len(protos) == 3 and all(norm(p) in hdr for p in protos)
    assert "#define CAVE_HIP_ABI_VERSION 10" in hdr
    return lib, ns


def abi_solve(stub, costs, n, demands, capacity, K, eval_costs=None, flags=F_ALL, workspace_bytes=None, null=(), entry="vrp_dp_wide"):
    """cave_hip_<entry>_solve on numpy inputs -> (rc, dict of numpy outputs; None where `flags` gives no buffer).  Outputs
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
        workspace_bytes = max(int(getattr(lib, f"cave_hip_{entry}_workspace_bytes")(n, K, N)), 0)
    ws = torch.full((workspace_bytes // 8,), -1, dtype=torch.int64, device="cuda") if workspace_bytes >= 8 else None
    rc = getattr(lib, f"cave_hip_{entry}_solve")(
        _lib.ptr(None if "costs" in null else c), _lib.ptr(ev), _lib.ptr(None if "demands" in null else q), float(capacity), K, N, n,
        _lib.ptr(t["sol"]), _lib.ptr(t["obj"]), _lib.ptr(t["eval"]), _lib.ptr(t["routes"]), _lib.ptr(t["status"]), _lib.ptr(ws),
        workspace_bytes if ws is not None else 0, _lib.current_stream())
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


def case_of(kind, n, K):
    """(costs, demands, capacity, sols, objs, routes) of a shape of the table: the fixture's row of `kind` at n = 18, 20,
    else the oracle's batch"""
    if (n, K) in WC.GOLDEN_SHAPES:
        i = WC.KINDS.index(kind)
        c, q, cap, sols, objs, routes = WC.golden(n, K)
        return c[i:i + 1], q[i], float(cap[i]), sols[i:i + 1], objs[i:i + 1], routes[i:i + 1]
    return WC.ref(kind, n, K)


def test_size_queries_and_rejected_arguments(stub):
    lib, _ = stub
    for n in range(0, 23):
        for K in range(0, 10):
            assert lib.cave_hip_vrp_dp_wide_slot_bytes(n, K) == WC.slot_bytes(n, K), (n, K)
            for N in (0, 1, 5, 124, 125, 195, 196, 512, 513, 100000, -1):
                assert lib.cave_hip_vrp_dp_wide_workspace_bytes(n, K, N) == WC.workspace_bytes(n, K, N), (n, K, N)
    n, K = 13, 3
    c, q, cap = WC.ref("gen", n, K)[:3]
    for nn, kk in ((12, 3), (21, 3), (13, 0), (13, 9)):   # n or K out of range
        assert abi_solve(stub, np.ones((1, VC.n_edges(nn)), np.float32), nn, np.ones(nn - 1), 1e3, kk, flags=F_SOL,
                         workspace_bytes=1 << 20)[0] == WC.E_INVALID
        assert b"13 <= n <= 20 and 1 <= K <= 8" in lib.cave_hip_last_error()
    assert abi_solve(stub, c, n, q, cap, K, flags=F_EVAL)[0] == WC.E_INVALID                        # eval without eval_costs
    for bad_cap in (0.0, -1.0, np.inf, np.nan):
        assert abi_solve(stub, c, n, q, bad_cap, K, eval_costs=c)[0] == WC.E_INVALID, bad_cap
    assert b"capacity" in lib.cave_hip_last_error()
    assert abi_solve(stub, c, n, q, cap, K, eval_costs=c, null=("demands",))[0] == WC.E_INVALID
    assert abi_solve(stub, c, n, q, cap, K, eval_costs=c, null=("costs",))[0] == WC.E_INVALID
    for wsb in (0, 8, WC.slot_bytes(n, K), WC.header_bytes(n) + WC.slot_bytes(n, K) - 8):            # too small
        assert abi_solve(stub, c, n, q, cap, K, eval_costs=c, workspace_bytes=wsb)[0] == WC.E_INVALID, wsb
        assert b"workspace" in lib.cave_hip_last_error()
    assert abi_solve(stub, np.zeros((0, VC.n_edges(n)), np.float32), n, q, cap, K, flags=F_SOL, workspace_bytes=0)[0] == 0   # N == 0


@pytest.mark.parametrize("shape", list(WC.SHAPES), ids=lambda s: f"n{s[0]}-K{s[1]}")
@pytest.mark.parametrize("kind", WC.KINDS)
def test_abi_routes_objectives_and_evals_equal_the_oracle(stub, kind, shape):
    n, K = shape
    costs, q, cap, sols, objs, routes = case_of(kind, n, K)
    ev = VC.instance_of("signed", len(costs), n, K, seed=3)[0]
    rc, o = abi_solve(stub, costs, n, q, cap, K, eval_costs=ev)
    assert rc == 0
    VC.check_solve(o, sols, objs, routes, n, eval_costs=ev, what=(kind, n, K))
    if n <= 14:  # the same bytes as the first entry (its tier 1; tier 2 at n = 13, K = 6)
        rc, o1 = abi_solve(stub, costs, n, q, cap, K, eval_costs=ev, entry="vrp_dp")
        assert rc == 0
        for k in o:
            assert np.array_equal(VC.bits(o[k]), VC.bits(o1[k])), (kind, n, K, k)
    if n <= 17:  # two launches, and the same instances in another batch order: the same bytes
        perm = np.roll(np.arange(len(costs)), 1)[::-1].copy()
        rc, o3 = abi_solve(stub, costs[perm], n, q, cap, K, eval_costs=ev[perm])
        assert rc == 0
        for k in o:
            assert np.array_equal(VC.bits(o3[k]), VC.bits(o[k][perm])), (kind, n, K, k, "batch order")


def test_one_slot_for_three_instances_and_fewer_slots_than_instances(stub):
    """a workspace of one slot with N = 3 reuses the slot; two slots for five instances leave a tail: workgroup 0 takes
    instances 0, 2, 4 and workgroup 1 instances 1, 3; the default workspace (five slots) gives the same bytes"""
    n, K = 15, 3
    costs, q, cap, sols, objs, routes = WC.ref("ties", n, K, N=5, seed=1)
    one = WC.header_bytes(n) + WC.slot_bytes(n, K)
    rc, o = abi_solve(stub, costs[:3], n, q, cap, K, eval_costs=costs[:3], workspace_bytes=one)
    assert rc == 0
    VC.check_solve(o, sols[:3], objs[:3], routes[:3], n, eval_costs=costs[:3], what="one slot")
    rc, o = abi_solve(stub, costs, n, q, cap, K, eval_costs=costs, workspace_bytes=one + WC.slot_bytes(n, K) + 8)
    assert rc == 0
    VC.check_solve(o, sols, objs, routes, n, eval_costs=costs, what="two slots")
    rc, od = abi_solve(stub, costs, n, q, cap, K, eval_costs=costs)
    assert rc == 0
    for k in o:
        assert np.array_equal(VC.bits(o[k]), VC.bits(od[k])), k


def test_failed_instances(stub):
    import torch

    from cave_amd import tight

    n, K = 15, 3
    bad, hit, case = WC.bad_batch(n, K)
    q, cap = case[1], case[2]
    for wsb in (None, WC.header_bytes(n) + 2 * WC.slot_bytes(n, K)):   # the bad instance's slot is reused
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
        tight.vrp_solve_hip_wide(torch.tensor(bad, device="cuda"), n, q, cap, K)


def test_infeasible_instances(stub):
    import torch

    from cave_amd import tight

    n = 15
    for costs, q, cap, K, want in WC.infeasible_calls(n):
        rc, o = abi_solve(stub, costs, n, q, cap, K, eval_costs=costs)
        assert rc == 0
        if want is None:
            VC.check_failed(o, VC.ST_INFEASIBLE, what=(cap, K))
            with pytest.raises(ValueError, match="infeasible"):
                tight.vrp_solve_hip_wide(torch.tensor(costs, device="cuda"), n, q, cap, K)
        else:
            VC.check_solve(o, *want, n, eval_costs=costs, what=(cap, K))


def test_null_output_combinations_leave_the_others_unchanged(stub):
    """the combination classes of tests/test_gpu_vrp_dp.py at a slot shape"""
    n, K, N = 15, 3, 3
    costs, q, cap, sols, objs, routes = WC.ref("ties", n, K, N=N, seed=2)
    ev = VC.instance_of("signed", N, n, K, seed=4)[0]
    rc, full = abi_solve(stub, costs, n, q, cap, K, eval_costs=ev)
    assert rc == 0
    VC.check_solve(full, sols, objs, routes, n, eval_costs=ev)
    for keep in [(1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 0, 0, 0)]:
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
    """INTEGRATION.md section 15's second function as printed: only eval and status are written"""
    import torch

    from cave_amd import _lib

    lib, ns = stub
    n, K = 15, 3
    pred, q, cap, _, _, routes = WC.ref("gen", n, K)
    true = VC.instance_of("signed", len(pred), n, K, seed=3)[0]
    p, t, dq = torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda"), torch.tensor(q, device="cuda")
    ev = torch.zeros(len(pred), dtype=torch.float64, device="cuda")
    st = torch.full((len(pred),), -7, dtype=torch.int32, device="cuda")
    wsb = WC.workspace_bytes(n, K, len(pred))
    ws = torch.empty(wsb // 8, dtype=torch.float64, device="cuda")
    ns["vrp_regret_numerators_wide"](lib, p.data_ptr(), t.data_ptr(), dq.data_ptr(), cap, K, len(pred), n, ev.data_ptr(), st.data_ptr(),
                                     ws.data_ptr(), wsb, _lib.current_stream())
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and np.array_equal(VC.bits(ev.cpu().numpy()), VC.bits(VC.routes_eval(true, routes, n)))
    with pytest.raises(RuntimeError, match="workspace"):
        ns["vrp_regret_numerators_wide"](lib, p.data_ptr(), t.data_ptr(), dq.data_ptr(), cap, K, 1, n, ev.data_ptr(), st.data_ptr(), None, 0,
                                         _lib.current_stream())


def test_slot_offsets_beyond_4_gib(stub):
    """n = 20 at K = 2 (no stored layer: phase 1 plus one split), 104 slots and N = 104: slot 98 starts beyond 4 GiB, the
    workspace has about 4.6 GB.  The rows are the fixture's instances repeated, and every row must equal its fixture; the
    demands and the capacity belong to the call, not to the row, and the fixture's three kinds have their own, so each
    kind fills a call of 104 rows."""
    import torch

    n, K, N = 20, 2, 104
    c, q, cap, sols, objs, routes = WC.golden(n, K)
    assert 97 * WC.slot_bytes(n, K) < 1 << 32 <= 98 * WC.slot_bytes(n, K)
    wsb = WC.header_bytes(n) + N * WC.slot_bytes(n, K)
    free, _ = torch.cuda.mem_get_info()
    assert free > wsb + (1 << 30), "the device has too little free memory for this test"
    for i in range(3):   # the three fixture instances, each repeated over all 104 slots (the demands are per call)
        rep = np.repeat(c[i:i + 1], N, axis=0)
        rc, o = abi_solve(stub, rep, n, q[i], float(cap[i]), K, eval_costs=rep, workspace_bytes=wsb)
        assert rc == 0
        VC.check_solve(o, np.repeat(sols[i:i + 1], N, 0), np.repeat(objs[i:i + 1], N), np.repeat(routes[i:i + 1], N, 0), n,
                       eval_costs=rep, what=("4 GiB", i))


@pytest.mark.parametrize("shape", [(13, 3), (15, 3), (15, 1)], ids=lambda s: f"n{s[0]}-K{s[1]}")
def test_python_layer(shape):
    import torch

    from cave_amd import tight

    assert "vrp_solve_hip_wide" in tight.__all__
    n, K = shape
    costs, q, cap, sols, objs, routes = WC.ref("gen", n, K)
    ev = VC.instance_of("signed", len(costs), n, K, seed=3)[0]
    c, e = torch.tensor(costs, device="cuda"), torch.tensor(ev, device="cuda")
    s, z, t = tight.vrp_solve_hip_wide(c, n, q, cap, K)
    s2, z2, t2, v = tight.vrp_solve_hip_wide(c, n, torch.tensor(q), cap, K, eval_costs=e)
    assert s.dtype == torch.float32 and z.dtype == torch.float64 and t.dtype == torch.int32 and t.shape == (len(costs), n + K)
    assert torch.equal(s, s2) and torch.equal(z, z2) and torch.equal(t, t2)
    VC.check_solve({"sol": s.cpu().numpy(), "obj": z.cpu().numpy(), "routes": t.cpu().numpy(), "eval": v.cpu().numpy()}, sols, objs, routes, n,
                   eval_costs=ev)
    empty = tight.vrp_solve_hip_wide(c[:0], n, q, cap, K)
    assert empty[0].shape == (0, VC.n_edges(n)) and empty[2].shape == (0, n + K)
    with pytest.raises(ValueError):
        tight.vrp_solve_hip_wide(c.cpu(), n, q, cap, K)                    # device
    with pytest.raises(ValueError):
        tight.vrp_solve_hip_wide(c.double(), n, q, cap, K)                 # dtype
    with pytest.raises(ValueError):
        tight.vrp_solve_hip_wide(c[:, :-1], n, q, cap, K)                  # shape
    with pytest.raises(ValueError):
        tight.vrp_solve_hip_wide(c, n, q, cap, K, eval_costs=e[:-1])       # eval_costs shape
    with pytest.raises(ValueError):
        tight.vrp_solve_hip_wide(c, n, q[:-1], cap, K)                     # demands
    for bad_cap in (0.0, float("inf")):
        with pytest.raises(ValueError):
            tight.vrp_solve_hip_wide(c, n, q, bad_cap, K)
    for bad_n, bad_K in ((12, 1), (21, 1), (n, 0), (n, 9)):
        with pytest.raises(ValueError):
            tight.vrp_solve_hip_wide(torch.ones(1, VC.n_edges(bad_n), device="cuda"), bad_n, np.ones(bad_n - 1), 1e3, bad_K)


@pytest.mark.parametrize("n", [12, 15])
def test_device_regret_takes_the_entry_of_its_size(n, monkeypatch):
    """condition 8: n = 12 goes through vrp_solve_hip, n = 15 through vrp_solve_hip_wide; random predictions against true
    costs and their true objectives, the regret within regret_bound of the sum formed from the reference results"""
    import torch

    from cave_amd import tight

    K, N = 3, 6
    true, q, cap, _, z, _ = WC.ref("gen", n, K, N=N, seed=6) if n > 14 else VC.host("gen", n, K, N=N, seed=6)
    pred = (true * np.random.default_rng(5).uniform(0.3, 3.0, true.shape)).astype(np.float32)
    z32 = z.astype(np.float32)
    solve = (lambda p: tight.vrp_solve(p, n, q, cap, K)) if n <= 14 else (lambda p: WC.solve_ref(p, n, q, cap, K))
    psols = np.stack([solve(p)[0] for p in pred])
    want = sum(float(c @ s) - float(zi) for c, s, zi in zip(true, psols, z32)) / float(np.abs(z32).sum() + 1e-7)
    bound = VC.regret_bound(true, psols, z32, n, K)
    calls = []
    for name in ("vrp_solve_hip", "vrp_solve_hip_wide"):
        monkeypatch.setattr(tight, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(tight, name), name))
    dev = tight.vrp_regret(pred, true, z32, n, q, cap, K, device="cuda")
    print(f"regret n={n} K={K} N={N}: reference {want!r} device {dev!r} |diff| {abs(dev - want):.3e} bound {bound:.3e}")
    assert calls == ["vrp_solve_hip" if n <= 14 else "vrp_solve_hip_wide"]
    assert abs(dev - want) <= bound
    on_dev = tight.vrp_regret(torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda"), torch.tensor(z32, device="cuda"),
                              n, torch.tensor(q, device="cuda"), cap, K, device="cuda")
    assert on_dev == dev
    if n > 14:
        with pytest.raises(ValueError):   # without a device the host's limit holds
            tight.vrp_regret(pred, true, z32, n, q, cap, K)


def test_cone_dataset_on_the_device_at_15_nodes():
    """condition 9: two instances; the cut loop (HiGHS, host) runs inside the constructor -- about a second per instance at
    this size"""
    import torch

    from cave_amd import tight

    n, K = 15, 3
    costs, q, cap, sols, objs, _ = WC.ref("gen", n, K, N=2)
    feats = np.zeros((2, 5), np.float32)
    ds = tight.VRPConeDataset(feats, costs, n, q, cap, K, device="cuda")
    assert torch.equal(ds.sols, torch.as_tensor(sols)) and torch.equal(ds.objs[:, 0], torch.as_tensor(objs.astype(np.float32)))
    for i in range(2):
        cuts = tight.vrp_rcc_cuts(costs[i], n, q, cap, K)[2]
        assert torch.equal(ds.ctrs[i], torch.as_tensor(tight.vrp_tight_normals(sols[i], n, cuts, K)))
    with pytest.raises(ValueError):   # without a device the host's limit holds
        tight.VRPConeDataset(feats, costs, n, q, cap, K)
