"""GPU tier: the wide Held-Karp tier (cave_amd/csrc/tsp_hk_wide.h, k_tsp_hk_wide.hip, 13 <= n <= 20) through the C ABI
(cave_hip_tsp_hk_wide_solve, bound by the ctypes stub of INTEGRATION.md section 14 as printed) and through the Python layer
(tight.tsp_solve_hip_wide, tsp_regret(device=), examples/train_sp_cave.py --nodes 15 --device-regret).

Oracles and bounds are those of the CPU tier (tests/tsp_hk_wide_cases.py, tests/tsp_hk_cases.py): tight.tsp_solve and
cave_hip_tsp_hk_solve at n = 13, 14, the numpy restatement at n = 15, 17, the committed fixture at n = 18, 19, 20; sols,
objs, tours and evals EQUAL; the regret within n 2^-23 sum_i sum_k |c_ik| sol_ik / sum_i |z_i|."""

import os
import re
import sys

import numpy as np
import pytest

import tsp_hk_cases as TC
import tsp_hk_wide_cases as WC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SOL, F_OBJ, F_EVAL, F_TOUR, F_STATUS = 2, 4, 8, 16, 32
F_ALL = 62
EACH = (("sol", F_SOL), ("obj", F_OBJ), ("eval", F_EVAL), ("tour", F_TOUR), ("status", F_STATUS))
GUARD = 8


@pytest.fixture(scope="module")
def stub():
    """a fresh handle of the library bound by INTEGRATION.md section 14's stub, and the stub's functions"""
    import ctypes as C

    from cave_amd import _lib

    _lib.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 14. Held-Karp TSP on the device up to 20 nodes"):]
    ns = {}
    exec(re.search(r"^```py\n(.*?)^```", sec, flags=re.S | re.M).group(1), ns)
    lib = C.CDLL(_lib.LIB_PATH)
    lib.cave_hip_last_error.restype = C.c_char_p
    ns["bind_tsp_hk_wide"](lib)
    norm = lambda t: re.sub(r"\s+", " ", t).strip()
    hdr = norm(open(os.path.join(ROOT, "include", "cave_hip.h")).read())
    protos = re.findall(r"int\d\d_t cave_hip_\w+\([^;]*\);", re.search(r"^```c\n(.*?)^```", sec, flags=re.S | re.M).group(1))
    assert len(protos) == 3 and all(norm(p) in hdr for p in protos)
    return lib, ns


def abi_solve(stub, costs, n, eval_costs=None, flags=F_ALL, workspace_bytes=None, entry="tsp_hk_wide"):
    """cave_hip_<entry>_solve on numpy inputs -> (rc, dict of numpy outputs; None where `flags` gives no buffer).  Outputs
    are sentinel-filled with GUARD extra elements, which are checked and cut off.  `workspace_bytes`: None = the size
    query's default.  entry="tsp_hk": section 12's entry on the package's own handle, for the comparison at n = 13, 14."""
    import torch

    from cave_amd import _lib

    lib = stub[0] if entry == "tsp_hk_wide" else _lib.load()
    N, d = costs.shape[0], TC.n_edges(n)
    c = torch.tensor(costs, device="cuda")
    ev = None if eval_costs is None else torch.tensor(eval_costs, device="cuda")
    size = {"sol": N * d, "obj": N, "eval": N, "tour": N * n, "status": N}
    fill = {"sol": (77.0, torch.float32), "obj": (77.0, torch.float64), "eval": (77.0, torch.float64), "tour": (-7, torch.int32),
            "status": (-7, torch.int32)}
    t = {k: torch.full((size[k] + GUARD,), fill[k][0], dtype=fill[k][1], device="cuda") if flags & f else None for k, f in EACH}
    if workspace_bytes is None:
        workspace_bytes = max(int(getattr(lib, f"cave_hip_{entry}_workspace_bytes")(n, N)), 0)
    ws = torch.full((workspace_bytes // 8,), -1, dtype=torch.int64, device="cuda") if workspace_bytes >= 8 else None
    rc = getattr(lib, f"cave_hip_{entry}_solve")(_lib.ptr(c), _lib.ptr(ev), N, n, _lib.ptr(t["sol"]), _lib.ptr(t["obj"]),
                                                 _lib.ptr(t["eval"]), _lib.ptr(t["tour"]), _lib.ptr(t["status"]), _lib.ptr(ws),
                                                 workspace_bytes if ws is not None else 0, _lib.current_stream())
    torch.cuda.synchronize()
    o = {}
    shape = {"sol": (N, d), "obj": (N,), "eval": (N,), "tour": (N, n), "status": (N,)}
    for k, v in t.items():
        if v is None:
            o[k] = None
            continue
        a = v.cpu().numpy()
        assert (a[size[k]:] == fill[k][0]).all(), (k, "written beyond its end")
        if rc != 0:
            assert (a == fill[k][0]).all(), (k, "written by a rejected call")
        o[k] = a[:size[k]].reshape(shape[k])
    return int(rc), o


def same_bytes(a, b, what=""):
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(TC.bits(a[k]), TC.bits(b[k]))), (what, k)


def test_size_queries_and_rejected_arguments(stub):
    lib, _ = stub
    for n in range(0, 23):
        assert lib.cave_hip_tsp_hk_wide_slot_bytes(n) == WC.slot_bytes(n), n
        for N in (0, 1, 5, 215, 216, 455, 456, 512, 513, 100000, -1):
            assert lib.cave_hip_tsp_hk_wide_workspace_bytes(n, N) == WC.workspace_bytes(n, N), (n, N)
    for n in (12, 21):
        assert abi_solve(stub, np.ones((1, TC.n_edges(n)), np.float32), n, flags=F_SOL, workspace_bytes=1 << 20)[0] == TC.E_INVALID
        assert b"13 <= n <= 20" in lib.cave_hip_last_error()
    c = TC.costs_of("ties", 2, 15)
    assert abi_solve(stub, c, 15, flags=F_EVAL)[0] == TC.E_INVALID                               # eval without eval_costs
    assert abi_solve(stub, c[:0], 15, flags=F_SOL, workspace_bytes=0)[0] == 0                    # N == 0
    for n in (13, 15):                                                                           # a slot is needed
        c = TC.costs_of("ties", 2, n)
        for wsb in (0, 8, WC.slot_bytes(n) - 8, WC.header_bytes(n) + WC.slot_bytes(n) - 8):
            assert abi_solve(stub, c, n, eval_costs=c, workspace_bytes=wsb)[0] == TC.E_INVALID, (n, wsb)   # (nothing written)
        assert b"workspace" in lib.cave_hip_last_error()


@pytest.mark.parametrize("n", [13, 14])
@pytest.mark.parametrize("kind", TC.KINDS)
def test_n13_n14_equal_the_host_and_the_first_tier(stub, kind, n):
    costs, sols, objs, tours = TC.host(kind, n)
    ev = TC.costs_of("signed", len(costs), n, seed=3)
    rc, o = abi_solve(stub, costs, n, eval_costs=ev)
    assert rc == 0
    TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=(kind, n))
    rc, o12 = abi_solve(stub, costs, n, eval_costs=ev, entry="tsp_hk")
    assert rc == 0
    same_bytes(o, o12, (kind, n, "cave_hip_tsp_hk_solve"))


@pytest.mark.parametrize("n,N", [(15, 3), (17, 2)])
def test_n15_n17_equal_the_restatement(stub, n, N):
    costs, sols, objs, tours = WC.ref("gen" if n == 15 else "ties", n, N=N)
    ev = TC.costs_of("signed", N, n, seed=3)
    rc, o = abi_solve(stub, costs, n, eval_costs=ev)
    assert rc == 0
    TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=n)


@pytest.mark.parametrize("n", WC.GOLDEN_NS)
def test_n18_to_n20_equal_the_fixture(stub, n):
    costs, sols, objs, tours, _ = WC.golden(n)
    ev = TC.costs_of("signed", 3, n, seed=3)
    rc, o = abi_solve(stub, costs, n, eval_costs=ev)
    assert rc == 0
    TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=n)


def test_repeatability_batch_order_slot_reuse_and_a_batch_of_one(stub):
    n = 15
    costs, sols, objs, tours = WC.ref("ties", n, N=5, seed=1)
    rc, o = abi_solve(stub, costs, n, eval_costs=costs)
    assert rc == 0
    TC.check_solve(o, sols, objs, tours, n, eval_costs=costs, what="default workspace")
    rc, o2 = abi_solve(stub, costs, n, eval_costs=costs)   # two launches: the same bytes
    assert rc == 0
    same_bytes(o, o2, "second launch")
    perm = np.roll(np.arange(len(costs)), 1)[::-1].copy()   # the same instances in another batch order
    rc, o3 = abi_solve(stub, costs[perm], n, eval_costs=costs[perm])
    assert rc == 0
    same_bytes(o3, {k: v[perm] for k, v in o.items()}, "batch order")
    # slot reuse and a tail: workgroup 0 takes instances 0, 2, 4 and workgroup 1 instances 1, 3
    rc, o4 = abi_solve(stub, costs, n, eval_costs=costs, workspace_bytes=WC.header_bytes(n) + 2 * WC.slot_bytes(n))
    assert rc == 0
    same_bytes(o, o4, "two slots")
    rc, o1 = abi_solve(stub, costs[:1], n, eval_costs=costs[:1])
    assert rc == 0
    same_bytes(o1, {k: v[:1] for k, v in o.items()}, "N = 1")


def test_slots_beyond_4_gib(stub):
    """n = 20, N = 110 on a workspace of exactly 110 slots (4.38 GB): slots 108 and 109 begin beyond 4 GiB, so a slot
    offset in 32 bits would send their workgroups into the slots of others"""
    n, N = 20, 110
    assert 108 * WC.slot_bytes(n) > 1 << 32 > 107 * WC.slot_bytes(n)
    costs, sols, objs, tours, _ = WC.golden(n)
    rows = np.arange(N) % 3
    rc, o = abi_solve(stub, costs[rows], n, eval_costs=costs[rows], workspace_bytes=WC.header_bytes(n) + N * WC.slot_bytes(n))
    assert rc == 0
    TC.check_solve(o, sols[rows], objs[rows], tours[rows], n, eval_costs=costs[rows], what="110 slots")


def test_a_non_finite_cost_fails_its_instance_alone(stub):
    n = 15
    bad, hit, ref = WC.bad_batch(n)
    clean = WC.ref("gen", n, N=6, seed=3)[0]
    for wsb in (None, WC.header_bytes(n) + 2 * WC.slot_bytes(n)):   # the bad instance's slot is reused
        rc, o = abi_solve(stub, bad, n, eval_costs=clean, workspace_bytes=wsb)
        assert rc == 0
        TC.check_bad(o, hit, ref, len(bad), what=(n, wsb))


def test_the_integration_stub_prices_tours(stub):
    """INTEGRATION.md section 14's second function as printed: only eval and status are written"""
    import torch

    from cave_amd import _lib

    lib, ns = stub
    n = 15
    pred, _, _, tours = WC.ref("gen", n, N=3)
    true = TC.costs_of("signed", len(pred), n, seed=3)
    p, t = torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda")
    ev = torch.zeros(len(pred), dtype=torch.float64, device="cuda")
    st = torch.full((len(pred),), -7, dtype=torch.int32, device="cuda")
    wsb = int(lib.cave_hip_tsp_hk_wide_workspace_bytes(n, len(pred)))
    ws = torch.empty(wsb // 8, dtype=torch.float64, device="cuda")
    ns["tsp_regret_numerators_wide"](lib, p.data_ptr(), t.data_ptr(), len(pred), n, ev.data_ptr(), st.data_ptr(), ws.data_ptr(), wsb,
                                     _lib.current_stream())
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and np.array_equal(TC.bits(ev.cpu().numpy()), TC.bits(TC.tour_eval(true, tours, n)))
    with pytest.raises(RuntimeError, match="workspace"):
        ns["tsp_regret_numerators_wide"](lib, p.data_ptr(), t.data_ptr(), 1, n, ev.data_ptr(), st.data_ptr(), None, 0, _lib.current_stream())


def test_python_layer():
    import torch

    from cave_amd import tight

    n = 15
    assert "tsp_solve_hip_wide" in tight.__all__
    costs, sols, objs, tours = WC.ref("gen", n, N=3)
    ev = TC.costs_of("signed", len(costs), n, seed=3)
    c, e = torch.tensor(costs, device="cuda"), torch.tensor(ev, device="cuda")
    s, z, t = tight.tsp_solve_hip_wide(c, n)
    s2, z2, t2, v = tight.tsp_solve_hip_wide(c, n, eval_costs=e)
    assert s.dtype == torch.float32 and z.dtype == torch.float64 and t.dtype == torch.int32 and v.dtype == torch.float64
    assert torch.equal(s, s2) and torch.equal(z, z2) and torch.equal(t, t2)
    TC.check_solve({"sol": s.cpu().numpy(), "obj": z.cpu().numpy(), "tour": t.cpu().numpy(), "eval": v.cpu().numpy()}, sols, objs, tours, n,
                   eval_costs=ev)
    empty = tight.tsp_solve_hip_wide(c[:0], n)
    assert empty[0].shape == (0, TC.n_edges(n)) and empty[2].shape == (0, n)
    with pytest.raises(ValueError):
        tight.tsp_solve_hip_wide(c.cpu(), n)                       # device
    with pytest.raises(ValueError):
        tight.tsp_solve_hip_wide(c.double(), n)                    # dtype
    with pytest.raises(ValueError):
        tight.tsp_solve_hip_wide(c[:, :-1], n)                     # shape
    with pytest.raises(ValueError):
        tight.tsp_solve_hip_wide(c, n, eval_costs=e[:-1])          # eval_costs shape
    for bad_n in (12, 21):
        with pytest.raises(ValueError, match="13 <= n <= 20"):
            tight.tsp_solve_hip_wide(torch.ones(1, TC.n_edges(bad_n), device="cuda"), bad_n)
    with pytest.raises(ValueError, match="3 <= n <= 14"):          # the first tier keeps its limit
        tight.tsp_solve_hip(c, n)
    bad = costs.copy()
    bad[1, 7] = np.nan
    with pytest.raises(ValueError, match="instance 1"):
        tight.tsp_solve_hip_wide(torch.tensor(bad, device="cuda"), n)


def test_device_regret_at_15_nodes():
    """n = 15, N = 8: random predictions against true costs and their true objectives.  The host's side of the comparison
    is tsp_regret's own arithmetic (a float32 dot product c . sol per instance) on the restatement's sols, since the host
    solver stops at 14 nodes; the bound is tsp_hk_cases.regret_bound"""
    from cave_amd import tight

    n, N = 15, 8
    true, _, z, _ = (np.array(a) for a in WC.ref("gen", n, N=N, seed=6))
    pred = (true * np.random.default_rng(5).uniform(0.3, 3.0, true.shape)).astype(np.float32)
    z32 = z.astype(np.float32)
    psols = np.stack([WC.solve_ref(p, n)[0] for p in pred])
    host = sum(float(c @ s) - float(zi) for c, s, zi in zip(true, psols, z32)) / float(np.abs(z32).sum() + 1e-7)
    bound = TC.regret_bound(true, psols, z32, n)
    dev = tight.tsp_regret(pred, true, z32, n, device="cuda")
    print(f"regret n={n} N={N}: host {host!r} device {dev!r} |diff| {abs(dev - host):.3e} bound {bound:.3e}")
    assert abs(dev - host) <= bound
    with pytest.raises(ValueError):   # the host limit stays
        tight.tsp_regret(pred[:1], true[:1], z32[:1], n)


def _example(argv):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_sp_cave

    return train_sp_cave.main(argv)


def test_training_example_at_15_nodes(capsys):
    base = ["--problem", "tsp", "--nodes", "15", "--num-data", "16", "--epochs", "1"]
    with pytest.raises(SystemExit):   # above 14 nodes the regret needs the device; said before the data set is built
        _example(base)
    assert "--device-regret" in capsys.readouterr().err
    hist = _example(base + ["--device-regret"])
    assert len(hist) == 2 and all(np.isfinite(x[2]) for x in hist) and np.isfinite(hist[1][1])
    assert "regret" in capsys.readouterr().out
