"""GPU tier: the Held-Karp kernels (cave_amd/csrc/tsp_hk.h, k_tsp_hk.hip) through the C ABI (cave_hip_tsp_hk_solve, bound
by the ctypes stub of INTEGRATION.md section 12 as printed) and through the Python layer (tight.tsp_solve_hip,
tsp_regret(device=), examples/train_sp_cave.py --device-regret).

Oracle: tight.tsp_solve; cases and bounds are those of the CPU tier (tests/tsp_hk_cases.py):
  1. objs, tours and sols equal the host's bit for bit, ties and negative costs included
  2. evals equal the fp64 sum of the tour's edges under eval_costs in tour order, bit for bit
  3. a non-finite cost fails its instance alone        4. absent outputs leave the others unchanged; nothing is written
     beyond an output                                   5. rejected arguments, size queries
  6. two launches, a two-slot and the default workspace, another batch order: the same bytes per instance
  7. tsp_regret(device=) within n 2^-23 sum_i sum_k |c_ik| sol_ik / sum_i |z_i| of the host's (the rounding of the host's
     float32 c @ s)                                     8. the training example with --device-regret."""

import itertools
import os
import re
import sys

import numpy as np
import pytest

import tsp_hk_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SOL, F_OBJ, F_EVAL, F_TOUR, F_STATUS = 2, 4, 8, 16, 32
F_ALL = 62
EACH = (("sol", F_SOL), ("obj", F_OBJ), ("eval", F_EVAL), ("tour", F_TOUR), ("status", F_STATUS))
GUARD = 8


@pytest.fixture(scope="module")
def stub():
    """a fresh handle of the library bound by INTEGRATION.md section 12's stub, and the stub's functions"""
    import ctypes as C

    from cave_amd import _lib

    _lib.load()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 12. Held-Karp TSP on the device"):]
    ns = {}
    exec(re.search(r"^```py\n(.*?)^```", sec, flags=re.S | re.M).group(1), ns)
    lib = C.CDLL(_lib.LIB_PATH)
    lib.cave_hip_last_error.restype = C.c_char_p
    ns["bind_tsp_hk"](lib)
    norm = lambda t: re.sub(r"\s+", " ", t).strip()
    hdr = norm(open(os.path.join(ROOT, "include", "cave_hip.h")).read())
    protos = re.findall(r"int\d\d_t cave_hip_\w+\([^;]*\);", re.search(r"^```c\n(.*?)^```", sec, flags=re.S | re.M).group(1))
    assert len(protos) == 3 and all(norm(p) in hdr for p in protos)
    return lib, ns


def abi_solve(stub, costs, n, eval_costs=None, flags=F_ALL, workspace_bytes=None):
    """cave_hip_tsp_hk_solve on numpy inputs -> (rc, dict of numpy outputs; None where `flags` gives no buffer).  Outputs
    are sentinel-filled with GUARD extra elements, which are checked and cut off.  `workspace_bytes`: None = the size
    query's default."""
    import torch

    from cave_amd import _lib

    lib, ns = stub
    N, d = costs.shape[0], TC.n_edges(n)
    c = torch.tensor(costs, device="cuda")
    ev = None if eval_costs is None else torch.tensor(eval_costs, device="cuda")
    size = {"sol": N * d, "obj": N, "eval": N, "tour": N * n, "status": N}
    fill = {"sol": (77.0, torch.float32), "obj": (77.0, torch.float64), "eval": (77.0, torch.float64), "tour": (-7, torch.int32),
            "status": (-7, torch.int32)}
    t = {k: torch.full((size[k] + GUARD,), fill[k][0], dtype=fill[k][1], device="cuda") if flags & f else None for k, f in EACH}
    if workspace_bytes is None:
        workspace_bytes = max(int(lib.cave_hip_tsp_hk_workspace_bytes(n, N)), 0)
    ws = torch.full((workspace_bytes // 8,), -1, dtype=torch.int64, device="cuda") if workspace_bytes >= 8 else None
    rc = lib.cave_hip_tsp_hk_solve(_lib.ptr(c), _lib.ptr(ev), N, n, _lib.ptr(t["sol"]), _lib.ptr(t["obj"]), _lib.ptr(t["eval"]),
                                   _lib.ptr(t["tour"]), _lib.ptr(t["status"]), _lib.ptr(ws), workspace_bytes if ws is not None else 0,
                                   _lib.current_stream())
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


def test_size_queries_and_rejected_arguments(stub):
    lib, _ = stub
    for n in range(0, 17):
        assert lib.cave_hip_tsp_hk_slot_bytes(n) == TC.slot_bytes(n), n
        for N in (0, 1, 5, 512, 513, 100000, -1):
            assert lib.cave_hip_tsp_hk_workspace_bytes(n, N) == TC.workspace_bytes(n, N), (n, N)
    for n in (2, 15):
        assert abi_solve(stub, np.ones((1, TC.n_edges(n)), np.float32), n, flags=F_SOL, workspace_bytes=0)[0] == TC.E_INVALID
    assert b"3 <= n <= 14" in lib.cave_hip_last_error()
    c = TC.host("gen", 4)[0]
    assert abi_solve(stub, c, 4, flags=F_EVAL)[0] == TC.E_INVALID                      # eval without eval_costs
    assert abi_solve(stub, np.zeros((0, 6), np.float32), 4, flags=F_SOL)[0] == 0       # N == 0
    assert abi_solve(stub, np.zeros((0, TC.n_edges(13)), np.float32), 13, flags=F_SOL, workspace_bytes=0)[0] == 0
    for n in (TC.WS_MIN_N, 14):                                                        # the global tier needs one slot
        c = TC.host("ties", n)[0]
        for wsb in (0, 8, TC.slot_bytes(n) - 8):
            assert abi_solve(stub, c, n, eval_costs=c, workspace_bytes=wsb)[0] == TC.E_INVALID, (n, wsb)
    assert abi_solve(stub, TC.host("ties", 12)[0], 12, flags=F_SOL, workspace_bytes=0)[0] == 0   # the LDS tier needs none


@pytest.mark.parametrize("n", list(TC.SHAPES))
@pytest.mark.parametrize("kind", TC.KINDS)
def test_abi_tours_objectives_and_evals_equal_the_host(stub, kind, n):
    costs, sols, objs, tours = TC.host(kind, n)
    ev = TC.costs_of("signed", len(costs), n, seed=3)
    rc, o = abi_solve(stub, costs, n, eval_costs=ev)
    assert rc == 0
    TC.check_solve(o, sols, objs, tours, n, eval_costs=ev, what=(kind, n))
    rc, o2 = abi_solve(stub, costs, n, eval_costs=ev)   # two launches: the same bytes
    assert rc == 0
    for k in o:
        assert np.array_equal(TC.bits(o[k]), TC.bits(o2[k])), (kind, n, k)
    perm = np.roll(np.arange(len(costs)), 1)[::-1].copy()   # the same instances in another batch order
    rc, o3 = abi_solve(stub, costs[perm], n, eval_costs=ev[perm])
    assert rc == 0
    for k in o:
        assert np.array_equal(TC.bits(o3[k]), TC.bits(o[k][perm])), (kind, n, k, "batch order")


def test_two_slots_five_instances_and_a_batch_of_one(stub):
    """slot reuse and a tail: workgroup 0 takes instances 0, 2, 4 and workgroup 1 instances 1, 3; the default workspace
    (five slots) gives the same bytes; N = 1 in both tiers"""
    n = TC.WS_MIN_N
    costs, sols, objs, tours = TC.host("ties", n, N=5, seed=1)
    rc, o = abi_solve(stub, costs, n, eval_costs=costs, workspace_bytes=2 * TC.slot_bytes(n))
    assert rc == 0
    TC.check_solve(o, sols, objs, tours, n, eval_costs=costs, what="two slots")
    rc, od = abi_solve(stub, costs, n, eval_costs=costs)
    assert rc == 0
    for k in o:
        assert np.array_equal(TC.bits(o[k]), TC.bits(od[k])), k
    for m in (8, n):
        c1 = np.ascontiguousarray(costs[:1, :TC.n_edges(m)])
        rc, o = abi_solve(stub, c1, m, eval_costs=c1)
        s, z, t = TC.tight.tsp_solve(c1[0], m)
        assert rc == 0
        TC.check_solve(o, s[None], np.asarray([z]), np.asarray([t], np.int32), m, eval_costs=c1, what=("N=1", m))


@pytest.mark.parametrize("n", [8, TC.WS_MIN_N])
def test_a_non_finite_cost_fails_its_instance_alone(stub, n):
    import torch

    from cave_amd import tight

    bad, hit, ref = TC.bad_batch(n)
    clean = TC.host("gen", n, N=6, seed=3)[0]
    for wsb in (None, 2 * TC.slot_bytes(n)) if TC.slot_bytes(n) else (None,):   # the bad instance's slot is reused
        rc, o = abi_solve(stub, bad, n, eval_costs=clean, workspace_bytes=wsb)
        assert rc == 0
        TC.check_bad(o, hit, ref, len(bad), what=(n, wsb))
    with pytest.raises(ValueError, match="instance 1"):   # the Python layer refuses the batch
        tight.tsp_solve_hip(torch.tensor(bad, device="cuda"), n)


@pytest.mark.parametrize("n", [4, TC.WS_MIN_N])
def test_every_null_output_combination_leaves_the_others_unchanged(stub, n):
    N = 3
    costs, sols, objs, tours = TC.host("ties", n, N=N, seed=2)
    ev = TC.costs_of("signed", N, n, seed=4)
    rc, full = abi_solve(stub, costs, n, eval_costs=ev)
    assert rc == 0
    TC.check_solve(full, sols, objs, tours, n, eval_costs=ev)
    combos = list(itertools.product((0, 1), repeat=5)) if n == 4 else [(1, 0, 0, 0, 0), (0, 1, 0, 1, 0), (0, 0, 1, 0, 1), (0, 0, 0, 0, 0)]
    for keep in combos:
        flags = sum(f for (_, f), k in zip(EACH, keep) if k)
        for with_ev in (True, False):
            if not with_ev and flags & F_EVAL:
                continue
            rc, o = abi_solve(stub, costs, n, eval_costs=ev if with_ev else None, flags=flags)
            assert rc == 0, (keep, with_ev)
            for k, f in EACH:
                assert (o[k] is None) == (not flags & f)
                if o[k] is not None:
                    assert np.array_equal(TC.bits(o[k]), TC.bits(full[k])), (keep, with_ev, k)


def test_the_integration_stub_prices_tours(stub):
    """INTEGRATION.md section 12's second function as printed: only eval and status are written"""
    import torch

    from cave_amd import _lib

    lib, ns = stub
    n = 8
    pred, _, _, tours = TC.host("gen", n)
    true = TC.costs_of("signed", len(pred), n, seed=3)
    p, t = torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda")
    ev = torch.zeros(len(pred), dtype=torch.float64, device="cuda")
    st = torch.full((len(pred),), -7, dtype=torch.int32, device="cuda")
    ns["tsp_regret_numerators"](lib, p.data_ptr(), t.data_ptr(), len(pred), n, ev.data_ptr(), st.data_ptr(), None, 0, _lib.current_stream())
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all() and np.array_equal(TC.bits(ev.cpu().numpy()), TC.bits(TC.tour_eval(true, tours, n)))
    with pytest.raises(RuntimeError, match="workspace"):
        ns["tsp_regret_numerators"](lib, p.data_ptr(), t.data_ptr(), 1, 13, ev.data_ptr(), st.data_ptr(), None, 0, _lib.current_stream())


@pytest.mark.parametrize("n", [8, TC.LDS_MAX_N, TC.WS_MIN_N])
def test_python_layer(n):
    import torch

    from cave_amd import tight

    costs, sols, objs, tours = TC.host("gen", n)
    ev = TC.costs_of("signed", len(costs), n, seed=3)
    c, e = torch.tensor(costs, device="cuda"), torch.tensor(ev, device="cuda")
    s, z, t = tight.tsp_solve_hip(c, n)
    s2, z2, t2, v = tight.tsp_solve_hip(c, n, eval_costs=e)
    assert s.dtype == torch.float32 and z.dtype == torch.float64 and t.dtype == torch.int32
    assert torch.equal(s, s2) and torch.equal(z, z2) and torch.equal(t, t2)
    TC.check_solve({"sol": s.cpu().numpy(), "obj": z.cpu().numpy(), "tour": t.cpu().numpy(), "eval": v.cpu().numpy()}, sols, objs, tours, n,
                   eval_costs=ev)
    empty = tight.tsp_solve_hip(c[:0], n)
    assert empty[0].shape == (0, TC.n_edges(n)) and empty[2].shape == (0, n)
    with pytest.raises(ValueError):
        tight.tsp_solve_hip(c.cpu(), n)                       # device
    with pytest.raises(ValueError):
        tight.tsp_solve_hip(c.double(), n)                    # dtype
    with pytest.raises(ValueError):
        tight.tsp_solve_hip(c[:, :-1], n)                     # shape
    with pytest.raises(ValueError):
        tight.tsp_solve_hip(c, n, eval_costs=e[:-1])          # eval_costs shape
    for bad_n in (2, 15):
        with pytest.raises(ValueError):
            tight.tsp_solve_hip(torch.ones(1, TC.n_edges(bad_n), device="cuda"), bad_n)


def test_device_regret_matches_the_host():
    """condition 7, at n = 8, N = 32: random predictions against true costs and their true objectives"""
    import torch

    from cave_amd import tight

    n, N = 8, 32
    true, _, z, _ = (np.array(a) for a in TC.host("gen", n, N=N, seed=6))   # (writable copies: they become tensors)
    pred = (true * np.random.default_rng(5).uniform(0.3, 3.0, true.shape)).astype(np.float32)
    z32 = z.astype(np.float32)
    host = tight.tsp_regret(pred, true, z32, n)
    psols = np.stack([tight.tsp_solve(p, n)[0] for p in pred])
    bound = TC.regret_bound(true, psols, z32, n)
    dev = tight.tsp_regret(pred, true, z32, n, device="cuda")
    print(f"regret n={n} N={N}: host {host!r} device {dev!r} |diff| {abs(dev - host):.3e} bound {bound:.3e}")
    assert abs(dev - host) <= bound
    on_dev = tight.tsp_regret(torch.tensor(pred, device="cuda"), torch.tensor(true, device="cuda"), torch.tensor(z32, device="cuda"),
                              n, device="cuda")
    assert on_dev == dev


def _example(argv):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train_sp_cave

    return train_sp_cave.main(argv)


def test_training_example_device_regret_matches_host_regret():
    """condition 8: the same losses; regrets within condition 7's bound -- tsp_gen_data costs are positive, so
    sum_i c_i . w(c_hat_i) / sum_i |z_i| = 1 + regret and the bound is n 2^-23 (1 + regret)"""
    n = 8
    base = ["--problem", "tsp", "--nodes", str(n), "--num-data", "48", "--epochs", "2", "--packed"]
    host, dev = _example(base), _example(base + ["--device-regret"])
    assert len(host) == len(dev) == 3
    for (e0, l0, r0), (e1, l1, r1) in zip(host, dev):
        print(f"epoch {e0}: loss {l0!r} / {l1!r}  regret {r0!r} / {r1!r}")
        assert e0 == e1 and (l0 == l1 or e0 == 0)
        assert abs(r0 - r1) <= n * 2.0 ** -23 * (1.0 + r0), (e0, r0, r1)


def test_training_example_device_regret_shortest_path():
    hist = _example(["--problem", "sp", "--grid", "5", "5", "--num-data", "48", "--epochs", "2", "--packed", "--device-regret"])
    assert len(hist) == 3 and all(np.isfinite(x[2]) for x in hist) and all(np.isfinite(x[1]) for x in hist[1:])
