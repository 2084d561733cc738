"""Cases of the CVRP dynamic-program kernels (cave_amd/csrc/vrp_dp.h), shared by the CPU tier (tests/test_vrp_dp_emul.py:
the kernels under the SIMT emulation) and the GPU tier (tests/test_gpu_vrp_dp.py).

The oracle is the project's own host code, tight.vrp_solve.  Host results are computed once per case and shared.

Bounds (derived, not measured):
  * objs, routes and sols: EQUAL.  The device performs the host's fp64 additions and strict comparisons in the host's
    candidate order; where the candidates of one set are spread over threads the (value, index) reduction is the
    first-minimum rule; the sets of one layer are independent, so no other order shows.
  * evals: EQUAL to the fp64 sum, from 0.0, of eval_costs over the routes' edges, route by route in route order, each
    route from the depot out and back (`routes_eval`): the device performs exactly these additions.
  * vrp_regret(device=) against the host's: (n + K) 2^-23 sum_i sum_k |c_ik| sol_ik / sum_i |z_i| (`regret_bound`):
    tsp_hk_cases.regret_bound's derivation with the number of selected edges, at most n - 1 + K, in place of n (the host
    prices with a float32 dot product: one rounding of at most 2^-24 of a partial sum per non-zero term, a factor two of
    margin; float(z) and the fp64 sums on either side round below 2^-50 of it).

Every generated instance is feasible (asserted on the host where the case is built; nothing is left out).
Infeasibility enters through `infeasible_calls` only.
"""

from __future__ import annotations

import numpy as np

from cave_amd import tight

ST_OK, ST_BAD_INPUT, ST_INFEASIBLE = 0, 3, 4
E_INVALID = -1
MAX_LDS = 160 * 1024
DEFAULT_SLOTS = 512
MAX_K = 8


def n_edges(n):
    return n * (n - 1) // 2


def eid(i, j, n):
    i, j = min(i, j), max(i, j)
    return i * n - i * (i + 1) // 2 + j - i - 1


def _r16(x):
    return (x + 15) & ~15


def valid(n, K):
    return 3 <= n <= 14 and 1 <= K <= MAX_K


def kmax(n, K):
    return min(K, (n - 1) // 2)


def hk_bytes(n):
    """(n-1) 2^(n-2) doubles: the Held-Karp entries (S, j) with j in S"""
    return 8 * (n - 1) * 2 ** (n - 2)


def part_bytes(n, K):
    """r and the stored layers g_2 .. g_{K'-1}: (K' - 1) 2^(n-1) doubles"""
    return 8 * (kmax(n, K) - 1) * 2 ** (n - 1)


def _fixed_lds(n):
    """D, cand [16] f64, priced edges [32] f64, demands [16] f64, g_k(full) [16] f64, the reduction's 256 values and 256
    indices, the binomials, the class offsets, state [16] i32, the route list [32] i32, the staged costs, the solution,
    the popcount-sorted list -- each rounded up to 16 bytes (cave_amd/csrc/vrp_dp.h)"""
    d = n_edges(n)
    return (_r16(8 * n * n) + 128 + 256 + 128 + 128 + 8 * 256 + 4 * 256 + _r16(2 * 14 * 14) + 32 + 64 + 128 + 2 * _r16(4 * d)
            + _r16(2 * 2 ** (n - 2)))


def tier(n, K):
    """0: both tables in LDS; 1: the Held-Karp table in the workspace slot; 2: both in the slot"""
    if _fixed_lds(n) + hk_bytes(n) + part_bytes(n, K) <= MAX_LDS:
        return 0
    return 1 if _fixed_lds(n) + part_bytes(n, K) <= MAX_LDS else 2


def slot_bytes(n, K):
    """include/cave_hip.h: the bytes of the tables that do not lie in LDS; -1 for an n or K out of range"""
    if not valid(n, K):
        return E_INVALID
    t = tier(n, K)
    return (hk_bytes(n) if t >= 1 else 0) + (part_bytes(n, K) if t == 2 else 0)


def lds_bytes(n, K):
    t = tier(n, K)
    return _fixed_lds(n) + (hk_bytes(n) if t == 0 else 0) + (part_bytes(n, K) if t <= 1 else 0)


def workspace_bytes(n, K, N):
    if not valid(n, K) or N < 0:
        return E_INVALID
    return slot_bytes(n, K) * min(N, DEFAULT_SLOTS)


LDS_MAX_N = max(n for n in range(3, 15) if slot_bytes(n, 3) == 0)   # the largest n whose slot size is 0 at K = 3
WS_MIN_N = LDS_MAX_N + 1

# (n, K) -> batch size.  m = 2 (one route); m = 3 (K' clamps to 1); the first real split; 2^m below / equal to the
# workgroup size; the reference test's CVRP-9; the last size with all tables in LDS and the first with a slot (tier 1);
# the cap; and one shape whose partition tables lie in the slot too (tier 2)
SHAPES = {(3, 1): 5, (4, 2): 5, (5, 2): 5, (6, 3): 5, (8, 3): 5, (9, 3): 5, (10, 3): 5, (LDS_MAX_N, 3): 3, (WS_MIN_N, 3): 3,
          (14, 2): 2, (13, 6): 2}
KINDS = ("gen", "ties", "signed")


def instance_of(kind, N, n, K, seed=0):
    """-> (costs (N, d) float32, demands (n-1,) float32, capacity)"""
    d, m, km = n_edges(n), n - 1, kmax(n, K)
    rng = np.random.default_rng(100 * n + 7919 * seed + 17 * K + 1)
    if kind == "gen":  # the data generator's draws; the reference test's capacity at its shape, else a binding one
        _, c, q = tight.vrp_gen_data(N, 5, n, seed=42 + seed)
        cap = 30.0 if (n, K) == (10, 3) else float(np.ceil(1.3 * float(q.sum()) / km + 5.0))
        return c, q, cap
    if kind == "ties":  # costs from {1, 2, 3}, integer demands: tied minima everywhere, loads that equal the capacity
        c = rng.integers(1, 4, (N, d)).astype(np.float32)
        q = rng.integers(1, 5, m).astype(np.float32)
        # (one route: the capacity IS the total load, so `<=` decides feasibility itself)
        cap = float(max(int(np.ceil(q.sum() / km)) + (1 if km > 1 else 0), int(np.sort(q)[-2:].sum())))
        return c, q, cap
    if kind == "signed":  # both signs: more routes can be cheaper, k* and a binding K decide; the capacity is loose
        c = rng.standard_normal((N, d)).astype(np.float32)
        c[: N // 3] = -np.abs(c[: N // 3])
        q = (rng.random(m) * 10).astype(np.float32)
        return c, q, float(np.ceil(q.sum()))
    raise KeyError(kind)


def pad_routes(routes, n, K):
    flat = [0]
    for r in routes:
        flat += r[1:]
    return np.asarray(flat + [-1] * (n + K - len(flat)), np.int32)


def solve_host(costs, n, q, cap, K):
    """tight.vrp_solve over a batch -> (sols, objs, routes [N, n + K] int32); an infeasible instance raises"""
    r = [tight.vrp_solve(c, n, q, cap, K) for c in costs]
    return (np.stack([s for s, _, _ in r]), np.asarray([o for _, o, _ in r], np.float64),
            np.stack([pad_routes(t, n, K) for _, _, t in r]))


_HOST = {}


def host(kind, n, K, N=None, seed=0):
    """(costs, demands, capacity, sols, objs, routes) of the host solver, cached"""
    N = SHAPES[(n, K)] if N is None else N
    k = (kind, n, K, N, seed)
    if k not in _HOST:
        c, q, cap = instance_of(kind, N, n, K, seed)
        sols, objs, routes = solve_host(c, n, q, cap, K)   # raises if an instance is infeasible: none may be
        assert np.isfinite(objs).all()
        if kind == "ties":  # some load equals the capacity exactly: the `<=` decides
            load = np.zeros(1 << (n - 1))
            for j in range(n - 1):
                load[1 << j:2 << j] = load[:1 << j] + np.float64(q[j])
            assert (load == cap).any(), (n, K, q, cap)
        _HOST[k] = (c, q, cap, sols, objs, routes)
        for a in (c, q, sols, objs, routes):
            a.setflags(write=False)
    return _HOST[k]


def routes_eval(eval_costs, routes, n):
    """the fp64 sum, from 0.0, of eval_costs over the edges of the route list in its order"""
    out = np.empty(len(routes), np.float64)
    for b, t in enumerate(routes):
        t = [int(v) for v in t if v >= 0]
        acc = np.float64(0.0)
        for a, c in zip(t, t[1:]):
            acc = acc + np.float64(eval_costs[b, eid(a, c, n)])
        out[b] = acc
    return out


def regret_bound(true, psols, z, n, K):
    return (n + K) * 2.0 ** -23 * (np.abs(true.astype(np.float64)) * psols).sum() / np.abs(z.astype(np.float64)).sum()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_solve(o, sols, objs, routes, n, eval_costs=None, what=""):
    """a batch of device outputs (dict of numpy arrays; None entries were not requested) against the host's, bit for bit"""
    if o.get("status") is not None:
        assert o["status"].dtype == np.int32 and (o["status"] == ST_OK).all(), (what, o["status"])
    if o.get("sol") is not None:
        assert o["sol"].dtype == np.float32 and np.array_equal(bits(o["sol"]), bits(sols)), (what, "sol")
    if o.get("obj") is not None:
        assert o["obj"].dtype == np.float64 and np.array_equal(bits(o["obj"]), bits(objs)), (what, "obj", o["obj"], objs)
    if o.get("routes") is not None:
        assert o["routes"].dtype == np.int32 and np.array_equal(o["routes"], routes), (what, "routes", o["routes"], routes)
    if o.get("eval") is not None:
        ref = routes_eval(eval_costs, routes, n)
        assert o["eval"].dtype == np.float64 and np.array_equal(bits(o["eval"]), bits(ref)), (what, "eval", o["eval"], ref)


def check_failed(o, st, what=""):
    """every instance of the batch failed with status `st`: zero sol, NaN obj and eval, routes of -1"""
    assert (o["status"] == st).all(), (what, o["status"])
    assert (o["sol"] == 0).all() and np.isnan(o["obj"]).all() and (o["routes"] == -1).all(), what
    if o.get("eval") is not None:
        assert np.isnan(o["eval"]).all(), what


def bad_batch(n, K, N=5):
    """good `gen` instances with a NaN in instance 1 and an inf in instance 4 -> (costs, bad ids, the clean batch's host case)"""
    case = host("gen", n, K, N=N, seed=3)
    bad = case[0].copy()
    bad[1, n_edges(n) - 1] = np.nan
    bad[4, 0] = np.inf
    return bad, (1, 4), case


def check_bad(o, hit, case, what=""):
    _, _, _, sols, objs, routes = case
    ok = np.ones(len(sols), bool)
    ok[list(hit)] = False
    assert (o["status"][~ok] == ST_BAD_INPUT).all() and (o["status"][ok] == ST_OK).all(), (what, o["status"])
    assert (o["sol"][~ok] == 0).all() and np.isnan(o["obj"][~ok]).all() and np.isnan(o["eval"][~ok]).all(), what
    assert (o["routes"][~ok] == -1).all(), what
    assert np.array_equal(o["sol"][ok], sols[ok]) and np.array_equal(bits(o["obj"][ok]), bits(objs[ok])), what
    assert np.array_equal(o["routes"][ok], routes[ok]), what


def infeasible_calls(n=8, K=3):
    """The designed infeasible batch -> a list of (costs, demands, capacity, K, expected), expected being None (every
    instance infeasible; the host raises too) or the host results.  A feasible batch of three; its instance 1 again in a
    call of its own with a demand pattern that breaks the capacity (one customer alone exceeds it); the instances 0 and 2
    beside it in their own call, unaffected; and the batch with K = 1 and a capacity below the total load."""
    c, q, cap, sols, objs, routes = host("gen", n, K, N=3, seed=5)
    broken = q.copy()
    broken[2] = np.float32(cap + 1.0)
    low = float(np.floor(float(q.astype(np.float64).sum()))) - 1.0
    calls = [(c, q, cap, K, (sols, objs, routes)),
             (c[1:2], broken, cap, K, None),
             (c[[0, 2]], q, cap, K, (sols[[0, 2]], objs[[0, 2]], routes[[0, 2]])),
             (c, q, low, 1, None)]
    for cc, qq, cp, kk, want in calls:   # the host agrees on which calls are infeasible
        if want is None:
            for ci in cc:
                try:
                    tight.vrp_solve(ci, n, qq, cp, kk)
                except ValueError:
                    continue
                raise AssertionError("designed to be infeasible")
    return calls
