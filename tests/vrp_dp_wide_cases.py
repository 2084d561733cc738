"""Cases of the wide CVRP tier (cave_amd/csrc/vrp_dp_wide.h, 13 <= n <= 20), shared by the CPU tier
(tests/test_vrp_dp_wide_emul.py: the kernels under the SIMT emulation) and the GPU tier (tests/test_gpu_vrp_dp_wide.py).

Oracles.  Up to n = 14 the project's own host code, tight.vrp_solve (tests/vrp_dp_cases.py `host`).  Beyond it the host
solver refuses, so `solve_ref` restates tight._vrp_tables / tight.vrp_solve in numpy for any n:
  * the Held-Karp table is tsp_hk_wide_cases.solve_ref's, vectorised by cardinality (`hk_table`: the same additions, +inf
    for k outside the set, np.argmin's first minimum), in tight._held_karp's layout, so tight._hk_walk walks it;
  * load(S), the popcount, the feasibility test and r(S) are tight._vrp_tables' own statements;
  * a stored layer g_k (k < K') is needed as VALUES only: g_k(S) = min over R of r(R) + g_{k-1}(S \\ R).  Every candidate is
    one fp64 addition of two table entries, each finite or +inf (never -inf, never NaN), and the minimum of a set of such
    numbers does not depend on the order they are taken in.  So the values are computed by a min-plus subset convolution
    (`_layer`: the sets that share their lowest customer are split on their highest bit, recursively, 3^m additions in all
    in numpy-sized pieces) over exactly the host's candidates plus pairs whose one side is +inf;
  * where the ORDER matters -- the argmin of g_k(S) on the walk back, and g_k(full) -- the candidates R are listed in
    ascending numeric order as the host lists them and np.argmin takes the first minimum;
  * the objective is the first minimum over k, the routes are walked back as tight.vrp_solve walks them.
tests/test_vrp_dp_wide_emul.py asserts it equal to tight.vrp_solve bit for bit at n <= 12 over the three kinds.

For n = 18 and 20 (0.8 s per instance at n = 18, K = 3; 0.5 s at n = 20, K = 2; 6 s at n = 20, K = 3 with its stored
layer) the results are kept in tests/golden/vrp_dp_wide.npz, written by tests/golden/make_vrp_dp_wide.py: per (n, K) in GOLDEN_SHAPES
one `gen`, one `ties` and one `signed` instance (costs, demands, capacities, routes, objectives), and the objective
tight.vrp_rcc_cuts (HiGHS, another algorithm) finds for the `gen` instance of GOLDEN_RCC: n = 20 at K = 3, the largest
fixture size (the loop ends within a second there).

Instances: vrp_dp_cases.instance_of, kinds gen / ties / signed.  Every generated instance is feasible (asserted where the
case is built; nothing is left out); infeasibility enters through `infeasible_calls` only.

Bounds: vrp_dp_cases' own -- sols, objs, routes and evals EQUAL (bit comparison), the regret within `regret_bound`.
"""

from __future__ import annotations

import os

import numpy as np

import vrp_dp_cases as VC
from cave_amd import tight

E_INVALID = VC.E_INVALID
MIN_N, MAX_N, MAX_K = 13, 20, 8
MAX_SLOTS, MAX_BYTES = 512, 8 << 30
KINDS = VC.KINDS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vrp_dp_wide.npz")
GOLDEN_SHAPES = ((18, 3), (20, 2), (20, 3))
GOLDEN_RCC = (20, 3)  # the largest fixture size: the cut loop finishes its `gen` instance within seconds (n = 20)
HOST_MAX_N = 14

# (n, K) -> batch size: the table of the issue.  13/3 and 13/6: the lower edge, byte-equal with the first entry (its tiers
# 1 and 2); 14/2: no stored layer; 14/3: the host's last size; 15/1: one route, the capacity decides; 15/3: the first size
# beyond the host; 16/4: two stored layers; 17/3: class offsets reach 2^16; 18/3, 20/2, 20/3: the fixture
SHAPES = {(13, 3): 3, (13, 6): 2, (14, 2): 2, (14, 3): 2, (15, 1): 3, (15, 3): 3, (16, 4): 2, (17, 3): 2, (18, 3): 3, (20, 2): 3,
          (20, 3): 3}


def valid(n, K):
    return MIN_N <= n <= MAX_N and 1 <= K <= MAX_K


def header_bytes(n):
    """the popcount-sorted list of the (n-1)-bit numbers, uint32"""
    return 4 * 2 ** (n - 1)


def slot_bytes(n, K):
    """include/cave_hip.h: the Held-Karp table, (n-1) 2^(n-2) doubles, then r and the stored layers, (K' - 1) 2^(n-1)
    doubles; -1 for an n or K out of range"""
    return VC.hk_bytes(n) + VC.part_bytes(n, K) if valid(n, K) else E_INVALID


def default_slots(n, K):
    return min(MAX_SLOTS, MAX_BYTES // slot_bytes(n, K))


def workspace_bytes(n, K, N):
    if not valid(n, K) or N < 0:
        return E_INVALID
    return header_bytes(n) + slot_bytes(n, K) * min(N, default_slots(n, K))


def lds_bytes(n):
    """cave_amd/csrc/vrp_dp_wide.h: D, the customers' block of D with an odd row stride, cand / priced edges / demands
    [32] f64, g_k(full) [16] f64, the reduction's 512 values and 512 indices, the class offsets, the state, the route list,
    the staged costs, the solution -- each rounded up to 16 bytes"""
    r16, m, d = VC._r16, n - 1, VC.n_edges(n)
    return r16(8 * n * n) + r16(8 * m * (m | 1)) + 3 * 256 + 128 + 8 * 512 + 4 * 512 + 128 + 64 + 128 + 2 * r16(4 * d)


def hk_table(cost, n):
    """tsp_hk_wide_cases.solve_ref's table in tight._held_karp's layout -> (D, dp [2^m, m], parent [2^m, m])"""
    m = n - 1
    iu = np.triu_indices(n, 1)  # lexicographic (i < j): the edge order
    D = np.zeros((n, n))
    D[iu] = np.asarray(cost, dtype=np.float64)
    D = D + D.T
    Dm = D[1:, 1:]
    full = 1 << m
    sets = np.arange(full, dtype=np.int64)
    pop = np.zeros(full, dtype=np.int64)
    for j in range(m):
        pop += sets >> j & 1
    dp = np.full((full, m), np.inf)
    parent = np.full((full, m), -1, dtype=np.int64)
    for j in range(m):
        dp[1 << j, j] = D[0, j + 1]
    for c in range(2, m + 1):
        S = sets[pop == c]
        for j in range(m):
            Sj = S[(S >> j & 1) == 1]
            cand = dp[Sj ^ (1 << j)] + Dm[:, j][None, :]  # [sets, k]; +inf where k is not in the predecessor set
            k = np.argmin(cand, axis=1)
            dp[Sj, j] = cand[np.arange(len(Sj)), k]
            parent[Sj, j] = k
    return D, dp, parent


def _minplus(A, B):
    """C[.., T] = min over sub a subset of T of A[.., sub] + B[.., T \\ sub], the last axis indexed by the subsets of b bits:
    split on the highest bit (it lies in sub, in T \\ sub, or in neither), the three subproblems stacked along axis 0"""
    h = A.shape[-1] // 2
    if h == 0:
        return A + B
    if A.shape[0] * 3 ** h.bit_length() > 1 << 25:  # the stacked pieces grow to batch 3^bits doubles: keep them small
        lo = _minplus(A[:, :h], B[:, :h])
        hi = np.minimum(_minplus(A[:, h:], B[:, :h]), _minplus(A[:, :h], B[:, h:]))
        return np.concatenate([lo, hi], axis=-1)
    Z = _minplus(np.concatenate([A[:, :h], A[:, h:], A[:, :h]]), np.concatenate([B[:, :h], B[:, :h], B[:, h:]]))
    z = Z.reshape(3, A.shape[0], h)
    return np.concatenate([z[0], np.minimum(z[1], z[2])], axis=-1)


def _layer(r, prev, m, k, pc):
    """the values of g_k over all sets: per lowest customer l, the sets S = 2^l | T 2^(l+1) and their candidates
    R = 2^l | sub 2^(l+1), sub over ALL subsets of T.  sub = T (R = S) adds the pair r(S) + prev(0) = +inf, which changes
    no minimum; sets of fewer than 2 k customers are +inf, as the host leaves them"""
    g = np.full(1 << m, np.inf)
    for l in range(m - 1):
        b = m - l - 1
        T = np.arange(1 << b, dtype=np.int64) << (l + 1)
        g[T | (1 << l)] = _minplus(r[T | (1 << l)][None, :], prev[T][None, :])[0]
    g[pc < 2 * k] = np.inf
    return g


def _candidates(S):
    """the proper subsets of S that hold its lowest bit, in ascending order (tight._vrp_tables' list)"""
    low = S & -S
    subs = np.zeros(1, dtype=np.int64)
    rest = S ^ low
    while rest:
        b = rest & -rest
        rest ^= b
        subs = np.concatenate([subs, subs | b])
    return (subs | low)[:-1]


def solve_ref(cost, n, demands, capacity, num_vehicle):
    """tight.vrp_solve for any n -> (sol (d,) float32, objective, routes); raises ValueError where it would"""
    m = n - 1
    full = 1 << m
    D, dp, parent = hk_table(cost, n)
    q = np.asarray(demands).reshape(-1)
    assert len(q) == m
    load = np.zeros(full)  # the fp64 sum of q_j over j in S, ascending j, from 0.0 -- the highest bit is added last
    for j in range(m):
        load[1 << j:2 << j] = load[:1 << j] + np.float64(q[j])
    pc = np.zeros(full, dtype=np.int64)
    for j in range(m):
        pc[1 << j:2 << j] = pc[:1 << j] + 1
    feas = (pc >= 2) & (load <= capacity)
    closed = dp + D[1:, 0][None, :]  # +inf where j is not in S
    r = np.where(feas, closed[np.arange(full), np.argmin(closed, axis=1)], np.inf)  # first minimum over j, ascending
    kmax = min(int(num_vehicle), m // 2)
    layers = [None, r]
    for k in range(2, kmax):  # the stored layers; layer K' is read at the full set only
        layers.append(_layer(r, layers[k - 1], m, k, pc))

    def split(S, k):  # g_k(S) and its argmin: the host's candidates in the host's order, first minimum
        R = _candidates(S)
        val = r[R] + layers[k - 1][S ^ R]
        i = int(np.argmin(val))
        return val[i], int(R[i])

    best, obj = 0, np.inf
    for k in range(1, kmax + 1):
        v = r[full - 1] if k == 1 else split(full - 1, k)[0]
        if k >= 2 and k < kmax:
            assert v == layers[k][full - 1] or (np.isinf(v) and np.isinf(layers[k][full - 1]))  # the two ways agree
        if v < obj:  # strict: the fewest routes win a tie
            best, obj = k, v
    if best == 0:
        raise ValueError("vrp_solve: the instance is infeasible (no partition into feasible routes)")
    routes, S = [], full - 1
    for k in range(best, 0, -1):
        R = split(S, k)[1] if k > 1 else S
        routes.append([0] + tight._hk_walk(D, dp, parent, R)[1][::-1] + [0])
        S ^= R
    sol = np.zeros(VC.n_edges(n), dtype=np.float32)
    for rt in routes:
        for a, b in zip(rt, rt[1:]):
            sol[VC.eid(a, b, n)] = 1.0
    return sol, float(obj), routes


def sols_of(routes, n):
    """0/1 edge indicators of padded route lists"""
    s = np.zeros((len(routes), VC.n_edges(n)), np.float32)
    for b, t in enumerate(routes):
        t = [int(v) for v in t if v >= 0]
        for a, c in zip(t, t[1:]):
            s[b, VC.eid(a, c, n)] = 1.0
    return s


def check_instance(kind, q, cap, n):
    """what vrp_dp_cases.host asserts of a `ties` case: some load equals the capacity exactly, so the `<=` decides"""
    if kind == "ties":
        load = np.zeros(1 << (n - 1))
        for j in range(n - 1):
            load[1 << j:2 << j] = load[:1 << j] + np.float64(q[j])
        assert (load == cap).any(), (n, q, cap)


_REF = {}


def ref(kind, n, K, N=None, seed=0):
    """(costs, demands, capacity, sols, objs, routes) of the oracle for vrp_dp_cases.instance_of(kind, N, n, K, seed),
    cached: tight.vrp_solve up to n = 14, `solve_ref` beyond.  An infeasible instance raises: none may be."""
    N = SHAPES[(n, K)] if N is None else N
    if n <= HOST_MAX_N:
        return VC.host(kind, n, K, N=N, seed=seed)
    k = (kind, n, K, N, seed)
    if k not in _REF:
        c, q, cap = VC.instance_of(kind, N, n, K, seed)
        res = [solve_ref(ci, n, q, cap, K) for ci in c]
        objs = np.asarray([o for _, o, _ in res], np.float64)
        assert np.isfinite(objs).all()
        check_instance(kind, q, cap, n)
        _REF[k] = (c, q, cap, np.stack([s for s, _, _ in res]), objs, np.stack([VC.pad_routes(t, n, K) for _, _, t in res]))
        for a in (c, q) + _REF[k][3:]:
            a.setflags(write=False)
    return _REF[k]


def golden_instances(n, K):
    """the fixture's three instances of (n, K), one per kind in KINDS order -> [(cost row, demands, capacity)]"""
    return [(lambda c, q, cap: (c[0], q, cap))(*VC.instance_of(kind, 1, n, K, seed=5)) for kind in KINDS]


_GOLD = {}


def golden(n, K):
    """(costs [3, d], demands [3, m], capacities [3], sols, objs, routes [3, n + K]) of the committed fixture"""
    if (n, K) not in _GOLD:
        t = f"{n}_{K}"
        with np.load(GOLDEN) as z:
            c, q, cap, o, rt = z["costs" + t], z["demands" + t], z["caps" + t], z["objs" + t], z["routes" + t]
        assert c.dtype == np.float32 and c.shape == (3, VC.n_edges(n)) and q.dtype == np.float32 and q.shape == (3, n - 1)
        assert cap.dtype == np.float64 and o.dtype == np.float64 and rt.dtype == np.int32 and rt.shape == (3, n + K)
        for i, (ci, qi, capi) in enumerate(golden_instances(n, K)):  # the fixture is of the instances this module draws
            assert np.array_equal(c[i], ci) and np.array_equal(q[i], qi) and cap[i] == capi, (n, K, i)
        _GOLD[(n, K)] = (c, q, cap, sols_of(rt, n), o, rt)
        for a in _GOLD[(n, K)]:
            a.setflags(write=False)
    return _GOLD[(n, K)]


def golden_rcc():
    """the objective tight.vrp_rcc_cuts found for the `gen` instance (row 0) of GOLDEN_RCC"""
    with np.load(GOLDEN) as z:
        return float(z["rcc%d_%d" % GOLDEN_RCC])


def bad_batch(n, K, N=5):
    """good `gen` instances with a NaN in instance 1 and an inf in instance 4 -> (costs, bad ids, the clean batch's case)"""
    case = ref("gen", n, K, N=N, seed=3)
    bad = case[0].copy()
    bad[1, VC.n_edges(n) - 1] = np.nan
    bad[4, 0] = np.inf
    return bad, (1, 4), case


def infeasible_calls(n=15, K=3):
    """vrp_dp_cases.infeasible_calls at a size of this tier -> a list of (costs, demands, capacity, K, expected), expected
    being None (every instance infeasible) or the reference results.  A feasible batch of three; its instance 1 again in a
    call of its own with a demand pattern that breaks the capacity (one customer alone exceeds it); the instances 0 and 2
    beside it in their own call, unaffected; and the batch with K = 1 and a capacity below the total load."""
    c, q, cap, sols, objs, routes = ref("gen", n, K, N=3, seed=5)
    broken = q.copy()
    broken[2] = np.float32(cap + 1.0)
    low = float(np.floor(float(q.astype(np.float64).sum()))) - 1.0
    calls = [(c, q, cap, K, (sols, objs, routes)),
             (c[1:2], broken, cap, K, None),
             (c[[0, 2]], q, cap, K, (sols[[0, 2]], objs[[0, 2]], routes[[0, 2]])),
             (c, q, low, 1, None)]
    # designed to be infeasible, by the model's own rules: a customer whose demand exceeds the capacity fits no route;
    # one route must carry the total load
    assert np.float64(broken[2]) > cap and q.astype(np.float64).sum() > low
    return calls
