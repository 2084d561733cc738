"""CPU tier: the host CVRP layer of cave_amd/tight.py -- the dynamic program `vrp_solve` (the definition the device
reproduces), the rounded-capacity cutting loop `vrp_rcc_cuts`, `vrp_tight_normals`, `vrp_gen_data`, `VRPConeDataset` and
`vrp_regret`.

  1. vrp_solve against brute force (all partitions x all orders) for n <= 7, a binding and a loose capacity, cases where
     both agree on infeasible included: objectives within 2 E 2^-52 sum |c| (two fp64 sums of the same E <= n - 1 + K
     terms in different orders), and vrp_solve's own routes are feasible and priced at its objective
  2. K = 1 with infinite capacity equals tsp_solve bit for bit
  3. the feasibility checks of the reference's testCVRPSolver restated, at n = 10 (its draw: capacity 30, 3 vehicles)
  4. the cut loop's objective equals the dynamic program's within 2 E 2^-52 sum_k |c_k| sol_k, E the selected edges
  5. vrp_tight_normals: row order, every row tight at sol; shapes through VRPConeDataset."""

import itertools

import numpy as np
import pytest

from cave_amd import tight


def _brute(cost, n, q, Q, K):
    """min over all partitions into at most K sets of >= 2 customers with load <= Q, each set in its best order"""
    m = n - 1
    _, eid = tight._edge_index(n)
    rc = {}
    for S in range(1, 1 << m):
        R = [j + 1 for j in range(m) if S >> j & 1]
        if len(R) >= 2 and sum(float(q[j - 1]) for j in R) <= Q:
            best = np.inf
            for p in itertools.permutations(R):
                if p[0] > p[-1]:
                    continue  # a route and its reverse cost the same
                t = [0] + list(p) + [0]
                best = min(best, sum(float(cost[eid[a, b]]) for a, b in zip(t, t[1:])))
            rc[S] = best

    def rec(S, k):
        if S == 0:
            return 0.0
        if k == 0:
            return np.inf
        low = S & -S
        return min([rc[R] + rec(S ^ R, k - 1) for R in rc if R & low and (R & S) == R], default=np.inf)

    return rec((1 << m) - 1, K)


def _check_feasible(sol, routes, n, q, Q, K):
    """the reference test's checks (test/test_optmodel.py testCVRPSolver), on the edge indicator and on the routes"""
    edges, _ = tight._edge_index(n)
    act = [(int(a), int(b)) for (a, b), s in zip(edges, sol) if s > 1e-2]
    deg = np.zeros(n, int)
    for a, b in act:
        deg[a] += 1
        deg[b] += 1
    assert (deg[1:] == 2).all()                      # every customer visited exactly once
    assert deg[0] <= 2 * K and deg[0] == 2 * len(routes)   # the number of vehicles
    adj = {v: set() for v in range(n)}               # no subtour: every customer connected to the depot
    for a, b in act:
        adj[a].add(b)
        adj[b].add(a)
    seen, todo = {0}, [0]
    while todo:
        for w in adj[todo.pop()]:
            if w not in seen:
                seen.add(w)
                todo.append(w)
    assert len(seen) == n
    assert sorted(v for r in routes for v in r[1:-1]) == list(range(1, n))
    for r in routes:                                 # loads, and the shape of a route
        assert r[0] == 0 and r[-1] == 0 and len(r) >= 4
        assert sum(float(q[v - 1]) for v in r[1:-1]) <= Q
    assert [min(r[1:-1]) for r in routes] == sorted(min(r[1:-1]) for r in routes)   # in order of their lowest customer


@pytest.mark.parametrize("n", [3, 4, 5, 6, 7])
def test_vrp_solve_against_brute_force(n):
    rng = np.random.default_rng(n)
    d, feasible, infeasible = n * (n - 1) // 2, 0, 0
    for trial in range(4):
        q = (rng.random(n - 1) * 10).astype(np.float32)
        cost = (rng.standard_normal(d) if trial % 2 else rng.random(d)).astype(np.float32)
        for Q in (12.0, float(np.ceil(q.sum()))):   # binding, loose
            for K in (1, 2, 3):
                want = _brute(cost, n, q, Q, K)
                if want == np.inf:
                    with pytest.raises(ValueError):
                        tight.vrp_solve(cost, n, q, Q, K)
                    infeasible += 1
                    continue
                sol, obj, routes = tight.vrp_solve(cost, n, q, Q, K)
                E = int(sol.sum())
                tol = 2 * E * 2.0 ** -52 * float(np.abs(cost.astype(np.float64)).sum())
                assert abs(obj - want) <= tol, (n, Q, K, obj, want)
                assert abs(float(cost.astype(np.float64) @ sol) - obj) <= tol
                _check_feasible(sol, routes, n, q, Q, K)
                feasible += 1
    assert feasible and (infeasible or n == 3)


@pytest.mark.parametrize("n", [3, 6, 9])
def test_one_vehicle_and_infinite_capacity_is_tsp_solve(n):
    rng = np.random.default_rng(10 + n)
    for cost in (rng.random(n * (n - 1) // 2).astype(np.float32), rng.integers(1, 4, n * (n - 1) // 2).astype(np.float32)):
        sol, obj, routes = tight.vrp_solve(cost, n, np.ones(n - 1), np.inf, 1)
        s2, o2, tour = tight.tsp_solve(cost, n)
        assert np.array_equal(sol, s2) and np.float64(obj).tobytes() == np.float64(o2).tobytes() and routes == [tour + [0]]


def test_tie_rules():
    """equal costs: the fewest routes win, and the route of the lowest customer is the numerically smallest set"""
    n = 7
    cost = np.zeros(n * (n - 1) // 2, np.float32)
    q = np.ones(n - 1, np.float32)
    _, obj, routes = tight.vrp_solve(cost, n, q, 6.0, 3)
    assert obj == 0.0 and len(routes) == 1
    _, obj, routes = tight.vrp_solve(cost, n, q, 3.0, 3)          # a load equal to the capacity is feasible
    assert obj == 0.0 and [sorted(r[1:-1]) for r in routes] == [[1, 2, 3], [4, 5, 6]]
    _, _, routes = tight.vrp_solve(cost, n, q, 2.0, 3)
    assert [sorted(r[1:-1]) for r in routes] == [[1, 2], [3, 4], [5, 6]]
    for Q, K in ((1.5, 3), (2.0, 2)):                             # no route of two fits; three routes are needed
        with pytest.raises(ValueError):
            tight.vrp_solve(cost, n, q, Q, K)


@pytest.fixture(scope="module")
def cvrp9():
    """the reference test's shape: 9 customers, capacity 30, 3 vehicles, demands uniform on [0, 10)"""
    n = 10
    feats, costs, q = tight.vrp_gen_data(6, 5, n, seed=11)
    assert q.shape == (n - 1,) and q.dtype == np.float32 and (q >= 0).all() and (q < 10).all()
    return n, feats, costs, q, 30.0, 3


def test_reference_feasibility_checks_at_n10(cvrp9):
    n, _, costs, q, Q, K = cvrp9
    rng = np.random.RandomState(0)
    for c in list(costs) + [rng.rand(n * (n - 1) // 2).astype(np.float32) for _ in range(3)]:
        sol, obj, routes = tight.vrp_solve(c, n, q, Q, K)
        _check_feasible(sol, routes, n, q, Q, K)
        assert abs(float(c.astype(np.float64) @ sol) - obj) <= 2 * sol.sum() * 2.0 ** -52 * float(np.abs(c).astype(np.float64) @ sol)


def test_cut_loop_reaches_the_dynamic_programs_objective(cvrp9):
    n, _, costs, q, Q, K = cvrp9
    for c in costs[:4]:
        sol, obj, _ = tight.vrp_solve(c, n, q, Q, K)
        x, z, cuts = tight.vrp_rcc_cuts(c, n, q, Q, K)
        E = int(sol.sum())
        assert abs(z - obj) <= 2 * E * 2.0 ** -52 * float(np.abs(c).astype(np.float64) @ sol), (z, obj)
        _, eid = tight._edge_index(n)
        for comp, rhs in cuts:   # every cut is a valid inequality: it holds at the dynamic program's vertex too
            assert len(comp) >= 2 and float(tight._cut_row(comp, eid, len(sol)) @ sol) <= rhs + 1e-9


def test_tight_normals_rows(cvrp9):
    n, _, costs, q, Q, K = cvrp9
    d = n * (n - 1) // 2
    edges, _ = tight._edge_index(n)
    for c, vehicles in ((costs[0], K), (costs[1], K), (costs[0], 2)):
        try:
            sol, _, routes = tight.vrp_solve(c, n, q, Q, vehicles)
        except ValueError:
            continue
        cuts = tight.vrp_rcc_cuts(c, n, q, Q, vehicles)[2]
        A = tight.vrp_tight_normals(sol, n, cuts, vehicles)
        depot = int(2 * len(routes) == 2 * vehicles)
        deg = np.zeros((n, d), np.float32)
        deg[edges[:, 0], np.arange(d)] = 1.0
        deg[edges[:, 1], np.arange(d)] = 1.0
        r = 0
        if depot:
            assert np.array_equal(A[0], deg[0]) and float(A[0] @ sol) == 2 * vehicles
            r = 1
        assert np.array_equal(A[r:r + n - 1], deg[1:]) and np.array_equal(A[r + n - 1:r + 2 * (n - 1)], -deg[1:])
        assert (A[r:r + n - 1] @ sol == 2).all()
        r += 2 * (n - 1)
        ncut = len(A) - r - d
        rhs_of = {tuple(np.flatnonzero(tight._cut_row(comp, tight._edge_index(n)[1], d))): rhs for comp, rhs in cuts}
        for row in A[r:r + ncut]:   # each a cut in <= orientation, tight at sol
            assert set(np.unique(row)) <= {0.0, 1.0} and float(row @ sol) == rhs_of[tuple(np.flatnonzero(row))]
        low, high = A[r + ncut:r + ncut + int((sol == 0).sum())], A[r + ncut + int((sol == 0).sum()):]
        assert len(high) == int(sol.sum()) and (low.sum(1) == -1).all() and (high.sum(1) == 1).all()
        assert np.array_equal(np.flatnonzero(low.sum(0)), np.flatnonzero(sol == 0)) and np.array_equal(np.flatnonzero(high.sum(0)), np.flatnonzero(sol == 1))


def test_final_routes_of_three_or_more_carry_their_tight_row(cvrp9):
    """the reference adds the cut at every incumbent, the final one included: where the cut loop ends at the dynamic
    program's vertex, each of its routes with three or more customers has the row x(E(S)) <= |S| - 1 among the tight ones"""
    n, _, costs, q, Q, K = cvrp9
    hit = 0
    for c in costs[:4]:
        sol, _, routes = tight.vrp_solve(c, n, q, Q, K)
        x, _, cuts = tight.vrp_rcc_cuts(c, n, q, Q, K)
        if not np.array_equal(x, sol):
            continue   # another optimum of a tie (never with the generator's costs, but not excluded)
        hit += 1
        for t in routes:
            if len(t) - 2 >= 3:
                assert (sorted(t[1:-1]), float(len(t) - 3)) in [(sorted(cmp), rhs) for cmp, rhs in cuts]
    assert hit


def test_cone_dataset_shapes_and_regret(cvrp9):
    n, feats, costs, q, Q, K = cvrp9
    ds = tight.VRPConeDataset(feats[:3], costs[:3], n, q, Q, K)
    d = n * (n - 1) // 2
    assert len(ds) == 3 and ds.sols.shape == (3, d) and ds.objs.shape == (3, 1) and len(ds.ctrs) == 3
    for i in range(3):
        f, c, s, z, A = ds[i]
        depot = int(float(s[:n - 1].sum()) == 2 * K)   # the depot's edges are the first n - 1
        assert A.shape == (depot + 2 * (n - 1) + ds.tight_cuts[i] + d, d) and A.dtype == s.dtype
        assert abs(float(c.double() @ s.double()) - float(z)) <= 1e-5 * abs(float(z))
    assert tight.vrp_regret(costs[:3], costs[:3], ds.objs.numpy(), n, q, Q, K) == pytest.approx(0.0, abs=1e-6)
    worse = tight.vrp_regret(costs[3:6], costs[:3], ds.objs.numpy(), n, q, Q, K)
    assert worse >= -1e-6
    with pytest.raises(ValueError):   # an infeasible instance raises
        tight.VRPConeDataset(feats[:1], costs[:1], n, q, 5.0, K)
