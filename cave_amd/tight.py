"""Gurobi-free tight-cone construction for shortest-path and small TSP instances (and data generators).

The reference obtains, per training instance, the optimal vertex from Gurobi and then stacks the
normals of the constraints tight at it (`optDatasetConstrs._getSols` + `_extract_tight_normals`,
/root/reference src/dataset.py:74-106,147-215).  For PyEPO's grid shortest-path model the LP is a
min-cost path on a DAG (arcs go right or down), so the optimal vertex comes from one dynamic
program and every rule of `_extract_tight_normals` can be applied without a solver:

  * every explicit constraint is a flow-conservation EQUALITY, always tight -> `+a` block then `-a`
    block (src/dataset.py:182-184);
  * no lazy cuts (src/dataset.py:186-196 contributes nothing);
  * every arc variable sits at a bound of its [0,1] box -> `-e_k` rows for arcs at 0, then `+e_k`
    rows for arcs at 1 (src/dataset.py:198-211).

This is the "next" row f2 of SURVEY.md §8 and lets BASELINE configs[0] (SP 5x5, 100 instances,
batch 32) run end to end without Gurobi/PyEPO.  Host-side numpy; nothing here is on the hot path.

The same dynamic program, the backtrack, the regret numerator and the tight cone in the sparse wire format also run on
the device, one wave per instance (`sp_solve_hip`, `sp_cones_hip`; cave_amd/csrc/sp_grid.h): the additions and
comparisons of `sp_solve` in `sp_solve`'s order, so paths and objectives are equal bit for bit, and the entries
`SparseCones.from_ragged([sp_tight_normals(...)])` would hold, without the dense matrix.  `SPConeDataset(...,
device=...)` and `sp_regret(..., device=...)` use them; without a device both do what they always did.

Small TSP (DFJ model, src/model/tsp.py:54-60): the optimal tour comes from the Held-Karp dynamic program
(`tsp_solve`, exact, O(n^2 2^n), n <= 14); the subtour-elimination rows come from the SAME lazy rule the
reference's callback applies (first edge that closes a cycle in union-find order -> the cut of its component,
src/model/tsp.py:41-60), applied to the successive optima of the cut relaxation {degree rows, cuts so far,
binary x} (`tsp_dfj_cuts`, solved with SciPy's HiGHS MILP).  Which cuts a branch-and-cut run generates depends
on the solver's search path, so the cut SET is a restatement of the rule, not of Gurobi's path; the tight ones
among them are then stacked exactly as `_extract_tight_normals` does (src/dataset.py:182-211):
`+Deg`, `-Deg`, tight cuts in `<=` orientation, `-e_k` at 0, `+e_k` at 1.

Held-Karp also runs on the device, one workgroup per instance (`tsp_solve_hip`; cave_amd/csrc/tsp_hk.h): the additions
and strict comparisons of `tsp_solve` in `tsp_solve`'s candidate order, so tours, edge indicators and objectives are
equal bit for bit, ties included, 3 <= n <= 14.  A second tier, written for a table in HBM, takes 13 <= n <= 20
(`tsp_solve_hip_wide`; cave_amd/csrc/tsp_hk_wide.h: a predecessor set loads its entries once and extends them to every
successor): the same recurrence bit for bit, beyond the 14 nodes at which the host's `tsp_solve` stops.
`tsp_regret(..., device=...)` uses the first up to 14 nodes and the second from 15 to 20; without a device it does what
it always did.  The DFJ cut set (`tsp_dfj_cuts`, `TSPConeDataset`) stays on the host at every size.

Small CVRP (the reference's `vrpModel`, src/model/vrp.py:114-209: depot degree <= 2K, customer degrees = 2, lazy
rounded-capacity cuts): the optimum comes from a dynamic program on top of the Held-Karp table (`vrp_solve`: a route
through a customer set costs its Held-Karp path plus the closing edge, a set-partition recurrence over the subsets picks
the routes), the cuts from the rule of the reference's callback applied to the successive optima of the cut relaxation
(`vrp_rcc_cuts`), the tight rows as for the TSP (`vrp_tight_normals`).  The dynamic program also runs on the device, one
workgroup per instance (`vrp_solve_hip`; cave_amd/csrc/vrp_dp.h), bit for bit, and from 13 to 20 nodes with its tables in
device memory (`vrp_solve_hip_wide`; cave_amd/csrc/vrp_dp_wide.h); `VRPConeDataset(..., device=...)` and
`vrp_regret(..., device=...)` use the first up to 14 nodes and the second beyond.  The cut loop stays on the host.

Tight cones of any binary LP on the device (`tight_cones_hip`; cave_amd/csrc/tight_cones.h): the rule of
`_extract_tight_normals` for a batch of vertices of one constraint system in CSR form (`LinSystem`: a model's `getA()`,
senses and right-hand sides; `tsp_system`, `vrp_system`, `sp_system` are the explicit rows of the three models restated
here) plus per-instance lazy rows (`cut_rows`: node sets as sparse rows), written directly as SparseCones -- the entries
`SparseCones.from_ragged` holds for the dense matrices `*_tight_normals` build, without those matrices.
`TSPConeDataset(..., device=)` and `VRPConeDataset(..., device=, cones="sparse")` use it.  Limits: d <= 65535 columns,
65535 rows per instance; the cut loops (HiGHS) stay on the host.
"""

from __future__ import annotations

import numpy as np

from .synth import sp_arcs

__all__ = ["sp_solve", "sp_tight_normals", "sp_gen_data", "SPConeDataset", "sp_regret", "sp_solve_hip", "sp_cones_hip",
           "tsp_solve", "tsp_dfj_cuts", "tsp_tight_normals", "tsp_gen_data", "TSPConeDataset", "tsp_regret", "tsp_solve_hip",
           "tsp_solve_hip_wide",
           "vrp_solve", "vrp_rcc_cuts", "vrp_tight_normals", "vrp_gen_data", "VRPConeDataset", "vrp_regret", "vrp_solve_hip",
           "vrp_solve_hip_wide",
           "LinSystem", "tsp_system", "vrp_system", "sp_system", "cut_rows", "tight_cones_hip"]


def sp_solve(cost: np.ndarray, h: int, w: int):
    """Shortest source->sink path on the h x w grid DAG.  Returns (sol (d,) float32 0/1, objective)."""
    arcs = sp_arcs(h, w)
    n = h * w
    dist = np.full(n, np.inf)
    pred = np.full(n, -1, dtype=np.int64)
    dist[0] = 0.0
    # arcs are emitted row by row, every arc goes to a larger node index: one pass in order is a valid DP
    for k, (a, b) in enumerate(arcs):
        nd = dist[a] + cost[k]
        if nd < dist[b]:
            dist[b] = nd
            pred[b] = k
    sol = np.zeros(len(arcs), dtype=np.float32)
    v = n - 1
    while v != 0:
        k = pred[v]
        sol[k] = 1.0
        v = arcs[k][0]
    return sol, float(dist[n - 1])


def sp_tight_normals(sol: np.ndarray, h: int, w: int) -> np.ndarray:
    """`_extract_tight_normals` for the grid shortest-path model at vertex `sol` (float32 (m, d))."""
    arcs = sp_arcs(h, w)
    d = len(arcs)
    # flow conservation row of node v: +1 on arcs entering v, -1 on arcs leaving v
    N = np.zeros((h * w, d), dtype=np.float32)
    N[arcs[:, 1], np.arange(d)] = 1.0
    N[arcs[:, 0], np.arange(d)] = -1.0
    low = np.where(sol <= 1e-5)[0]
    high = np.where(sol >= 1 - 1e-5)[0]
    low_rows = np.zeros((len(low), d), dtype=np.float32)
    low_rows[np.arange(len(low)), low] = -1.0
    high_rows = np.zeros((len(high), d), dtype=np.float32)
    high_rows[np.arange(len(high)), high] = 1.0
    return np.vstack([N, -N, low_rows, high_rows]).astype(np.float32)


def sp_gen_data(num_data: int, num_feat: int, h: int, w: int, deg: int = 4, noise_width: float = 0.5, seed: int = 135):
    """Features and arc costs in the style of PyEPO's shortest-path generator (polynomial of degree
    `deg` of a random linear map, multiplicative noise), as used by code_sample.py:26-29 for TSP."""
    rng = np.random.RandomState(seed)
    d = len(sp_arcs(h, w))
    Bm = rng.binomial(1, 0.5, (d, num_feat))
    x = rng.normal(0, 1, (num_data, num_feat))
    c = (x @ Bm.T / np.sqrt(num_feat) + 3.0) ** deg + 1.0
    c /= 3.5 ** deg
    c *= rng.uniform(1 - noise_width, 1 + noise_width, c.shape)
    return x.astype(np.float32), c.astype(np.float32)


def _hip_solve(who: str, entry: str, costs, eval_costs, d: int, columns: str, own, ws_args, call):
    """One launch of the exact-solver entry cave_hip_<entry>_solve, the part `sp_solve_hip`, `tsp_solve_hip[_wide]` and
    `vrp_solve_hip` share: costs (N, d) float32 on the device and eval_costs like it or None are checked (`who` and
    `columns`, e.g. "a TSP on 5 nodes has 10 edges", go into the messages); sols, objs, evals (with eval_costs) and the
    status are allocated, then the entry's own tensors `own(N, device)` (a list) and -- `ws_args`: the size query's
    arguments in front of N, None: the entry has no workspace -- the default workspace for the call;
    `call(solve, costs, eval_costs, N, sols, objs, evals, status, own, ws, ws_bytes, stream)`, all pointers, launches
    under the device guard.  -> (sols, objs, evals or None, index of the first instance whose status is not OK or None,
    status, own)."""
    import torch

    from . import _lib

    lib = _lib.load()
    if not (isinstance(costs, torch.Tensor) and costs.is_cuda and costs.dtype == torch.float32 and costs.dim() == 2):
        raise ValueError(f"{who}: costs must be a (N, d) float32 tensor on the device")
    if costs.shape[1] != d:
        raise ValueError(f"{who}: {columns}, costs has {costs.shape[1]} columns")
    costs = costs.contiguous()
    if eval_costs is not None:
        if not (isinstance(eval_costs, torch.Tensor) and eval_costs.dtype == torch.float32 and eval_costs.shape == costs.shape
                and eval_costs.device == costs.device):
            raise ValueError(f"{who}: eval_costs must match costs in shape, dtype and device")
        eval_costs = eval_costs.contiguous()
    N, dev = costs.shape[0], costs.device
    sols = torch.empty(N, d, dtype=torch.float32, device=dev)
    objs = torch.empty(N, dtype=torch.float64, device=dev)
    evals = torch.empty(N, dtype=torch.float64, device=dev) if eval_costs is not None else None
    status = torch.empty(N, dtype=torch.int32, device=dev)
    own = own(N, dev)
    ws_bytes = 0
    if ws_args is not None:
        ws_bytes = int(getattr(lib, f"cave_hip_{entry}_workspace_bytes")(*ws_args, N))
        if ws_bytes < 0:
            _lib.check(ws_bytes, f"cave_hip_{entry}_workspace_bytes")
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev) if ws_bytes and N else None
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(call(getattr(lib, f"cave_hip_{entry}_solve"), p(costs), p(eval_costs), N, p(sols), p(objs), p(evals), p(status),
                        [p(t) for t in own], p(ws), ws_bytes if ws is not None else 0, _lib.current_stream()),
                   f"cave_hip_{entry}_solve")
    bad = int(torch.nonzero(status != _lib.ST_OK)[0]) if N and bool((status != _lib.ST_OK).any()) else None
    return sols, objs, evals, bad, status, own


def _regret_hip(evals_of, pred_costs, true_costs, true_objs, device) -> float:
    """The `device=` branch of `sp_regret`, `tsp_regret` and `vrp_regret`: the three inputs go to the device as float32,
    `evals_of(pred, true)` solves under pred and prices under true there, the fp64 sums are formed there."""
    import torch

    device = torch.device(device)
    cp, c, z = (torch.as_tensor(t).detach().to(device=device, dtype=torch.float32) for t in (pred_costs, true_costs, true_objs))
    evals = evals_of(cp, c)
    z = z.reshape(-1).to(torch.float64)
    return float(((evals - z).sum() / (z.abs().sum() + 1e-7)).item())


def _sp_grid_call(costs, h: int, w: int, eval_costs=None, cones: bool = False):
    """One launch of cave_hip_sp_grid_solve on a (N, d) float32 device tensor -> (sols, objs, evals or None, key, val)."""
    import torch

    from . import _lib

    _lib.load()  # (no device: ImportError before any check of the arguments)
    h, w = int(h), int(w)
    d = h * (w - 1) + (h - 1) * w

    def own(N, dev):
        return [torch.empty(N * 5 * d, dtype=t, device=dev) if cones else None for t in (torch.int32, torch.float32)]

    sols, objs, evals, bad, _, (key, val) = _hip_solve(
        "sp_solve_hip", "sp_grid", costs, eval_costs, d, f"a {h} x {w} grid has {d} arcs", own, None,
        lambda solve, c, e, N, s, o, ev, st, x, ws, wsb, stream: solve(c, e, N, h, w, s, o, ev, st, x[0], x[1], stream))
    if bad is not None:
        raise ValueError(f"sp_solve_hip: instance {bad} has a non-finite cost")
    return sols, objs, evals, key, val


def sp_solve_hip(costs, h: int, w: int, eval_costs=None):
    """`sp_solve` for a batch on the device: costs (N, d) float32 -> (sols (N, d) float32 0/1, objs (N,) float64), equal
    to the host's bit for bit.  With `eval_costs` (N, d) a third result: evals (N,) float64, each path priced under the
    second cost tensor (the regret numerator).  A non-finite cost raises ValueError."""
    sols, objs, evals, _, _ = _sp_grid_call(costs, h, w, eval_costs)
    return (sols, objs) if eval_costs is None else (sols, objs, evals)


def sp_cones_hip(costs, h: int, w: int):
    """Solve and, in the same launch, write the tight cones of the optimal vertices in the sparse wire format ->
    (SparseCones on the device, sols, objs): the tensors `SparseCones.from_ragged([sp_tight_normals(s, h, w) for s in
    sols])` holds, without a dense matrix or a host round trip.  Needs 2 h w + d <= 65535."""
    from .sparse import SparseCones

    sols, objs, _, key, val = _sp_grid_call(costs, h, w, None, cones=True)
    d = sols.shape[1]
    return SparseCones.from_uniform(2 * h * w + d, d, 5 * d, key, val), sols, objs


class SPConeDataset:
    """`optDatasetConstrs` (src/dataset.py:26-130) for the grid shortest path, without Gurobi:
    feats, costs, sols, objs and the ragged list of tight-constraint normals `ctrs`.

    With `device`: solved on the device in one launch (`sp_cones_hip`); feats, costs, sols and objs live there, there is
    no dense `ctrs` list, `.cones` is the SparseCones of the whole set on the device and item i carries its one-instance
    slice (views, no copy) -- what `collate_sparse`, `ConeStore.from_sparse(dataset.cones)` and `prefetch` take."""

    def __init__(self, feats: np.ndarray, costs: np.ndarray, h: int, w: int, device=None):
        import torch

        self.h, self.w = h, w
        self.cones = None
        if device is not None:
            device = torch.device(device)
            self.feats = torch.as_tensor(feats, dtype=torch.float32).to(device)
            self.costs = torch.as_tensor(costs, dtype=torch.float32).to(device)
            self.cones, self.sols, objs = sp_cones_hip(self.costs, h, w)
            self.objs = objs.to(torch.float32)[:, None]
            self._off1 = self.cones.ent_off[:2]
            return
        sols, objs, ctrs = [], [], []
        for c in costs:
            s, o = sp_solve(c, h, w)
            sols.append(s)
            objs.append([o])
            ctrs.append(sp_tight_normals(s, h, w))
        self.feats = torch.as_tensor(feats, dtype=torch.float32)
        self.costs = torch.as_tensor(costs, dtype=torch.float32)
        self.sols = torch.as_tensor(np.stack(sols), dtype=torch.float32)
        self.objs = torch.as_tensor(np.asarray(objs), dtype=torch.float32)
        self.ctrs = [torch.as_tensor(c, dtype=torch.float32) for c in ctrs]

    def __len__(self) -> int:
        return len(self.feats)

    def __getitem__(self, i: int):
        if self.cones is not None:
            from .sparse import SparseCones

            i = int(i) % len(self)
            z = 5 * self.cones.d  # entries per instance
            cone = SparseCones(self.cones.m_max, self.cones.d, self._off1, self.cones.key[i * z:(i + 1) * z],
                               self.cones.val[i * z:(i + 1) * z])
            return self.feats[i], self.costs[i], self.sols[i], self.objs[i], cone
        return self.feats[i], self.costs[i], self.sols[i], self.objs[i], self.ctrs[i]


def sp_regret(pred_costs: np.ndarray, true_costs: np.ndarray, true_objs: np.ndarray, h: int, w: int, device=None) -> float:
    """Normalised regret sum(c . w(c_hat) - z*) / sum(z*) (PyEPO `metric.regret` for a MIN problem).

    With `device`: arrays or tensors, moved to the device if they are not there; solved and priced there in one launch
    (fp64 sums), only the scalar comes back."""
    if device is not None:
        return _regret_hip(lambda cp, c: sp_solve_hip(cp, h, w, eval_costs=c)[2], pred_costs, true_costs, true_objs, device)
    loss = 0.0
    for cp, c, z in zip(pred_costs, true_costs, true_objs):
        s, _ = sp_solve(cp, h, w)
        loss += float(c @ s) - float(z)
    return loss / float(np.abs(true_objs).sum() + 1e-7)


# ------------------------------------------------------------------ small TSP (DFJ)

def _edge_index(n: int):
    from .synth import tsp_edges

    edges = tsp_edges(n)
    eid = -np.ones((n, n), dtype=np.int64)
    eid[edges[:, 0], edges[:, 1]] = np.arange(len(edges))
    eid[edges[:, 1], edges[:, 0]] = np.arange(len(edges))
    return edges, eid


def _held_karp(cost: np.ndarray, n: int):
    """The Held-Karp table of `tsp_solve` and `vrp_solve`: -> (edges, eid, D, dp, parent).  dp[S, j] is the cheapest path
    from the depot through the customer set S (node j+1 is bit j) that ends in j; parent[S, j] its last-but-one node
    (lowest index on a tie, np.argmin's rule), -1 where the path is the single edge from the depot."""
    if n > 14:
        raise ValueError("Held-Karp is meant for n <= 14 here (2^n n^2 work and memory)")
    edges, eid = _edge_index(n)
    D = np.zeros((n, n))
    D[edges[:, 0], edges[:, 1]] = cost
    D[edges[:, 1], edges[:, 0]] = cost
    m = n - 1  # nodes 1..n-1 as bits 0..m-1; node 0 is the depot
    full = 1 << m
    dp = np.full((full, m), np.inf)
    parent = np.full((full, m), -1, dtype=np.int64)
    for j in range(m):
        dp[1 << j, j] = D[0, j + 1]
    Dm = D[1:, 1:]
    for mask in range(1, full):
        row = dp[mask]
        if not np.isfinite(row).any():
            continue
        # extend every end node k of `mask` to every j outside it
        cand = row[:, None] + Dm  # (k, j)
        best_k = np.argmin(cand, axis=0)
        best = cand[best_k, np.arange(m)]
        for j in range(m):
            if mask >> j & 1:
                continue
            nm = mask | (1 << j)
            if best[j] < dp[nm, j]:
                dp[nm, j] = best[j]
                parent[nm, j] = best_k[j]
    return edges, eid, D, dp, parent


def _hk_walk(D, dp, parent, mask: int):
    """Close the cheapest path through the customer set `mask` at the depot and walk it back: -> (cost with the closing
    edge, nodes from the closing edge's end back to the first customer).  First minimum over the end nodes."""
    last = dp[mask] + D[1:, 0]
    j = int(np.argmin(last))
    obj = float(last[j])
    walk = []
    while j >= 0:
        walk.append(j + 1)
        pj = int(parent[mask, j])
        mask ^= 1 << j
        j = pj
    return obj, walk


def tsp_solve(cost: np.ndarray, n: int):
    """Optimal tour of the symmetric TSP with edge costs `cost` (lexicographic (i<j) order, d = n(n-1)/2) by
    the Held-Karp dynamic program.  Returns (sol (d,) float32 0/1 edge indicator, objective, tour list)."""
    edges, eid, D, dp, parent = _held_karp(cost, n)
    obj, walk = _hk_walk(D, dp, parent, (1 << (n - 1)) - 1)
    tour = [0] + walk[::-1]
    sol = np.zeros(len(edges), dtype=np.float32)
    for a, b in zip(tour, tour[1:] + tour[:1]):
        sol[eid[a, b]] = 1.0
    return sol, obj, tour


def _first_subtour(sel_edges, n: int):
    """The reference callback's detection (src/model/tsp.py:47-56): union-find over the selected edges in
    order; the first edge that closes a cycle names the component to cut (None if that is the whole tour)."""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in sel_edges:
        ri, rj = find(i), find(j)
        if ri == rj:
            comp = [k for k in range(n) if find(k) == ri]
            return comp if len(comp) < n else None
        parent[ri] = rj
    return None


def tsp_dfj_cuts(cost: np.ndarray, n: int, max_rounds: int = 200):
    """DFJ cutting loop: solve {degree rows, cuts so far, x binary} exactly (HiGHS), cut the first subtour found
    by the reference's rule, repeat.  Returns (sol (d,) 0/1, objective, list of node sets cut)."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    from scipy.sparse import csr_matrix, vstack

    edges, eid = _edge_index(n)
    d = len(edges)
    deg = np.zeros((n, d))
    deg[edges[:, 0], np.arange(d)] = 1.0
    deg[edges[:, 1], np.arange(d)] = 1.0
    cons = [LinearConstraint(csr_matrix(deg), 2.0, 2.0)]
    cuts: list[list[int]] = []
    for _ in range(max_rounds):
        res = milp(np.asarray(cost, dtype=np.float64), constraints=cons, integrality=np.ones(d), bounds=Bounds(0, 1))
        if res.status != 0:
            raise RuntimeError(f"cut relaxation not solved (status {res.status})")
        x = np.round(res.x)
        sel = [(int(edges[k, 0]), int(edges[k, 1])) for k in np.flatnonzero(x > 0.5)]
        comp = _first_subtour(sel, n)
        if comp is None:
            return x.astype(np.float32), float(cost @ x), cuts
        row = np.zeros((1, d))
        for a in range(len(comp)):
            for b in range(a + 1, len(comp)):
                row[0, eid[comp[a], comp[b]]] = 1.0
        cons.append(LinearConstraint(csr_matrix(row), -np.inf, len(comp) - 1.0))
        cuts.append(comp)
    raise RuntimeError("DFJ cutting loop did not terminate")


def tsp_tight_normals(sol: np.ndarray, n: int, cuts, tol: float = 1e-5) -> np.ndarray:
    """`_extract_tight_normals` (src/dataset.py:147-215) for the DFJ model at vertex `sol`: degree equalities
    (`+a` block then `-a` block), the lazy cuts that are tight at `sol` (already `<=` rows), `-e_k` at 0, `+e_k` at 1."""
    edges, eid = _edge_index(n)
    d = len(edges)
    deg = np.zeros((n, d), dtype=np.float32)
    deg[edges[:, 0], np.arange(d)] = 1.0
    deg[edges[:, 1], np.arange(d)] = 1.0
    rows = [deg, -deg]
    lazy = []
    for comp in cuts:
        r = np.zeros(d, dtype=np.float32)
        for a in range(len(comp)):
            for b in range(a + 1, len(comp)):
                r[eid[comp[a], comp[b]]] = 1.0
        if abs((len(comp) - 1.0) - float(r @ sol)) < tol:  # src/dataset.py:192-193
            lazy.append(r)
    if lazy:
        rows.append(np.asarray(lazy, dtype=np.float32))
    low = np.where(sol <= tol)[0]
    high = np.where((sol >= 1 - tol) & ~(sol <= tol))[0]
    low_rows = np.zeros((len(low), d), dtype=np.float32)
    low_rows[np.arange(len(low)), low] = -1.0
    high_rows = np.zeros((len(high), d), dtype=np.float32)
    high_rows[np.arange(len(high)), high] = 1.0
    return np.vstack(rows + [low_rows, high_rows]).astype(np.float32)


def tsp_gen_data(num_data: int, num_feat: int, n: int, deg: int = 4, noise_width: float = 0.5, seed: int = 42):
    """Features and edge costs in the style of PyEPO's TSP generator used by code_sample.py:20: Euclidean
    distances between random node positions plus a polynomial of a random linear map of the features, with
    multiplicative noise.  Returns (feats (N, p) float32, costs (N, d) float32)."""
    from .synth import tsp_edges

    rng = np.random.RandomState(seed)
    edges = tsp_edges(n)
    d = len(edges)
    pos = np.r_[rng.uniform(-2, 2, (n // 2, 2)), rng.normal(0, 1, (n - n // 2, 2))]
    dist = np.linalg.norm(pos[edges[:, 0]] - pos[edges[:, 1]], axis=1)
    Bm = rng.binomial(1, 0.5, (d, num_feat))
    x = rng.normal(0, 1, (num_data, num_feat))
    time = (x @ Bm.T / np.sqrt(num_feat) + 3.0) ** deg / 3.0 ** (deg - 1)
    time *= rng.uniform(1 - noise_width, 1 + noise_width, time.shape)
    return x.astype(np.float32), (dist[None, :] * 3.0 + time).astype(np.float32)


class TSPConeDataset:
    """`optDatasetConstrs` (src/dataset.py:26-130) for the DFJ TSP model without Gurobi.

    With `device`: the cut loop runs on the host as always and its vertex is kept; the tight cones are written on the
    device by `tight_cones_hip` from the degree rows (`tsp_system`) and the cuts as sparse lazy rows (`cut_rows`).  There
    is no dense `ctrs` list: feats, costs, sols and objs live on the device, `.cones` is the SparseCones of the whole set
    and item i carries its one-instance slice (views, no copy), as `SPConeDataset(..., device=)` does."""

    def __init__(self, feats: np.ndarray, costs: np.ndarray, n: int, device=None):
        import torch

        self.n = n
        self.cones = None
        if device is not None:
            device = torch.device(device)
            sols, objs, cuts = [], [], []
            for c in costs:
                s, o, k = tsp_dfj_cuts(c, n)
                sols.append(s)
                objs.append(o)
                cuts.append(k)
            sols = torch.as_tensor(np.stack(sols), dtype=torch.float32).to(device)
            cones, n_rows = _tight_cones_call(tsp_system(n), sols, cut_rows(n, cuts), 1e-5)
            _device_cone_items(self, device, feats, costs, sols, objs, cones)
            self.tight_cuts = [int(v) - 2 * n - sols.shape[1] for v in n_rows.tolist()]
            return
        sols, objs, ctrs, ncuts = [], [], [], []
        for c in costs:
            s, o, cuts = tsp_dfj_cuts(c, n)
            sols.append(s)
            objs.append([o])
            A = tsp_tight_normals(s, n, cuts)
            ctrs.append(A)
            ncuts.append(len(A) - 2 * n - len(s))
        self.feats = torch.as_tensor(feats, dtype=torch.float32)
        self.costs = torch.as_tensor(costs, dtype=torch.float32)
        self.sols = torch.as_tensor(np.stack(sols), dtype=torch.float32)
        self.objs = torch.as_tensor(np.asarray(objs), dtype=torch.float32)
        self.ctrs = [torch.as_tensor(c, dtype=torch.float32) for c in ctrs]
        self.tight_cuts = ncuts

    def __len__(self) -> int:
        return len(self.feats)

    def __getitem__(self, i: int):
        if self.cones is not None:
            return _device_cone_item(self, i)
        return self.feats[i], self.costs[i], self.sols[i], self.objs[i], self.ctrs[i]


def _tsp_hk_hip(who: str, entry: str, lo: int, hi: int, costs, n: int, eval_costs):
    """`tsp_solve_hip` and `tsp_solve_hip_wide`: the node range, the tours and the launch of cave_hip_<entry>_solve."""
    import torch

    from . import _lib

    _lib.load()  # (no device: ImportError before any check of the arguments)
    n = int(n)
    if not lo <= n <= hi:
        raise ValueError(f"{who}: Held-Karp on the device takes {lo} <= n <= {hi} nodes, not {n}")
    d = n * (n - 1) // 2
    sols, objs, evals, bad, _, (tours,) = _hip_solve(
        who, entry, costs, eval_costs, d, f"a TSP on {n} nodes has {d} edges",
        lambda N, dev: [torch.empty(N, n, dtype=torch.int32, device=dev)], (n,),
        lambda solve, c, e, N, s, o, ev, st, x, ws, wsb, stream: solve(c, e, N, n, s, o, ev, x[0], st, ws, wsb, stream))
    if bad is not None:
        raise ValueError(f"{who}: instance {bad} has a non-finite cost")
    return (sols, objs, tours) if eval_costs is None else (sols, objs, tours, evals)


def tsp_solve_hip(costs, n: int, eval_costs=None):
    """`tsp_solve` for a batch on the device: costs (N, d) float32, d = n (n-1) / 2, 3 <= n <= 14 -> (sols (N, d) float32
    0/1, objs (N,) float64, tours (N, n) int32 starting at node 0), equal to the host's bit for bit.  With `eval_costs`
    (N, d) a fourth result: evals (N,) float64, each tour priced under the second cost tensor (the regret numerator; the
    fp64 sum of its n edges in tour order).  For n = 13, 14 the table of the dynamic program lies in a workspace that is
    allocated here for the call (at most 512 slots: 101 MB, 218 MB).  A non-finite cost raises ValueError."""
    return _tsp_hk_hip("tsp_solve_hip", "tsp_hk", 3, 14, costs, n, eval_costs)


def tsp_solve_hip_wide(costs, n: int, eval_costs=None):
    """`tsp_solve_hip` for 13 <= n <= 20 (cave_hip_tsp_hk_wide_solve, cave_amd/csrc/tsp_hk_wide.h): the same arguments,
    checks, results and errors, the same recurrence bit for bit -- beyond the host solver's 14 nodes, what `tsp_solve`
    would return if it went that far.  The table always lies in a workspace that is allocated here for the call: one slot
    of (n-1) 2^(n-2) doubles per workgroup (0.9 MB at n = 15, 39.8 MB at n = 20), min(N, 512, 8 GiB / slot) of them
    (215 slots, 8.6 GB at n = 20), behind a 4 * 2^(n-1)-byte list."""
    return _tsp_hk_hip("tsp_solve_hip_wide", "tsp_hk_wide", 13, 20, costs, n, eval_costs)


def tsp_regret(pred_costs: np.ndarray, true_costs: np.ndarray, true_objs: np.ndarray, n: int, device=None) -> float:
    """Normalised regret sum(c . w(c_hat) - z*) / sum(z*) with w(.) from Held-Karp.

    With `device`: arrays or tensors, moved to the device if they are not there; solved and priced there in one launch
    (fp64 sums), only the scalar comes back.  Up to 14 nodes through `tsp_solve_hip`, 15 to 20 through
    `tsp_solve_hip_wide`; without a device the host solver's limit of 14 nodes holds."""
    if device is not None:
        solve = tsp_solve_hip if int(n) <= 14 else tsp_solve_hip_wide
        return _regret_hip(lambda cp, c: solve(cp, n, eval_costs=c)[3], pred_costs, true_costs, true_objs, device)
    loss = 0.0
    for cp, c, z in zip(pred_costs, true_costs, true_objs):
        s, _, _ = tsp_solve(cp, n)
        loss += float(c @ s) - float(z)
    return loss / float(np.abs(true_objs).sum() + 1e-7)


# ------------------------------------------------------------------ small CVRP (2-degree model, rounded-capacity cuts)

def _vrp_tables(cost: np.ndarray, n: int, demands, capacity: float, num_vehicle: int):
    """The tables of `vrp_solve`: Held-Karp, r(S) (the cheapest feasible route through S; +inf otherwise) and the layers
    g_k(S) (the cheapest partition of S into exactly k feasible routes) with their argmins."""
    edges, eid, D, dp, parent = _held_karp(cost, n)
    m = n - 1
    full = 1 << m
    q = np.asarray(demands).reshape(-1)
    if len(q) != m:
        raise ValueError(f"vrp_solve: {m} customers, {len(q)} demands")
    # load(S): the fp64 sum of q_j over j in S, ascending j, from 0.0 -- the highest bit is added last
    load = np.zeros(full)
    for j in range(m):
        load[1 << j:2 << j] = load[:1 << j] + np.float64(q[j])
    pc = np.zeros(full, dtype=np.int64)
    for j in range(m):
        pc[1 << j:2 << j] = pc[:1 << j] + 1
    feas = (pc >= 2) & (load <= capacity)
    closed = dp + D[1:, 0][None, :]  # +inf where j is not in S
    r = np.where(feas, closed[np.arange(full), np.argmin(closed, axis=1)], np.inf)  # first minimum over j, ascending
    kmax = min(int(num_vehicle), m // 2)
    layers, args = [None, r], [None, None]  # layers[k][S] = g_k(S)
    for k in range(2, kmax + 1):
        prev = layers[k - 1]
        g = np.full(full, np.inf)
        arg = np.zeros(full, dtype=np.int64)
        for S in ([full - 1] if k == kmax else range(full)):  # the last layer is read at the full set only
            if pc[S] < 2 * k:
                continue
            low = S & -S
            subs = np.zeros(1, dtype=np.int64)  # the subsets of S without its lowest bit, in ascending order
            rest = S ^ low
            while rest:
                b = rest & -rest
                rest ^= b
                subs = np.concatenate([subs, subs | b])
            R = (subs | low)[:-1]  # proper subsets that hold the lowest bit, ascending
            val = r[R] + prev[S ^ R]
            i = int(np.argmin(val))  # first minimum; an infinite pair never beats the initial +inf
            if val[i] < np.inf:
                g[S], arg[S] = val[i], R[i]
        layers.append(g)
        args.append(arg)
    return edges, eid, D, dp, parent, layers, args, kmax


def vrp_solve(cost: np.ndarray, n: int, demands, capacity: float, num_vehicle: int):
    """Optimal solution of the CVRP of the reference's `vrpModel` (src/model/vrp.py): node 0 the depot, customers 1..n-1
    with `demands` (n-1,), at most `num_vehicle` depot-anchored routes of at least two customers each (the reference
    excludes single-customer routes so that x stays binary), every route's load <= capacity, every customer on one route.
    Exact, by dynamic programming: a route through the customer set R costs the Held-Karp path through R plus the closing
    edge; a set-partition recurrence over the subsets picks the routes.

    Returns (sol (d,) float32 0/1 edge indicator, objective, routes), each route `[0, customers..., 0]`, routes in order
    of their lowest customer.  Ties: the first minimum everywhere -- fewest routes, then the numerically smallest
    customer set for the route of the lowest customer, then Held-Karp's rule inside a route.  With one vehicle and
    infinite capacity this is `tsp_solve`, bit for bit.  Raises ValueError where no feasible partition exists."""
    edges, eid, D, dp, parent, layers, args, kmax = _vrp_tables(cost, n, demands, capacity, num_vehicle)
    full = (1 << (n - 1)) - 1
    best, obj = 0, np.inf
    for k in range(1, kmax + 1):
        if layers[k][full] < obj:  # strict: the fewest routes win a tie
            best, obj = k, layers[k][full]
    if best == 0:
        raise ValueError("vrp_solve: the instance is infeasible (no partition into feasible routes)")
    routes, S = [], full
    for k in range(best, 0, -1):
        R = int(args[k][S]) if k > 1 else S
        routes.append([0] + _hk_walk(D, dp, parent, R)[1][::-1] + [0])
        S ^= R
    sol = np.zeros(len(edges), dtype=np.float32)
    for rt in routes:
        for a, b in zip(rt, rt[1:]):
            sol[eid[a, b]] = 1.0
    return sol, float(obj), routes


def _cut_row(comp, eid, d: int) -> np.ndarray:
    r = np.zeros(d)
    for a in range(len(comp)):
        for b in range(a + 1, len(comp)):
            r[eid[comp[a], comp[b]]] = 1.0
    return r


def vrp_rcc_cuts(cost: np.ndarray, n: int, demands, capacity: float, num_vehicle: int, max_rounds: int = 400):
    """The cutting loop of the reference's `vrpModel`: solve {depot degree <= 2K, customer degrees = 2, cuts so far, x
    binary} exactly (HiGHS), form the components of the selected customer-customer edges and give every component S of
    three or more customers the rounded-capacity cut x(E(S)) <= |S| - ceil(q(S) / Q) -- the rule of `_vrpCallback`
    (src/model/vrp.py:184-209), which adds the cut at every incumbent, violated or not, so each final route of three or
    more customers carries its tight row.  One deviation: a two-customer component over capacity gets x_ab <= 0 (the
    reference skips components below three and would accept that route).  The loop stops when no added cut is violated.
    Meant for feasible instances (`vrp_solve` decides that first).  Returns (sol (d,) 0/1, objective, cuts), a cut being
    (sorted customer list, right-hand side)."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    from scipy.sparse import csr_matrix

    edges, eid = _edge_index(n)
    d = len(edges)
    q = np.asarray(demands, dtype=np.float64).reshape(-1)
    deg = np.zeros((n, d))
    deg[edges[:, 0], np.arange(d)] = 1.0
    deg[edges[:, 1], np.arange(d)] = 1.0
    cons = [LinearConstraint(csr_matrix(deg[:1]), -np.inf, 2.0 * num_vehicle), LinearConstraint(csr_matrix(deg[1:]), 2.0, 2.0)]
    cuts, seen = [], set()
    cost = np.asarray(cost, dtype=np.float64)
    for _ in range(max_rounds):
        res = milp(cost, constraints=cons, integrality=np.ones(d), bounds=Bounds(0, 1), options={"mip_rel_gap": 0})
        if res.status != 0:
            raise RuntimeError(f"cut relaxation not solved (status {res.status})")
        x = np.round(res.x)
        parent = list(range(n))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        for k in np.flatnonzero(x > 0.5):
            a, b = int(edges[k, 0]), int(edges[k, 1])
            if a != 0:
                parent[find(a)] = find(b)
        comps: dict = {}
        for v in range(1, n):
            comps.setdefault(find(v), []).append(v)
        violated = False
        for comp in comps.values():
            load = float(sum(q[v - 1] for v in comp))
            if len(comp) >= 3:
                rhs = float(len(comp) - int(np.ceil(load / capacity)))
            elif len(comp) == 2 and load > capacity:
                rhs = 0.0
            else:
                continue
            key = (tuple(comp), rhs)
            if key in seen:
                continue
            seen.add(key)
            row = _cut_row(comp, eid, d)
            cons.append(LinearConstraint(csr_matrix(row[None, :]), -np.inf, rhs))
            cuts.append((list(comp), rhs))
            violated = violated or float(row @ x) > rhs + 0.5
        if not violated:
            return x.astype(np.float32), float(cost @ x), cuts
    raise RuntimeError("rounded-capacity cutting loop did not terminate")


def vrp_tight_normals(sol: np.ndarray, n: int, cuts, num_vehicle: int, tol: float = 1e-5) -> np.ndarray:
    """`_extract_tight_normals` (src/dataset.py:147-215) for the `vrpModel` at vertex `sol`.  Row order: the depot row
    `+a` if the depot degree equals 2K (a tight `<=` row), the customer degree equalities (`+a` block then `-a` block),
    the cuts that are tight at `sol`, `-e_k` at 0, `+e_k` at 1."""
    edges, eid = _edge_index(n)
    d = len(edges)
    deg = np.zeros((n, d), dtype=np.float32)
    deg[edges[:, 0], np.arange(d)] = 1.0
    deg[edges[:, 1], np.arange(d)] = 1.0
    rows = []
    if abs(2.0 * num_vehicle - float(deg[0] @ sol)) < tol:
        rows.append(deg[:1])
    rows += [deg[1:], -deg[1:]]
    lazy = []
    for comp, rhs in cuts:
        r = _cut_row(comp, eid, d).astype(np.float32)
        if abs(rhs - float(r @ sol)) < tol:
            lazy.append(r)
    if lazy:
        rows.append(np.asarray(lazy, dtype=np.float32))
    low = np.where(sol <= tol)[0]
    high = np.where((sol >= 1 - tol) & ~(sol <= tol))[0]
    low_rows = np.zeros((len(low), d), dtype=np.float32)
    low_rows[np.arange(len(low)), low] = -1.0
    high_rows = np.zeros((len(high), d), dtype=np.float32)
    high_rows[np.arange(len(high)), high] = 1.0
    return np.vstack(rows + [low_rows, high_rows]).astype(np.float32)


def vrp_gen_data(num_data: int, num_feat: int, n: int, deg: int = 4, noise_width: float = 0.5, seed: int = 42):
    """Features and edge costs of `tsp_gen_data`, and one demand vector for the data set drawn as the reference's CVRP
    test draws it (uniform on [0, 10), test/test_optmodel.py:111).  Returns (feats (N, p) float32, costs (N, d) float32,
    demands (n-1,) float32)."""
    feats, costs = tsp_gen_data(num_data, num_feat, n, deg=deg, noise_width=noise_width, seed=seed)
    demands = (np.random.RandomState(seed + 7919).rand(n - 1) * 10).astype(np.float32)
    return feats, costs, demands


def _vrp_dp_hip(who: str, entry: str, lo: int, hi: int, costs, n: int, demands, capacity: float, num_vehicle: int, eval_costs):
    """`vrp_solve_hip` and `vrp_solve_hip_wide`: the checks, the routes, the demands on the device and the launch of
    cave_hip_<entry>_solve."""
    import torch

    from . import _lib

    _lib.load()  # (no device: ImportError before any check of the arguments)
    n, K = int(n), int(num_vehicle)
    if not lo <= n <= hi:
        raise ValueError(f"{who}: the dynamic program on the device takes {lo} <= n <= {hi} nodes, not {n}")
    if not 1 <= K <= 8:
        raise ValueError(f"{who}: 1 <= num_vehicle <= 8, not {K}")
    capacity = float(capacity)
    if not (np.isfinite(capacity) and capacity > 0):
        raise ValueError(f"{who}: capacity must be finite and positive")
    d = n * (n - 1) // 2

    def own(N, dev):  # the routes, and the demands on the device
        q = demands if isinstance(demands, torch.Tensor) else torch.from_numpy(np.array(demands, dtype=np.float32))
        q = q.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if q.numel() != n - 1:
            raise ValueError(f"{who}: {n - 1} customers, {q.numel()} demands")
        return [torch.empty(N, n + K, dtype=torch.int32, device=dev), q]

    sols, objs, evals, bad, status, (routes, _) = _hip_solve(
        who, entry, costs, eval_costs, d, f"a CVRP on {n} nodes has {d} edges", own, (n, K),
        lambda solve, c, e, N, s, o, ev, st, x, ws, wsb, stream: solve(c, e, x[1], capacity, K, N, n, s, o, ev, x[0], st, ws, wsb, stream))
    if bad is not None:
        if int(status[bad]) == _lib.ST_INFEASIBLE:
            raise ValueError(f"{who}: instance {bad} is infeasible (no partition into feasible routes)")
        raise ValueError(f"{who}: instance {bad} has a non-finite cost, or a demand is negative or non-finite")
    return (sols, objs, routes) if eval_costs is None else (sols, objs, routes, evals)


def vrp_solve_hip(costs, n: int, demands, capacity: float, num_vehicle: int, eval_costs=None):
    """`vrp_solve` for a batch on the device: costs (N, d) float32, d = n (n-1) / 2, 3 <= n <= 14, demands (n-1,) shared
    by the batch (taken as float32), 1 <= num_vehicle <= 8 -> (sols (N, d) float32 0/1, objs (N,) float64, routes
    (N, n + num_vehicle) int32: `0, customers of route 1, 0, ..., 0`, then -1), equal to the host's bit for bit.  With
    `eval_costs` (N, d) a fourth result: evals (N,) float64, the routes priced under the second cost tensor (the regret
    numerator; the fp64 sum of their edges in route order).  Tables that do not fit the LDS lie in a workspace that is
    allocated here for the call (at most 512 slots).  A non-finite cost, a negative or non-finite demand or an
    infeasible instance raises ValueError."""
    return _vrp_dp_hip("vrp_solve_hip", "vrp_dp", 3, 14, costs, n, demands, capacity, num_vehicle, eval_costs)


def vrp_solve_hip_wide(costs, n: int, demands, capacity: float, num_vehicle: int, eval_costs=None):
    """`vrp_solve_hip` for 13 <= n <= 20 (cave_hip_vrp_dp_wide_solve, cave_amd/csrc/vrp_dp_wide.h): the same arguments,
    checks, results and errors, the same recurrences bit for bit -- beyond the host solver's 14 nodes, what `vrp_solve`
    would return if it went that far.  The tables always lie in a workspace that is allocated here for the call: one
    slot per workgroup of (n-1) 2^(n-2) doubles for the Held-Karp table and (min(K, (n-1)/2) - 1) 2^(n-1) doubles for the
    route costs and the stored layers (39.8 MB + 4.2 MB per layer at n = 20), min(N, 512, 8 GiB / slot) of them, behind a
    4 * 2^(n-1)-byte list.  The work of a stored layer is 3^(n-1) / 2 table pairs per instance: none at K = 2, one layer
    at K = 3."""
    return _vrp_dp_hip("vrp_solve_hip_wide", "vrp_dp_wide", 13, 20, costs, n, demands, capacity, num_vehicle, eval_costs)


def _vrp_solve_hip_for(n: int):
    """the device entry `vrp_regret(device=)` and `VRPConeDataset(device=)` take: the first tier up to 14 nodes, the wide
    one from 15 to 20"""
    return vrp_solve_hip if int(n) <= 14 else vrp_solve_hip_wide


class VRPConeDataset:
    """`optDatasetConstrs` (src/dataset.py:26-130) for the reference's `vrpModel` without Gurobi: sols and objs from the
    dynamic program (`vrp_solve`; on the device with `device`, `vrp_solve_hip` up to 14 nodes and `vrp_solve_hip_wide`
    from 15 to 20, beyond the host solver's reach), cuts from the cutting loop
    (`vrp_rcc_cuts`, host), rows those tight at the dynamic program's vertex -- a cut is a valid inequality, so it is a
    valid generator at any vertex where it is tight.  An infeasible instance raises ValueError, as the reference does
    without `skip_infeas`.

    `cones="sparse"` (needs `device`): the device solver's vertices stay on the device and the tight cones are written
    there by `tight_cones_hip` from `vrp_system` and the cuts as sparse lazy rows (`cut_rows`): no dense `ctrs` list,
    feats, costs, sols and objs on the device, `.cones` the SparseCones of the whole set, item i its one-instance slice.
    The default, `cones="dense"`, is what it always was."""

    def __init__(self, feats: np.ndarray, costs: np.ndarray, n: int, demands, capacity: float, num_vehicle: int, device=None,
                 cones: str = "dense"):
        import torch

        self.n, self.capacity, self.num_vehicle = n, float(capacity), int(num_vehicle)
        self.demands = np.asarray(demands, dtype=np.float32).reshape(-1)
        costs = np.asarray(costs, dtype=np.float32)
        if cones not in ("dense", "sparse"):
            raise ValueError(f"VRPConeDataset: cones must be 'dense' or 'sparse', not {cones!r}")
        self.cones = None
        if cones == "sparse":
            if device is None:
                raise ValueError("VRPConeDataset: cones='sparse' writes the cones on the device and needs `device`")
            device = torch.device(device)
            s, o, _ = _vrp_solve_hip_for(n)(torch.as_tensor(costs).to(device), n, self.demands, capacity, num_vehicle)
            cuts = [vrp_rcc_cuts(c, n, self.demands, capacity, num_vehicle)[2] for c in costs]
            made, n_rows = _tight_cones_call(vrp_system(n, num_vehicle), s, cut_rows(n, cuts), 1e-5)
            _device_cone_items(self, device, feats, costs, s, o.cpu().numpy(), made)
            depot = ((s[:, :n - 1].to(torch.float64).sum(1) - 2.0 * self.num_vehicle).abs() < 1e-5).to(torch.int32)  # its row is tight
            self.tight_cuts = [int(v) for v in (n_rows - depot - 2 * (n - 1) - s.shape[1]).tolist()]
            return
        if device is not None:
            s, o, _ = _vrp_solve_hip_for(n)(torch.as_tensor(costs).to(torch.device(device)), n, self.demands, capacity, num_vehicle)
            sols, objs = list(s.cpu().numpy()), [[float(v)] for v in o.cpu().numpy()]
        else:
            sols, objs = [], []
            for c in costs:
                s, o, _ = vrp_solve(c, n, self.demands, capacity, num_vehicle)
                sols.append(s)
                objs.append([o])
        ctrs, ncuts = [], []
        for c, s in zip(costs, sols):
            cuts = vrp_rcc_cuts(c, n, self.demands, capacity, num_vehicle)[2]
            A = vrp_tight_normals(s, n, cuts, num_vehicle)
            ctrs.append(A)
            ncuts.append(int(sum(abs(rhs - float(_cut_row(comp, _edge_index(n)[1], len(s)) @ s)) < 1e-5 for comp, rhs in cuts)))
        self.feats = torch.as_tensor(feats, dtype=torch.float32)
        self.costs = torch.as_tensor(costs, dtype=torch.float32)
        self.sols = torch.as_tensor(np.stack(sols), dtype=torch.float32)
        self.objs = torch.as_tensor(np.asarray(objs), dtype=torch.float32)
        self.ctrs = [torch.as_tensor(c, dtype=torch.float32) for c in ctrs]
        self.tight_cuts = ncuts

    def __len__(self) -> int:
        return len(self.feats)

    def __getitem__(self, i: int):
        if self.cones is not None:
            return _device_cone_item(self, i)
        return self.feats[i], self.costs[i], self.sols[i], self.objs[i], self.ctrs[i]


def vrp_regret(pred_costs: np.ndarray, true_costs: np.ndarray, true_objs: np.ndarray, n: int, demands, capacity: float,
               num_vehicle: int, device=None) -> float:
    """Normalised regret sum(c . w(c_hat) - z*) / sum(z*) with w(.) from `vrp_solve`.

    With `device`: arrays or tensors, moved to the device if they are not there; solved and priced there in one launch
    (fp64 sums), only the scalar comes back.  Up to 14 nodes through `vrp_solve_hip`, 15 to 20 through
    `vrp_solve_hip_wide`; without a device the host solver's limit of 14 nodes holds."""
    demands = np.asarray(demands.detach().cpu() if hasattr(demands, "detach") else demands, dtype=np.float32).reshape(-1)
    if device is not None:
        solve = _vrp_solve_hip_for(n)
        return _regret_hip(lambda cp, c: solve(cp, n, demands, capacity, num_vehicle, eval_costs=c)[3], pred_costs, true_costs,
                           true_objs, device)
    loss = 0.0
    for cp, c, z in zip(pred_costs, true_costs, true_objs):
        s, _, _ = vrp_solve(cp, n, demands, capacity, num_vehicle)
        loss += float(c @ s) - float(np.asarray(z).reshape(-1)[0])
    return loss / float(np.abs(true_objs).sum() + 1e-7)


# ------------------------------------------------------------------ tight cones of any binary LP, on the device

_SENSES = {"<": 0, "<=": 0, "L": 0, 0: 0, ">": 1, ">=": 1, "G": 1, 1: 1, "=": 2, "==": 2, "E": 2, 2: 2}
MAX_DIM = 65535  # columns of a system and rows of a cone (16 bits each in a key)


class LinSystem:
    """A constraint system `A x (sense) rhs` in the CSR form the tight-cone kernels read (`struct cave_lin_system`,
    include/cave_hip.h): what a Gurobi model hands out as `getA()` restricted to the cost columns, `Sense` and `RHS`.

    `A`: a scipy.sparse matrix or a dense (R, d) array; `senses`: one of '<', '>', '=' per row (Gurobi's characters; also
    '<=', '>=', '==' and the codes 0, 1, 2) or one for all rows; `rhs`: a number per row or one for all.  Canonicalised on
    the host once: coefficients as float32, columns sorted within a row, repeated entries summed, explicit zeros dropped.
    `to(device)` moves the five arrays there once (cached per device)."""

    def __init__(self, A, senses, rhs):
        from scipy.sparse import csr_matrix, issparse

        if issparse(A):
            M = csr_matrix(A, dtype=np.float64, copy=True)
        else:
            a = np.asarray(A, dtype=np.float64)
            if a.ndim != 2:
                raise ValueError("LinSystem: A must be a scipy.sparse matrix or a dense (R, d) array")
            M = csr_matrix(a)
        R, d = M.shape
        if not 1 <= d <= MAX_DIM:
            raise ValueError(f"LinSystem: need 1 <= d <= {MAX_DIM} columns, not {d}")
        M.sum_duplicates()
        M.data = M.data.astype(np.float32).astype(np.float64)  # (a value that underflows in float32 is an explicit zero)
        M.eliminate_zeros()
        M.sort_indices()
        if not np.isfinite(M.data).all():
            raise ValueError("LinSystem: a coefficient is not finite")
        if isinstance(senses, (str, bytes, int, np.integer)):
            senses = [senses] * R
        senses = [s.decode() if isinstance(s, bytes) else (int(s) if isinstance(s, np.integer) else s) for s in senses]
        if len(senses) != R:
            raise ValueError(f"LinSystem: {R} rows, {len(senses)} senses")
        for s in senses:
            if not isinstance(s, (str, int)) or s not in _SENSES:
                raise ValueError(f"Invalid constraint sense {s!r}.")  # (the reference's message, src/dataset.py:176)
        rhs = np.asarray(rhs, dtype=np.float64)
        rhs = np.full(R, float(rhs)) if rhs.ndim == 0 else rhs.reshape(-1).copy()
        if len(rhs) != R:
            raise ValueError(f"LinSystem: {R} rows, {len(rhs)} right-hand sides")
        if not np.isfinite(rhs).all():
            raise ValueError("LinSystem: a right-hand side is not finite")
        self.R, self.d = int(R), int(d)
        self.row_off = M.indptr.astype(np.int64)
        self.col = M.indices.astype(np.int32)
        self.coef = M.data.astype(np.float32)
        self.sense = np.array([_SENSES[s] for s in senses], dtype=np.int8)
        self.rhs = rhs
        self._dev: dict = {}

    @property
    def nnz(self) -> int:
        return int(self.col.size)

    def dense(self) -> np.ndarray:
        """the (R, d) float32 matrix (tests, small systems)"""
        a = np.zeros((self.R, self.d), dtype=np.float32)
        a[np.repeat(np.arange(self.R), np.diff(self.row_off)), self.col] = self.coef
        return a

    def to(self, device):
        """-> (struct cave_lin_system over this system's arrays on `device`, the tensors it points to); moved once"""
        import torch

        from . import _lib

        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._dev.get(device)
        if hit is None:
            t = [torch.from_numpy(a).to(device) for a in (self.row_off, self.col, self.coef, self.sense, self.rhs)]
            c = _lib.LinSystemC(R=self.R, Z=self.nnz, d=self.d, reserved=0, row_off=t[0].data_ptr(), col=t[1].data_ptr(),
                                coef=t[2].data_ptr(), sense=t[3].data_ptr(), rhs=t[4].data_ptr())
            hit = self._dev[device] = (c, t)
        return hit


def _edge_rows(n: int):
    """the node-edge incidence of the complete graph on n nodes in CSR form: row v holds its n-1 edges, ascending"""
    from scipy.sparse import csr_matrix

    from .synth import tsp_edges

    edges = tsp_edges(n)
    d = len(edges)
    return csr_matrix((np.ones(2 * d), (np.r_[edges[:, 0], edges[:, 1]], np.r_[np.arange(d), np.arange(d)])), shape=(n, d))


def tsp_system(n: int) -> LinSystem:
    """The explicit rows of the DFJ model (src/model/tsp.py:54-60): every node's degree == 2."""
    return LinSystem(_edge_rows(int(n)), "=", 2.0)


def vrp_system(n: int, num_vehicle: int) -> LinSystem:
    """The explicit rows of `vrpModel` (src/model/vrp.py): depot degree <= 2K, every customer's degree == 2."""
    n = int(n)
    return LinSystem(_edge_rows(n), ["<"] + ["="] * (n - 1), [2.0 * int(num_vehicle)] + [2.0] * (n - 1))


def sp_system(h: int, w: int) -> LinSystem:
    """The explicit rows of the grid shortest-path model: flow conservation per node (+1 on the arcs entering it, -1 on
    those leaving it) == -1 at the source, +1 at the sink, 0 elsewhere."""
    from scipy.sparse import csr_matrix

    arcs = sp_arcs(h, w)
    d, nn = len(arcs), h * w
    A = csr_matrix((np.r_[np.ones(d), -np.ones(d)], (np.r_[arcs[:, 1], arcs[:, 0]], np.r_[np.arange(d), np.arange(d)])), shape=(nn, d))
    rhs = np.zeros(nn)
    rhs[0], rhs[nn - 1] = -1.0, 1.0
    return LinSystem(A, "=", rhs)


def cut_rows(n: int, cuts_per_instance, sense="<"):
    """Lazy rows from node sets, built sparse: per instance a list of cuts, a cut being a node list S -- the subtour row
    x(E(S)) <= |S| - 1 of `tsp_dfj_cuts` -- or a pair (S, rhs) as `vrp_rcc_cuts` returns.  -> (LinSystem of all the rows
    in list order, lazy_off (N+1,) int64): what `tight_cones_hip(..., lazy=)` takes.  Edge columns as everywhere here:
    lexicographic (i < j)."""
    from scipy.sparse import csr_matrix

    n = int(n)
    d = n * (n - 1) // 2
    cols, ptr, rhs, off = [], [0], [], [0]
    for cuts in cuts_per_instance:
        for cut in cuts:
            pair = isinstance(cut, tuple) and len(cut) == 2 and not np.isscalar(cut[0])
            comp = np.unique(np.asarray(cut[0] if pair else cut, dtype=np.int64))
            if comp.size and (comp[0] < 0 or comp[-1] >= n):
                raise ValueError(f"cut_rows: a node outside 0..{n - 1}")
            a, b = np.triu_indices(comp.size, 1)
            a, b = comp[a], comp[b]
            cols.append(a * n - a * (a + 1) // 2 + b - a - 1)  # ascending: (a, b) runs in lexicographic order
            ptr.append(ptr[-1] + a.size)
            rhs.append(float(cut[1]) if pair else comp.size - 1.0)
        off.append(len(rhs))
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    A = csr_matrix((np.ones(cols.size), cols, np.asarray(ptr, dtype=np.int64)), shape=(len(rhs), d))
    return LinSystem(A, sense, np.asarray(rhs, dtype=np.float64)), np.asarray(off, dtype=np.int64)


def _tight_cones_call(system: LinSystem, sols, lazy, tol: float):
    """count pass, prefix sums, one host read, fill pass -> (SparseCones on the device, n_rows (N,) int32 there)"""
    import ctypes as C

    import torch

    from . import _lib
    from .sparse import SparseCones

    lib = _lib.load()  # (no device: ImportError before any check of the arguments)
    if not isinstance(system, LinSystem):
        raise TypeError("tight_cones_hip: system must be a LinSystem")
    if not (isinstance(sols, torch.Tensor) and sols.is_cuda and sols.dtype == torch.float32 and sols.dim() == 2):
        raise ValueError("tight_cones_hip: sols must be a (N, d) float32 tensor on the device")
    if sols.shape[1] != system.d:
        raise ValueError(f"tight_cones_hip: the system has {system.d} columns, sols has {sols.shape[1]}")
    tol = float(tol)
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("tight_cones_hip: tol must be finite and >= 0")
    sols = sols.contiguous()
    N, dev = sols.shape[0], sols.device
    sys_c, _keep = system.to(dev)
    lazy_c, lazy_off = None, None
    if lazy is not None:
        lz, off = lazy
        off = off if isinstance(off, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64))
        if not isinstance(lz, LinSystem) or lz.d != system.d:
            raise ValueError("tight_cones_hip: lazy must be (LinSystem over the same columns, lazy_off)")
        if off.numel() != N + 1:
            raise ValueError(f"tight_cones_hip: lazy_off must hold N + 1 = {N + 1} offsets")
        lazy_c, _keep_lazy = lz.to(dev)
        lazy_off = off.to(device=dev, dtype=torch.int64).contiguous()
    n_rows = torch.empty(N, dtype=torch.int32, device=dev)
    n_ent = torch.empty(N, dtype=torch.int64, device=dev)
    status = torch.empty(N, dtype=torch.int32, device=dev)
    ent_off = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    p = _lib.ptr
    ref = lambda c: None if c is None else C.byref(c)  # noqa: E731
    with torch.cuda.device(dev):
        stream = _lib.current_stream()
        _lib.check(lib.cave_hip_tight_cones_count(ref(sys_c), ref(lazy_c), p(lazy_off), p(sols), N, tol, p(n_rows), p(n_ent),
                                                  p(status), stream), "cave_hip_tight_cones_count")
        if N:
            torch.cumsum(n_ent, 0, out=ent_off[1:])
            total, m_max, failed = (int(v) for v in torch.stack([ent_off[-1], n_rows.max().to(torch.int64),
                                                                  (status != _lib.ST_OK).any().to(torch.int64)]).tolist())
        else:
            total, m_max, failed = 0, 0, 0
        if failed:
            bad = int(torch.nonzero(status != _lib.ST_OK)[0])
            if int(status[bad]) == _lib.ST_TOO_LARGE:
                raise ValueError(f"tight_cones_hip: instance {bad} has more than {MAX_DIM} tight rows")
            raise ValueError(f"tight_cones_hip: instance {bad} has a non-finite solution value or a lazy row that breaks the "
                             "contract of cave_lin_system (or the shared system does)")
        key = torch.empty(total, dtype=torch.int32, device=dev)
        val = torch.empty(total, dtype=torch.float32, device=dev)
        _lib.check(lib.cave_hip_tight_cones_fill(ref(sys_c), ref(lazy_c), p(lazy_off), p(sols), N, tol, p(ent_off), total,
                                                 p(key), p(val), None, stream), "cave_hip_tight_cones_fill")
    return SparseCones(m_max, system.d, ent_off, key, val), n_rows


def tight_cones_hip(system: LinSystem, sols, lazy=None, tol: float = 1e-5):
    """`_extract_tight_normals` (src/dataset.py:147-215) for a batch of vertices on the device: sols (N, d) float32 there,
    `system` the model's explicit rows, `lazy` None or `(LinSystem, lazy_off)` -- the rows lazy_off[b]:lazy_off[b+1] are
    instance b's lazy constraints (`cut_rows` builds the pair from node sets) -> the SparseCones
    `SparseCones.from_ragged([that function's matrix per instance])` holds, on the device, without the dense matrix:
    count pass, `torch.cumsum`, one host read (the total and the largest row count), fill pass.  Limits: d <= 65535
    columns, 65535 rows per instance.  The first instance the device rejects raises ValueError."""
    return _tight_cones_call(system, sols, lazy, tol)[0]


def _device_cone_items(self, device, feats, costs, sols, objs, cones):
    """what the `device=` forms of the TSP and CVRP data sets keep: everything on the device, the whole set's cones, and
    the offsets that slice an item's cone out of them (instances differ in size)"""
    import torch

    self.feats = torch.as_tensor(feats, dtype=torch.float32).to(device)
    self.costs = torch.as_tensor(costs, dtype=torch.float32).to(device)
    self.sols = sols
    self.objs = torch.as_tensor(np.asarray(objs), dtype=torch.float32).reshape(-1, 1).to(device)
    self.cones = cones
    self._ent = [int(v) for v in cones.ent_off.tolist()]
    z = torch.zeros(len(self._ent) - 1, dtype=torch.int64, device=device)
    self._off2 = torch.stack([z, cones.ent_off[1:] - cones.ent_off[:-1]], dim=1)  # row i: the ent_off of item i's cone


def _device_cone_item(self, i: int):
    from .sparse import SparseCones

    i = int(i) % len(self)
    lo, hi = self._ent[i], self._ent[i + 1]
    cone = SparseCones(self.cones.m_max, self.cones.d, self._off2[i], self.cones.key[lo:hi], self.cones.val[lo:hi])
    return self.feats[i], self.costs[i], self.sols[i], self.objs[i], cone
