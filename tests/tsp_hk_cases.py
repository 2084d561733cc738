"""Cases of the Held-Karp kernels (cave_amd/csrc/tsp_hk.h), shared by the CPU tier (tests/test_tsp_hk_emul.py: the kernels
under the SIMT emulation) and the GPU tier (tests/test_gpu_tsp_hk.py).

The oracle is the project's own host code, tight.tsp_solve.  Host results are computed once per (n, cost kind, N) and
shared.

Bounds (derived, not measured):
  * objs, tours and sols: EQUAL.  The device performs the host's fp64 additions and strict comparisons in the host's
    candidate order; the entries of one cardinality are independent, so no other order shows.
  * evals: EQUAL to the fp64 sum of the tour's n edge costs under eval_costs in tour order, left to right, the closing
    edge last (`tour_eval`): the device performs exactly these additions.
  * tsp_regret(device=) against the host's: n 2^-23 sum_i sum_k |c_ik| sol_ik / sum_i |z_i| (`regret_bound`).  The host
    prices a tour with a float32 dot product of n non-zero terms (the zero terms add exactly): n - 1 roundings of at most
    2^-24 of a partial sum, each partial sum at most sum_k |c_k| sol_k (1 + 2^-24)^n -- so (n - 1) 2^-24 (1 + ..) per
    instance, and n 2^-23 is that with a factor two of margin; float(z) and the fp64 sums on either side round below
    2^-50 of it.  The same derivation as the shortest-path test's.
"""

from __future__ import annotations

import numpy as np

from cave_amd import tight

ST_OK, ST_BAD_INPUT = 0, 3
E_INVALID = -1
MAX_LDS = 160 * 1024
DEFAULT_SLOTS = 512


def n_edges(n):
    return n * (n - 1) // 2


def eid(i, j, n):
    i, j = min(i, j), max(i, j)
    return i * n - i * (i + 1) // 2 + j - i - 1


def _r16(x):
    return (x + 15) & ~15


def table_bytes(n):
    """(n-1) 2^(n-2) doubles: the entries (S, j) with j in S"""
    return 8 * (n - 1) * 2 ** (n - 2)


def _fixed_lds(n):
    """D, two 16-double arrays, the binomials, the class offsets, two 16-int arrays, the staged costs, the solution, the
    popcount-sorted list -- each rounded up to 16 bytes (cave_amd/csrc/tsp_hk.h)"""
    d = n_edges(n)
    return _r16(8 * n * n) + 128 + 128 + _r16(2 * 14 * 14) + 32 + 64 + 64 + 2 * _r16(4 * d) + _r16(2 * 2 ** (n - 2))


def in_lds(n):
    return _fixed_lds(n) + table_bytes(n) <= MAX_LDS


def lds_bytes(n):
    """LDS of one workgroup: the small arrays, and the table where all of it fits 160 KiB"""
    return _fixed_lds(n) + (table_bytes(n) if in_lds(n) else 0)


def slot_bytes(n):
    """include/cave_hip.h: 0 where the table lies in LDS, else the table's bytes; -1 for an n out of range"""
    if n < 3 or n > 14:
        return E_INVALID
    return 0 if in_lds(n) else table_bytes(n)


def workspace_bytes(n, N):
    if n < 3 or n > 14 or N < 0:
        return E_INVALID
    return slot_bytes(n) * min(N, DEFAULT_SLOTS)


LDS_MAX_N = max(n for n in range(3, 15) if slot_bytes(n) == 0)   # 12
WS_MIN_N = LDS_MAX_N + 1                                           # 13

# n -> batch size: the smallest tables (m = 2), entries below / not a multiple of the workgroup, the LDS limit, the first
# global-tier size, the cap (0.2 s per instance on the host)
SHAPES = {3: 5, 4: 5, 7: 5, 8: 5, LDS_MAX_N: 4, WS_MIN_N: 4, 14: 3}
KINDS = ("gen", "ties", "signed")


def costs_of(kind, N, n, seed=0):
    d = n_edges(n)
    rng = np.random.default_rng(100 * n + 7919 * seed + 1)
    if kind == "gen":  # the data generator's draws
        return tight.tsp_gen_data(N, 5, n, seed=42 + seed)[1]
    if kind == "ties":  # integer costs from {1, 2, 3}: nearly every minimum is tied, the tie rule decides the tour
        return rng.integers(1, 4, (N, d)).astype(np.float32)
    if kind == "signed":  # costs of both signs (a tour has n edges whatever their signs)
        c = rng.standard_normal((N, d)).astype(np.float32)
        c[: N // 3] = -np.abs(c[: N // 3])
        return c
    raise KeyError(kind)


_HOST = {}


def host(kind, n, N=None, seed=0):
    """(costs, sols, objs, tours) of the host solver, cached"""
    N = SHAPES[n] if N is None else N
    k = (kind, n, N, seed)
    if k not in _HOST:
        c = costs_of(kind, N, n, seed)
        r = [tight.tsp_solve(ci, n) for ci in c]
        _HOST[k] = (c, np.stack([s for s, _, _ in r]), np.asarray([o for _, o, _ in r], np.float64),
                    np.asarray([t for _, _, t in r], np.int32).reshape(N, n))
        for a in _HOST[k]:
            a.setflags(write=False)
    return _HOST[k]


def tour_eval(eval_costs, tours, n):
    """the fp64 sum of eval_costs over the tour's n edges in tour order, left to right, the closing edge last"""
    out = np.empty(len(tours), np.float64)
    for b, t in enumerate(tours):
        acc = np.float64(0.0)
        for i in range(n):
            acc = acc + np.float64(eval_costs[b, eid(int(t[i]), int(t[(i + 1) % n]), n)])
        out[b] = acc
    return out


def regret_bound(true, psols, z, n):
    return n * 2.0 ** -23 * (np.abs(true.astype(np.float64)) * psols).sum() / np.abs(z.astype(np.float64)).sum()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check_solve(o, sols, objs, tours, n, eval_costs=None, what=""):
    """a batch of device outputs (dict of numpy arrays; None entries were not requested) against the host's, bit for bit"""
    if o.get("status") is not None:
        assert o["status"].dtype == np.int32 and (o["status"] == ST_OK).all(), (what, o["status"])
    if o.get("sol") is not None:
        assert o["sol"].dtype == np.float32 and np.array_equal(bits(o["sol"]), bits(sols)), (what, "sol")
    if o.get("obj") is not None:
        assert o["obj"].dtype == np.float64 and np.array_equal(bits(o["obj"]), bits(objs)), (what, "obj", o["obj"], objs)
    if o.get("tour") is not None:
        assert o["tour"].dtype == np.int32 and np.array_equal(o["tour"], tours), (what, "tour", o["tour"], tours)
    if o.get("eval") is not None:
        ref = tour_eval(eval_costs, tours, n)
        assert o["eval"].dtype == np.float64 and np.array_equal(bits(o["eval"]), bits(ref)), (what, "eval", o["eval"], ref)


def bad_batch(n, N=6):
    """good `gen` instances with a NaN in instance 1 and an inf in instance 4 -> (costs, bad ids, host results of all N
    instances of the clean batch)"""
    c, sols, objs, tours = host("gen", n, N=N, seed=3)
    bad = c.copy()
    d = n_edges(n)
    bad[1, d - 1] = np.nan
    bad[4, 0] = np.inf
    return bad, (1, 4), (sols, objs, tours)


def check_bad(o, hit, ref, N, what=""):
    sols, objs, tours = ref
    ok = np.ones(N, bool)
    ok[list(hit)] = False
    assert (o["status"][~ok] == ST_BAD_INPUT).all() and (o["status"][ok] == ST_OK).all(), (what, o["status"])
    assert (o["sol"][~ok] == 0).all() and np.isnan(o["obj"][~ok]).all() and np.isnan(o["eval"][~ok]).all(), what
    assert (o["tour"][~ok] == -1).all(), what
    assert np.array_equal(o["sol"][ok], sols[ok]) and np.array_equal(bits(o["obj"][ok]), bits(objs[ok])), what
    assert np.array_equal(o["tour"][ok], tours[ok]), what
