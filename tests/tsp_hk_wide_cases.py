"""Cases of the wide Held-Karp tier (cave_amd/csrc/tsp_hk_wide.h, 13 <= n <= 20), shared by the CPU tier
(tests/test_tsp_hk_wide_emul.py: the kernels under the SIMT emulation) and the GPU tier (tests/test_gpu_tsp_hk_wide.py).

Oracles.  Up to n = 14 the project's own host code, tight.tsp_solve (tests/tsp_hk_cases.py).  Beyond it the host solver
refuses, so `solve_ref` restates its recurrence in numpy, vectorised by cardinality: every entry (S, j) has one
predecessor set S \\ {j}, its candidates are dp[S \\ {j}, k] + D[k+1][j+1] -- the fp64 additions tight._held_karp performs,
with +inf for k outside the set -- and np.argmin over k takes the first minimum, as the host's does.  The closing edge and
the walk back use the stored argmins.  tests/test_tsp_hk_wide_emul.py asserts it against tight.tsp_solve bit for bit at
n <= 13.  For n = 18, 19, 20 (0.5 - 2 s per instance) its results are kept in tests/golden/tsp_hk_wide.npz, written by
tests/golden/make_tsp_hk_wide.py: per n one `gen`, one `ties` and one `signed` instance (costs, tours, objectives) and the
objective tight.tsp_dfj_cuts (HiGHS, another algorithm) finds for the `gen` one.

Bounds: as tests/tsp_hk_cases.py -- sols, objs, tours and evals EQUAL; the regret within `regret_bound`.
"""

from __future__ import annotations

import os

import numpy as np

import tsp_hk_cases as TC

E_INVALID = TC.E_INVALID
MIN_N, MAX_N = 13, 20
MAX_SLOTS, MAX_BYTES = 512, 8 << 30
KINDS = TC.KINDS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsp_hk_wide.npz")
GOLDEN_NS = (18, 19, 20)


def slot_bytes(n):
    """include/cave_hip.h: the table, (n-1) 2^(n-2) doubles; -1 for an n out of range"""
    return 8 * (n - 1) * 2 ** (n - 2) if MIN_N <= n <= MAX_N else E_INVALID


def header_bytes(n):
    """the popcount-sorted list of the (n-1)-bit numbers, uint32"""
    return 4 * 2 ** (n - 1)


def default_slots(n):
    return min(MAX_SLOTS, MAX_BYTES // slot_bytes(n))


def workspace_bytes(n, N):
    if not MIN_N <= n <= MAX_N or N < 0:
        return E_INVALID
    return header_bytes(n) + slot_bytes(n) * min(N, default_slots(n))


def lds_bytes(n):
    """cave_amd/csrc/tsp_hk_wide.h: D, the customers' block of D with an odd row stride, two 32-double arrays, the class
    offsets, the state, the tour, the staged costs, the solution -- each rounded up to 16 bytes"""
    r16, m, d = TC._r16, n - 1, TC.n_edges(n)
    return r16(8 * n * n) + r16(8 * m * (m | 1)) + 256 + 256 + 128 + 64 + 128 + 2 * r16(4 * d)


def solve_ref(cost, n):
    """tight.tsp_solve's recurrence for any n, vectorised by cardinality -> (sol (d,) float32, objective, tour list)"""
    m, d = n - 1, TC.n_edges(n)
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
    parent = np.full((full, m), -1, dtype=np.int8)
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
    last = dp[full - 1] + D[1:, 0]
    j = int(np.argmin(last))
    obj = float(last[j])
    walk, mask = [], full - 1
    while j >= 0:
        walk.append(j + 1)
        pj = int(parent[mask, j])
        mask ^= 1 << j
        j = pj
    tour = [0] + walk[::-1]
    sol = np.zeros(d, dtype=np.float32)
    for a, b in zip(tour, tour[1:] + tour[:1]):
        sol[TC.eid(a, b, n)] = 1.0
    return sol, obj, tour


def sols_of(tours, n):
    """0/1 edge indicators of tours"""
    s = np.zeros((len(tours), TC.n_edges(n)), np.float32)
    for b, t in enumerate(tours):
        for i in range(n):
            s[b, TC.eid(int(t[i]), int(t[(i + 1) % n]), n)] = 1.0
    return s


_REF = {}


def ref(kind, n, N, seed=0):
    """(costs, sols, objs, tours) of the restatement on tsp_hk_cases.costs_of(kind, N, n, seed), cached"""
    k = (kind, n, N, seed)
    if k not in _REF:
        c = TC.costs_of(kind, N, n, seed)
        r = [solve_ref(ci, n) for ci in c]
        _REF[k] = (c, np.stack([s for s, _, _ in r]), np.asarray([o for _, o, _ in r], np.float64),
                   np.asarray([t for _, _, t in r], np.int32).reshape(N, n))
        for a in _REF[k]:
            a.setflags(write=False)
    return _REF[k]


def golden_costs(n):
    """the fixture's three cost rows of n nodes: one per kind, in KINDS order"""
    return np.concatenate([TC.costs_of(kind, 1, n, seed=5) for kind in KINDS]).astype(np.float32)


_GOLD = {}


def golden(n):
    """(costs, sols, objs, tours, the DFJ loop's objective of row 0) of the committed fixture, n in GOLDEN_NS"""
    if n not in _GOLD:
        with np.load(GOLDEN) as z:
            c, t, o, f = z[f"costs{n}"], z[f"tours{n}"], z[f"objs{n}"], float(z[f"dfj{n}"])
        assert c.dtype == np.float32 and c.shape == (3, TC.n_edges(n)) and t.dtype == np.int32 and t.shape == (3, n) and o.dtype == np.float64
        _GOLD[n] = (c, sols_of(t, n), o, t, f)
        for a in _GOLD[n][:4]:
            a.setflags(write=False)
    return _GOLD[n]


def bad_batch(n, N=6):
    """good `gen` instances with a NaN in instance 1 and an inf in instance 4 -> (costs, bad ids, reference results of all N
    instances of the clean batch)"""
    c, sols, objs, tours = (TC.host if n <= 14 else ref)("gen", n, N=N, seed=3)
    bad = c.copy()
    bad[1, TC.n_edges(n) - 1] = np.nan
    bad[4, 0] = np.inf
    return bad, (1, 4), (sols, objs, tours)
