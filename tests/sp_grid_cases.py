"""Cases of the grid shortest-path kernel (cave_amd/csrc/sp_grid.h), shared by the CPU tier (tests/test_sp_grid_emul.py:
the kernel under the SIMT emulation) and the GPU tier (tests/test_gpu_sp_grid.py).

The oracle is the project's own host code: tight.sp_solve for paths and objectives, tight.sp_tight_normals through
SparseCones.from_ragged for the cones.  Host results are computed once per (shape, cost kind) and shared.

Bounds (derived, not measured):
  * sols and objs: EQUAL.  The device performs the host's fp64 additions and strict comparisons in the host's order.
  * evals against costs.astype(float64) @ sol: (h + w) 2^-52 sum_k |c_k| sol_k -- an fp64 sum of h + w - 2 exactly
    converted fp32 terms in another order; each of the at most h + w - 3 additions rounds by 2^-53 of a partial sum.
  * cones: EQUAL as tensors.
"""

from __future__ import annotations

import numpy as np

from cave_amd import tight
from cave_amd.sparse import SparseCones
from cave_amd.synth import sp_arcs

ST_OK, ST_BAD_INPUT = 0, 3
E_INVALID = -1
MAX_LDS = 160 * 1024

# shape -> batch size.  30x30 keeps a small batch: its dense host cones are 24.6 MB each
SHAPES = {(1, 2): 64, (1, 7): 64, (7, 1): 64, (2, 2): 64, (5, 5): 64, (12, 12): 64, (30, 30): 12,
          (2, 64): 64, (2, 65): 64, (64, 2): 64, (65, 2): 64, (3, 70): 64, (70, 3): 64}
KINDS = ("gen", "ties", "signed", "spread")


def n_arcs(h, w):
    return h * (w - 1) + (h - 1) * w


def _r16(x):
    return (x + 15) & ~15


def lds_bytes(h, w):
    """LDS of one instance as include/cave_hip.h documents it: the costs, for w > 64 the fp64 column handed from strip to
    strip, a predecessor byte per node, each rounded up to 16 bytes; -1 beyond 160 KiB or for h w < 2"""
    if h < 1 or w < 1 or h * w < 2:
        return -1
    need = _r16(4 * n_arcs(h, w)) + (_r16(8 * h) if w > 64 else 0) + _r16(h * w)
    return need if need <= MAX_LDS else -1


def lds_limit_shapes(w=134):
    """(largest h that fits at this width, the next one): the shape at the LDS limit and the one just above"""
    h = 1
    while lds_bytes(h + 1, w) > 0:
        h += 1
    return (h, w), (h + 1, w)


def costs_of(kind, N, h, w, seed=0):
    d = n_arcs(h, w)
    rng = np.random.default_rng(1000 * h + w + 7919 * seed)
    if kind == "gen":  # the data generator's draws
        return tight.sp_gen_data(N, 5, h, w, seed=135 + seed)[1]
    if kind == "ties":  # integer costs from {1, 2}: equal path lengths at most nodes, the tie rule decides
        return rng.integers(1, 3, (N, d)).astype(np.float32)
    if kind == "signed":  # negative and mixed-sign costs (a DAG: no cycles to worry about)
        c = rng.standard_normal((N, d)).astype(np.float32)
        c[: N // 4] = -np.abs(c[: N // 4])
        return c
    if kind == "spread":  # magnitudes over e^-10 .. e^10
        return np.exp(rng.uniform(-10.0, 10.0, (N, d))).astype(np.float32)
    raise KeyError(kind)


_HOST = {}


def host(kind, h, w, N=None):
    """(costs, sols, objs) of the host solver, cached"""
    N = SHAPES[(h, w)] if N is None else N
    k = (kind, h, w, N)
    if k not in _HOST:
        c = costs_of(kind, N, h, w)
        so = [tight.sp_solve(ci, h, w) for ci in c]
        _HOST[k] = (c, np.stack([s for s, _ in so]), np.asarray([o for _, o in so], np.float64))
    return _HOST[k]


_CONES = {}


def host_cones(kind, h, w, N=None):
    """SparseCones.from_ragged of the host's tight normals at the host's solutions, cached (dense blocks one at a time)"""
    N = SHAPES[(h, w)] if N is None else N
    k = (kind, h, w, N)
    if k not in _CONES:
        sols = host(kind, h, w, N)[1]
        _CONES[k] = SparseCones.from_ragged(tight.sp_tight_normals(s, h, w) for s in sols)
    return _CONES[k]


def cone_coo(sol, h, w):
    """The entries of tight.sp_tight_normals(sol, h, w) without the dense matrix, as a SparseCones.from_coo item -- for
    the one shape whose dense block would not fit a host (128x128: 8.5 GB).  The tests check it against from_ragged on the
    small shapes before they rely on it."""
    arcs = sp_arcs(h, w)
    d, n = len(arcs), h * w
    k = np.arange(d)
    low, high = np.where(sol <= 1e-5)[0], np.where(sol >= 1 - 1e-5)[0]
    rows = np.r_[arcs[:, 1], arcs[:, 0], n + arcs[:, 1], n + arcs[:, 0], 2 * n + np.arange(len(low)), 2 * n + len(low) + np.arange(len(high))]
    cols = np.r_[k, k, k, k, low, high]
    vals = np.r_[np.ones(d), -np.ones(d), -np.ones(d), np.ones(d), -np.ones(len(low)), np.ones(len(high))].astype(np.float32)
    return rows, cols, vals, 2 * n + d


def eval_bound(costs, sols, h, w):
    return (h + w) * 2.0 ** -52 * (np.abs(costs.astype(np.float64)) * sols).sum(axis=1)


def check_solve(o, costs, sols, objs, h, w, eval_costs=None, what=""):
    """conditions 1 and 2 on one batch of device outputs (dict of numpy arrays; None entries were not requested)"""
    if o.get("status") is not None:
        assert (o["status"] == ST_OK).all(), (what, o["status"])
    if o.get("sol") is not None:
        assert o["sol"].dtype == np.float32 and np.array_equal(o["sol"], sols), (what, "sol")
    if o.get("obj") is not None:
        assert o["obj"].dtype == np.float64 and np.array_equal(o["obj"], objs), (what, "obj", np.abs(o["obj"] - objs).max())
    if o.get("eval") is not None:
        ref = (eval_costs.astype(np.float64) * sols).sum(axis=1)
        err, bound = np.abs(o["eval"] - ref), eval_bound(eval_costs, sols, h, w)
        assert (err <= bound).all(), (what, "eval", float((err - bound).max()))


def check_cones(key, val, ref: SparseCones, N, h, w, what=""):
    """condition 4 on flat key / val arrays of N instances"""
    d = n_arcs(h, w)
    assert ref.B == N and ref.d == d and ref.m_max == 2 * h * w + d, what
    assert np.array_equal(ref.ent_off.numpy(), 5 * d * np.arange(N + 1)), (what, "ent_off")
    assert np.array_equal(np.asarray(key).view(np.int32), ref.key.numpy()), (what, "key")
    assert np.array_equal(np.asarray(val), ref.val.numpy()), (what, "val")
