"""A plain numpy restatement of the reference's extraction rule for tight constraint normals (`_extract_tight_normals`
and `_orient_row`, src/dataset.py:147-215 of the reference), on dense matrices: the oracle of the tight-cone kernels
(tests/tight_cones_cases.py) wherever no model-specific host function (`sp_tight_normals`, `tsp_tight_normals`,
`vrp_tight_normals`) applies.  TEST INFRASTRUCTURE ONLY.

The rule, per vertex x (taken to fp64) and tolerance tol, every block in `<=` orientation:
    the explicit rows with |rhs - a.x| < tol:  the `<=` ones, then the `>=` ones negated, then the `==` ones, then the
    `==` ones negated;   the lazy rows with |rhs - a.x| < tol in list order, `>=` negated, `==` as the row followed by its
    negation;   -e_k where x_k <= tol;   +e_k where x_k >= 1 - tol and not x_k <= tol.
"""

from __future__ import annotations

import numpy as np

LE, GE, EQ = 0, 1, 2


def oriented(row: np.ndarray, sense: int):
    """a row in `<=` orientation: one row, or two for an equality"""
    if sense == LE:
        return [row]
    if sense == GE:
        return [-row]
    if sense == EQ:
        return [row, -row]
    raise ValueError(f"Invalid constraint sense {sense!r}.")


def tight_normals(A, sense, rhs, lazy, sol, tol: float = 1e-5) -> np.ndarray:
    """A (R, d), sense (R,) codes, rhs (R,); lazy: a list of (row (d,), sense, rhs); sol (d,) -> (m, d) float32"""
    x = np.asarray(sol, dtype=np.float64)
    d = x.size
    blocks = []
    A = np.asarray(A, dtype=np.float64).reshape(-1, d)
    sense = np.asarray(sense).reshape(-1)
    if len(A):
        tight = np.abs(np.asarray(rhs, dtype=np.float64) - A @ x) < tol
        for code, sign in ((LE, 1.0), (GE, -1.0), (EQ, 1.0), (EQ, -1.0)):
            pick = tight & (sense == code)
            if pick.any():
                blocks.append(sign * A[pick])
    lazy_rows = []
    for row, s, r in lazy:
        row = np.asarray(row, dtype=np.float64)
        if abs(float(r) - float(row @ x)) < tol:
            lazy_rows += oriented(row, int(s))
    if lazy_rows:
        blocks.append(np.asarray(lazy_rows))
    low = x <= tol
    high = (x >= 1 - tol) & ~low
    for mask, v in ((low, -1.0), (high, 1.0)):
        idx = np.flatnonzero(mask)
        if len(idx):
            unit = np.zeros((len(idx), d))
            unit[np.arange(len(idx)), idx] = v
            blocks.append(unit)
    if not blocks:
        return np.zeros((0, d), dtype=np.float32)
    return np.vstack(blocks).astype(np.float32)
