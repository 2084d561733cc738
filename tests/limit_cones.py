"""+-1 cones that sit ON the limits of the one-wave "lite" solver (TEST INFRASTRUCTURE; numpy only, seeded).

The solver behind the fused step kernel (cave_amd/csrc/cone_step.h, include/cave_hip.h) takes cones with d <= 256,
<= 32 reduced rows ordered [free | <= 8 bound rows], <= 8 entries per column and <= 1536 non-zeros -- and, since the
slot header and the solve half were made to agree, only those whose active-set scratch fits the arena of a solve-only
launch (`scratch_fits` below restates the rule; the tests check it against the kernel, not the other way round).
TSP-20 / TSP-12 / SP 5x5, the structured cones of the rest of the suite, stay far from every one of these limits.

A cone is drawn as `n_free + n_bound` rows with entries in {-1, +1}: row by row, each row takes the currently emptiest
columns that still hold fewer than `col_cap` entries.  The dense block is
    [rows[:n_free], -rows[:n_free], rows[n_free:], unit rows +-e_k on about half of the coordinates], zero-padded:
a +a / -a pair is ONE reduced row with a free multiplier, a single row one with a non-negative multiplier.
"""

from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class Case:
    name: str
    d: int
    n_free: int
    n_bound: int
    nnz: int            # non-zeros of the reduced rows (a free row counts once)
    col_cap: int = 8
    kind: str = "in"    # "in": the lite solver takes it;  "out": refused by a documented limit;
    #                     "scratch": within the documented limits, refused because the active-set scratch does not fit
    defect: str = ""    # how an "out" cone is spoiled (see _spoil)
    unit_share: float = 0.5  # share of the coordinates that get a unit row
    what: str = ""

    @property
    def p(self):
        return self.n_free + self.n_bound

    @property
    def chn8(self):
        return 8 if self.nnz <= 512 else (16 if self.nnz <= 1024 else 24)


def scratch_doubles(p, nI):
    """doubles of scratch the active-set loop needs (cone_step.h: XS, S, four vectors, flags)"""
    return p * nI + nI * (nI | 1) + 4 * nI + (nI + 7) // 8


IN_CASES = [
    Case("d256_16f8b_1536", 256, 16, 8, 1536, what="d, bound rows, non-zeros, chn8 = 24 at once; KC slot 4; own scratch block (297 > d)"),
    Case("d256_27f5b_1536", 256, 27, 5, 1536, what="p = 32 (ldh = 33, lane 32 holds mptr[p]); scratch in tvec (206)"),
    Case("d255_25f6b_1056", 255, 25, 6, 1056, what="odd d, partial fourth slot, chn8 = 24 just above 1024; scratch 253 <= d"),
    Case("d193_19f8b_1027", 193, 19, 8, 1027, what="first d with a fourth slot; uneven rows; 8 bound rows, own scratch block"),
    Case("d256_21f7b_1400", 256, 21, 7, 1400, what="accepted side of the scratch rule: 28 rows / 7 bound rows (274 doubles, own block)"),
    Case("d256_19f8b_1350", 256, 19, 8, 1350, what="accepted side of the scratch rule: 27 rows / 8 bound rows (321 doubles, own block)"),
    Case("d256_25f6b_1488", 256, 25, 6, 1488, what="31 rows / 6 bound rows: 253 doubles, the last that tvec holds at d = 256"),
    Case("d256_16f8b_1024", 256, 16, 8, 1024, what="chn8 = 16 exactly at its upper edge"),
    Case("d256_16f8b_512", 256, 16, 8, 512, what="chn8 = 8 exactly at its upper edge"),
    Case("d64_8f8b_512", 64, 8, 8, 512, what="every column full (no dummy slot in any ell word); need 233 >> d"),
    Case("d256_32f0b_1536", 256, 32, 0, 1536, what="32 free rows, no bound rows"),
    Case("d256_0f8b_1200", 256, 0, 8, 1200, what="no free rows"),
    Case("d40_0f1b_2", 40, 0, 1, 2, what="smallest system: one bound row of two entries"),
    Case("d40_1f0b_2", 40, 1, 0, 2, what="smallest system: one free row of two entries"),
]
SCRATCH_CASES = [
    Case("d256_24f8b_1536", 256, 24, 8, 1536, kind="scratch", what="every documented limit at once: scratch 361 doubles"),
    Case("d256_26f6b_1536", 256, 26, 6, 1536, kind="scratch", what="p = 32, 6 bound rows: scratch 259 doubles, d = 256"),
    Case("d256_20f8b_1400", 256, 20, 8, 1400, kind="scratch", what="just beyond the rule: 28 rows / 8 bound rows"),
    Case("d256_22f7b_1450", 256, 22, 7, 1450, kind="scratch", what="just beyond the rule: 29 rows / 7 bound rows"),
    Case("d120_24f8b_960", 120, 24, 8, 960, kind="scratch", what="p = 32, 8 bound rows at a small d"),
    Case("d253_23f8b_1240", 253, 23, 8, 1240, kind="scratch", what="the shape of TSP-23 with 8 cuts: p = 31"),
]

OUT_CASES = [
    Case("d200_25f8b", 200, 25, 8, 990, kind="out", what="33 reduced rows"),
    Case("d200_20f9b", 200, 20, 9, 870, kind="out", what="9 bound rows"),
    Case("d64_col9", 64, 8, 8, 480, kind="out", defect="col9", what="one column of 9 entries"),
    Case("d256_1568", 256, 24, 8, 1568, kind="out", what="49 per row: 1568 non-zeros"),
    Case("d200_order", 200, 10, 4, 420, kind="out", defect="order", what="a +a / -a pair after the bound rows"),
    Case("d200_two", 200, 10, 4, 420, kind="out", defect="two", what="one entry 2.0"),
]


def solve_lds_bytes(d):
    """LDS of a solve-only launch at dimension d, restated (step_solve_lds_bytes of cone_step.h; tests/test_step_emul.py
    compares the two for every d)"""
    a8 = lambda x: (x + 7) & ~7
    P = 32
    s = 64 + 2 * a8(4 * d) + a8(d) + a8(4 * (P + 1)) + a8(P)
    s += 16 + 16 * d + 16 + 4 * 768 + 8 * (33 + 64 + 65) + 40
    s += 2 * a8(8 * d) + a8(8 * (d + 1)) + a8(4 * d)
    s += 2 * 8 * 33 + 5 * a8(8 * P) + a8(8 * P * (P | 1)) + a8(P) + 64
    return (s + 255) & ~255


def solve_arena_left(d, p):
    """bytes the solve half's arena has left for the scratch block in a SOLVE-ONLY launch, p reduced rows (replays the
    allocations of run_lite_instance against solve_lds_bytes(d) - 64; every mode, 24 entries per lane)"""
    a8 = lambda x: (x + 7) & ~7
    a16 = lambda x: (x + 15) & ~15
    cap = solve_lds_bytes(d) - 64
    pp = max(p, 1)
    off = 0
    for nbytes, al in ((4 * d, 8), (4 * d, 8), (d, 8), (4 * (pp + 1), 8), (pp, 8), (16 * d, 16), (128 * 24, 16),
                       (8 * 162, 8), (40, 8), (8 * d, 8), (8 * d, 8), (8 * (d + 1), 8), (4 * d, 8), (8 * 33, 8), (8 * 33, 8),
                       (8 * pp, 8), (8 * pp, 8), (8 * pp, 8), (8 * pp, 8), (8 * pp, 8), (8 * max(p * (p | 1), 1), 8), (pp, 8)):
        off = (a16(off) if al == 16 else a8(off)) + nbytes
    return cap - a8(off)


def scratch_fits(d, p, nI):
    need = scratch_doubles(p, nI)
    return need <= d or 8 * need <= solve_arena_left(d, p)


def draw_rows(rng, d, n_rows, nnz, col_cap):
    """n_rows rows of +-1 with `nnz` entries in all (as even as possible), each row on the emptiest open columns"""
    rows = np.zeros((n_rows, d), np.float32)
    counts = np.zeros(d, np.int64)
    for i in range(n_rows):
        k = nnz // n_rows + (1 if i < nnz % n_rows else 0)
        order = np.lexsort((rng.random(d), counts))
        cols = order[counts[order] < col_cap][:k]
        assert len(cols) == k, "no room under col_cap"
        rows[i, cols] = rng.choice(np.array([-1.0, 1.0], np.float32), k)
        counts[cols] += 1
    return rows


def dense_block(rng, rows, n_free, d, unit_share=0.5):
    units = []
    for k in range(d):
        u = rng.random()
        if u < unit_share:
            sg = (1.0, -1.0) if u < 0.05 * unit_share else ((1.0,) if rng.random() < 0.5 else (-1.0,))
            for s in sg:
                e = np.zeros(d, np.float32)
                e[k] = s
                units.append(e)
    blk = [rows[:n_free], -rows[:n_free], rows[n_free:]]
    if units:
        blk.append(np.stack(units))
    return np.concatenate(blk, axis=0)


def _spoil(rng, case, rows):
    """the defect of an "out" case, applied to the drawn rows; returns (rows, n_free, tail rows appended after the bound rows)"""
    tail = None
    if case.defect == "col9":
        miss = np.flatnonzero(rows[:, 0] == 0)
        have = int((rows[:, 0] != 0).sum())
        rows[miss[:9 - have], 0] = 1.0
        assert (rows[:, 0] != 0).sum() == 9
    elif case.defect == "two":
        i, k = 1, int(np.flatnonzero(rows[1])[0])
        rows[i, k] = 2.0
    elif case.defect == "order":
        a = draw_rows(rng, case.d, 1, 30, 8)
        tail = np.concatenate([a, -a], axis=0)
    return rows, tail


def cone(case, seed, b):
    rng = np.random.default_rng([seed, b, case.d, case.p])
    rows = draw_rows(rng, case.d, case.p, case.nnz, case.col_cap)
    tail = None
    if case.kind == "out":
        rows, tail = _spoil(rng, case, rows)
    blk = dense_block(rng, rows, case.n_free, case.d, case.unit_share)
    if tail is not None:  # after the bound rows, before the unit rows
        n_head = 2 * case.n_free + case.n_bound
        blk = np.concatenate([blk[:n_head], tail, blk[n_head:]], axis=0)
    return blk, rows


def predictions(rng, ctrs):
    """[Gaussian, Gaussian, inside the cone, zero, Gaussian * 1e-6, Gaussian * 1e3, Gaussian ...]"""
    B, m, d = ctrs.shape
    y = rng.standard_normal((B, d)).astype(np.float32)
    if B > 2:
        lam = rng.random(m).astype(np.float32) * (rng.random(m) < 0.5)
        y[2] = lam @ ctrs[2]
    if B > 3:
        y[3] = 0.0
    if B > 4:
        y[4] *= np.float32(1e-6)
    if B > 5:
        y[5] *= np.float32(1e3)
    return y


BENIGN = {d: Case(f"d{d}_benign", d, 10, 3, 5 * d // 2 if d >= 100 else 130) for d in (64, 200, 256)}


def batch(case, seed, B=6, m_max=0):
    """-> dict: ctrs [B, m_max, d], pred [B, d], rows (the reduced rows of every instance, [free | bound]), case.
    "in" / "scratch" cases: every instance is a cone of the case.  "out": instance 1 is, the others are small
    qualifying cones of the same d (their results must not depend on their neighbour)."""
    per = []
    for b in range(B):
        c = case if (case.kind != "out" or b == 1) else BENIGN[case.d]
        per.append((c,) + cone(c, seed, b))
    m = max(blk.shape[0] for _, blk, _ in per)
    m_max = max(m_max, m)
    ctrs = np.zeros((B, m_max, case.d), np.float32)
    for b, (_, blk, _) in enumerate(per):
        ctrs[b, :blk.shape[0]] = blk
    rng = np.random.default_rng([seed, 977, case.d, case.p])
    return {"ctrs": ctrs, "pred": predictions(rng, ctrs), "rows": [r for _, _, r in per], "cases": [c for c, _, _ in per],
            "case": case}


def header_of(case, rows):
    """the slot header words a packed cone of `case` must show: (p, non-zeros, nF, longest column, entries per lane)"""
    return (case.p, int((rows != 0).sum()), case.n_free, int((rows != 0).sum(0).max()), case.chn8)


def dense_nnz(ctrs):
    return int((ctrs != 0).reshape(len(ctrs), -1).sum(1).max())


def m_max_for_fused(ctrs, d):
    """rows a dense batch needs so that the step's per-instance budget of 4 (m_max + d) + 128 non-zeros holds its
    entries (a free row arrives twice)"""
    need = dense_nnz(ctrs)
    m = ctrs.shape[1]
    while 4 * (m + d) + 128 < need:
        m += 1
    return m
