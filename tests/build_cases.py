"""Inputs of the cone-build tests (TEST INFRASTRUCTURE; numpy only, seeded).

Families (each case is one dense batch [B, m, d] float32, 2 <= B <= 8 unless a shape allows only one instance):
  A  random mixes: zero rows, unit rows (+-1, 2.5, -0.25), copies and negations of earlier rows, fresh rows; once with
     +-1 entries and once with Gaussian entries; d in {1, 3, 17, 64, 65, 190}, m in {0, 1, 16, 40, 130}
  B  pairing cases: twin order, duplicates on either side, twins far apart, rows of 64 / 65 / 200 entries, near-twins,
     shifted columns, 40 pairs, and p_raw (general rows) of 1, NT / TEAM and NT / TEAM + 1 for every workgroup shape
  C  signature collisions: different rows that agree in length and in their first kHashPrefix = 12 entries.  The build
     may leave their twins unpaired (build_ref.is_valid_reduction), so these are NOT compared exactly.
  D  thresholds and values: s1 and sqrt(s2) just below, at and just above 1e-7 with every partial sum exact, a
     subnormal entry, -0.0 entries, one 2.0 among +-1 rows, unit rows only, +e_k with -e_k, m = 0
  E  the lite limits: tests/limit_cones.py IN_CASES at B = 2, and one family-C instance that ends with ten bound rows

`check_inputs` asserts what the exact comparison relies on: apart from the rows named as threshold rows, every
non-zero row keeps its s1 and its l2 norm a factor of 4 away from 1e-7, so the order of a float32 summation cannot
decide a class.  A threshold row keeps the quantity under test EXACT under the build's own summation (float32 in
column order for rows of up to 64 entries, double for longer rows) and the other quantity a factor 1.25 away (a float32
sum of n <= 64 terms of one sign is off by at most n 2^-24 relative)."""

from __future__ import annotations

from fractions import Fraction

import numpy as np

import limit_cones as LC

K_HASH_PREFIX, K_LONG_ROW = 12, 64
T32 = np.float32(1e-7)
TEAM = 4                        # WaveCtx / BlockCtx<NW>::TEAM (ctx_wave.h, ctx_block.h)
ROWS_PER_PASS = (16, 32, 64)    # NT / TEAM of the 1-, 2- and 4-wave (also "8") workgroup shapes
UNIT_VALUES = (1.0, -1.0, 2.5, -0.25)


def _case(name, family, insts, m=None, exact_rows=()):
    """stack instances (lists of rows or [m_i, d] arrays) into one zero-padded batch"""
    insts = [np.asarray(a, np.float32) for a in insts]
    d = insts[0].shape[1]
    mm = max([a.shape[0] for a in insts] + [m or 0])
    ctrs = np.zeros((len(insts), mm, d), np.float32)
    for b, a in enumerate(insts):
        ctrs[b, :a.shape[0]] = a
    c = {"name": name, "family": family, "ctrs": ctrs, "exact_rows": set(exact_rows)}
    check_inputs(c)
    return c


def _row(d, cols, vals):
    r = np.zeros(d, np.float32)
    r[np.asarray(cols, np.int64)] = np.asarray(vals, np.float32)
    return r


def _fresh(rng, d, kind, n=None, nmax=6):
    """a general row: n (default 2 .. nmax) entries, +-1 or Gaussian with 1e-2 <= |v|"""
    n = int(rng.integers(2, min(d, nmax) + 1)) if n is None else n
    cols = np.sort(rng.choice(d, n, replace=False))
    if kind == "pm1":
        vals = rng.choice(np.array([-1.0, 1.0], np.float32), n)
    else:
        vals = rng.standard_normal(n).astype(np.float32)
        vals = np.where(np.abs(vals) < 1e-2, np.float32(0.5), vals)
    return _row(d, cols, vals)


# ------------------------------------------------------------------------------------------------------------- A
A_DIMS, A_ROWS = (1, 3, 17, 64, 65, 190), (0, 1, 16, 40, 130)


def random_mix(rng, m, d, kind):
    A = np.zeros((m, d), np.float32)
    for r in range(m):
        u = rng.random()
        earlier = [q for q in range(r) if A[q].any()]
        if u < 0.15:
            continue
        if u < 0.40 or d < 2:
            A[r, int(rng.integers(d))] = UNIT_VALUES[int(rng.integers(4))]
        elif u < 0.55 and earlier:
            A[r] = A[earlier[int(rng.integers(len(earlier)))]]
        elif u < 0.75 and earlier:
            A[r] = -A[earlier[int(rng.integers(len(earlier)))]]
        elif rng.random() < 0.1 and d > 8:
            A[r] = _fresh(rng, d, kind, n=int(rng.integers(d // 2, d + 1)))   # rows of more than 64 entries at d = 190
        else:
            A[r] = _fresh(rng, d, kind)
    return A


def family_a():
    out = []
    for kind in ("pm1", "gauss"):
        for d in A_DIMS:
            for m in A_ROWS:
                rng = np.random.default_rng([1, d, m, kind == "pm1"])
                B = 2 if m == 130 else 4
                out.append(_case(f"A_{kind}_d{d}_m{m}", "A", [random_mix(rng, m, d, kind) for _ in range(B)], m=m))
    return out


# ------------------------------------------------------------------------------------------------------------- B
def _distinct(rng, d, n, kind="pm1", nmax=4):
    """n general rows of which no two are equal or opposite"""
    rows, seen = [], set()
    while len(rows) < n:
        r = _fresh(rng, d, kind, nmax=nmax)
        if r.tobytes() in seen or (-r).tobytes() in seen:
            continue
        seen.add(r.tobytes())
        rows.append(r)
    return rows


def family_b():
    rng = np.random.default_rng(2)
    d = 40
    a, g = _fresh(rng, d, "pm1", n=5), _fresh(rng, d, "gauss", n=5)
    z = np.zeros(d, np.float32)
    e = lambda k, v=1.0: _row(d, [k], [v])
    out = []
    for tag, x in (("pm1", a), ("gauss", g)):
        x2 = x.copy()
        j = int(np.flatnonzero(x)[2])
        x2[j] *= 2.0
        sh = np.roll(x, 1)
        out.append(_case(f"B_twins_{tag}", "B", [
            [x, -x], [-x, x], [x, x, -x], [x, -x, -x], [x, -x, x, -x],
            [x, z, e(3), e(3, -1.0), z, e(7, 2.5), -x, e(9)],      # zero rows and unit rows between the twins
            [x, -x2],                                              # equal but for one value: no pair
            [x, -sh],                                              # equal values on shifted columns: no pair
        ]))
    # rows of 64 and 65 entries (kLongRow: the one-wave-per-row pass), 200 entries at d = 256
    for n, dd in ((64, 80), (65, 80), (200, 256)):
        for tag in ("pm1", "gauss"):
            l1, l2 = _fresh(rng, dd, tag, n=n), _fresh(rng, dd, tag, n=n)
            s = _fresh(rng, dd, tag, n=3)
            out.append(_case(f"B_long{n}_{tag}", "B", [[l1, -l1], [s, l1, l2, -s, -l1], [-l2, l1, l2, l1]]))
    # 40 pairs in one instance, twins in random positions
    rows = _distinct(rng, d, 40)
    both = rows + [-r for r in rows]
    out.append(_case("B_40pairs", "B", [[both[i] for i in rng.permutation(80)] for _ in range(2)]))
    # p_raw general rows: 1, NT / TEAM and NT / TEAM + 1 of every workgroup shape -- pairs, and a single when odd
    insts = []
    for pr in (1,) + tuple(x + s for x in ROWS_PER_PASS for s in (0, 1)):
        rows = _distinct(rng, 24, pr // 2 + pr % 2, nmax=3)
        both = rows[:pr // 2] + [-r for r in rows[:pr // 2]] + rows[pr // 2:]
        assert len(both) == pr
        insts.append([both[i] for i in rng.permutation(pr)] + [_row(24, [5], [1.0])])
    out.append(_case("B_praw", "B", insts))
    return out


# ------------------------------------------------------------------------------------------------------------- C
def colliding(d, n, variants):
    """`variants` different +-1 rows of n entries on columns 0 .. n-1 that agree in their first 12 entries (+1): the
    signs of the entries from K_HASH_PREFIX on count in binary"""
    assert n > K_HASH_PREFIX and variants <= 2 ** (n - K_HASH_PREFIX)
    rows = []
    for v in range(variants):
        r = _row(d, np.arange(n), np.ones(n))
        for bit in range(n - K_HASH_PREFIX):
            if (v >> bit) & 1:
                r[n - 1 - bit] = -1.0
        rows.append(r)
    return rows


def family_c():
    a, b = colliding(40, 14, 2)
    a13, b13 = colliding(40, 13, 2)
    l = _row(120, np.arange(70), np.ones(70))
    l2 = l.copy()
    l2[69] = -1.0
    u = _row(40, [20], [1.0])
    return [
        _case("C_abab", "C", [[a, b, -a, -b], [a, -a, b, -b, u], [-b, a, -a, b]]),
        _case("C_13", "C", [[a13, b13, -a13, -b13], [b13, -b13, u, a13, -a13]]),
        _case("C_long70", "C", [[l, l2, -l, -l2], [l2, -l, l, -l2]]),
        _case("C_one_twin", "C", [[a, b, -a], [b, -a, a], [-a, a, b, u]]),
    ]


def ten_bound_rows(d=40):
    """five colliding rows and their negations: the rules give five free rows; a build that misses every pair keeps ten
    bound rows (and ten entries in twelve columns), which no lite slot takes"""
    rows = colliding(d, 15, 5)
    return np.stack(rows + [-r for r in rows] + [_row(d, [30], [1.0]), _row(d, [31], [-1.0])])


# ------------------------------------------------------------------------------------------------------------- D
def pow2_pieces(x):
    """the set bits of a positive float32, largest first: powers of two that sum to x exactly"""
    fr = Fraction(float(np.float32(x)))
    out, k = [], 200
    while fr > 0:
        while Fraction(2) ** k > fr:
            k -= 1
        out.append(2.0 ** k)
        fr -= Fraction(2) ** k
    return out


def s1_row(d, target, n_min=2):
    """a row whose |entries| are powers of two that sum to `target` exactly (split until there are n_min of them)"""
    ps = pow2_pieces(target)
    while len(ps) < n_min:
        ps = sorted(ps[1:] + [ps[0] / 2, ps[0] / 2], reverse=True)
    assert len(ps) <= d
    sg = np.where(np.arange(len(ps)) % 3 == 1, -1.0, 1.0)
    return _row(d, np.arange(len(ps)), np.array(ps) * sg)


def s2_row(d, target, n_min=2):
    """a row whose squared entries are powers of two that sum to `target` exactly"""
    ps = []
    for q in pow2_pieces(target):   # an odd power of two is two squares
        k = int(round(np.log2(q)))
        ps += [q] if k % 2 == 0 else [q / 2, q / 2]
    while len(ps) < n_min:          # one square = four squares of half the entry
        ps = sorted(ps[1:] + [ps[0] / 4] * 4, reverse=True)
    assert len(ps) <= d, len(ps)
    sg = np.where(np.arange(len(ps)) % 3 == 1, -1.0, 1.0)
    return _row(d, np.arange(len(ps)), np.sqrt(np.array(ps)) * sg)


def s2_targets():
    """float32 values x with sqrtf(x) just below, at and just above float32(1e-7)"""
    t = T32
    x = np.float32(np.float64(t) ** 2)
    sq = lambda v: np.sqrt(np.float32(v), dtype=np.float32)
    while sq(x) >= t:
        x = np.nextafter(x, np.float32(0))
    below = x                                   # the largest x whose root is below t
    while sq(x) < t:
        x = np.nextafter(x, np.float32(1))
    at = x
    while sq(x) <= t:
        x = np.nextafter(x, np.float32(1))
    return below, at, x


def family_d():
    d = 80
    lo, hi = np.nextafter(T32, np.float32(0)), np.nextafter(T32, np.float32(1))
    s2lo, s2at, s2hi = s2_targets()
    g = _row(d, [70, 71, 72], [1.0, -1.0, 1.0])
    u = _row(d, [75], [1.0])
    thr_short = [s1_row(d, lo), s1_row(d, T32), s1_row(d, hi), s2_row(d, s2lo), s2_row(d, s2at), s2_row(d, s2hi)]
    thr_long = [s1_row(d, lo, 65), s1_row(d, T32, 65), s1_row(d, hi, 65), s2_row(d, s2lo, 65), s2_row(d, s2at, 65),
                s2_row(d, s2hi, 65)]
    assert all((r != 0).sum() <= K_LONG_ROW for r in thr_short) and all((r != 0).sum() > K_LONG_ROW for r in thr_long)
    out = [
        _case("D_thresholds_short", "D", [[g, r, u] for r in thr_short], exact_rows={(b, 1) for b in range(6)}),
        _case("D_thresholds_long", "D", [[g, r, u] for r in thr_long], exact_rows={(b, 1) for b in range(6)}),
    ]
    dd = 17
    a = _row(dd, [1, 4, 9], [1.0, -1.0, 1.0])
    b = _row(dd, [2, 4, 11, 12], [-1.0, 1.0, 1.0, -1.0])
    sub = _row(dd, [3, 8], [1.0, 1e-40])
    assert 0 < abs(float(sub[8])) < 1.2e-38   # a subnormal float32
    nz = np.float32(-0.0)
    a_nz, e_nz, z_nz = a.copy(), _row(dd, [6], [-1.0]), np.zeros(dd, np.float32)
    a_nz[[0, 5, 16]] = nz
    e_nz[[0, 7]] = nz
    z_nz[:] = nz
    two = a.copy()
    two[4] = 2.0
    e = lambda k, v: _row(dd, [k], [v])
    out += [
        _case("D_subnormal", "D", [[a, -a, sub, e(5, 1.0)], [sub, -sub], [a, b]]),
        _case("D_negzero", "D", [[a_nz, z_nz, e_nz, -a], [z_nz, z_nz], [a_nz, a, e_nz]]),
        _case("D_one_two", "D", [[a, b, -a, e(5, 1.0)], [a, b, -two, e(5, 1.0)], [a, b, -a, e(5, 2.0)]]),
        _case("D_units_only", "D", [[e(0, 1.0), e(3, -1.0), e(3, -2.5), e(16, 0.25)], [e(1, 1.0)]]),
        _case("D_plus_minus_unit", "D", [[e(4, 1.0), e(4, -1.0), a], [e(4, -0.25), a, e(4, 2.5), e(4, 1.0), -a]]),
        _case("D_m0", "D", [np.zeros((0, dd), np.float32)] * 2),
    ]
    return out


# ------------------------------------------------------------------------------------------------------------- E
def family_e(max_d=256):
    out = []
    for case in LC.IN_CASES:
        if case.d <= max_d:
            out.append({"name": "E_" + case.name, "family": "E", "ctrs": LC.batch(case, 11, B=2)["ctrs"], "exact_rows": set(),
                        "limit_case": case})
    return out


def e_missed_pairs():
    blk = ten_bound_rows()
    easy = np.stack(colliding(40, 15, 1) + [-colliding(40, 15, 1)[0], _row(40, [30], [1.0])])
    return _case("E_ten_bound_rows", "E", [easy, blk])


def all_exact():
    return family_a() + family_b() + family_d()


# ------------------------------------------------------------------------------------------------------ input check
def _exact_under_build(vals, square):
    """is sum |v| (or sum v^2) exact the way build_cone adds it: float32 in entry order up to 64 entries, else double
    (any order: exact in double means the exact sum fits 53 bits and so does every partial sum of these inputs)"""
    terms = [Fraction(float(v)) ** 2 if square else abs(Fraction(float(v))) for v in vals]
    exact = sum(terms, Fraction(0))
    if len(vals) > K_LONG_ROW:
        acc = 0.0
        for v in sorted(vals, key=abs):
            acc += float(v) * float(v) if square else abs(float(v))
        return Fraction(acc) == exact and Fraction(float(np.float32(acc))) == exact
    acc = np.float32(0)
    for v in vals:
        acc = np.float32(acc + (np.float32(v) * np.float32(v) if square else np.abs(np.float32(v))))
    return Fraction(float(acc)) == exact


def check_inputs(case):
    t = float(T32)
    for b, A in enumerate(case["ctrs"]):
        for r in range(A.shape[0]):
            v = A[r][A[r] != 0]
            if len(v) == 0:
                continue
            s1 = float(np.abs(v.astype(np.longdouble)).sum())
            nrm = float(np.sqrt((v.astype(np.longdouble) ** 2).sum()))
            far = lambda x, f: x >= f * t or x * f <= t
            if (b, r) in case["exact_rows"]:
                assert far(s1, 1.25) or _exact_under_build(v, False), (case["name"], b, r, s1)
                assert far(nrm, 1.25) or _exact_under_build(v, True), (case["name"], b, r, nrm)
            else:
                assert far(s1, 4.0) and far(nrm, 4.0), (case["name"], b, r, s1, nrm)


def sparse_of(ctrs):
    """(ent_off int64, key uint32, val float32): the sparse wire format of a dense batch (-0.0 is no entry)"""
    ctrs = np.asarray(ctrs, np.float32)
    B = ctrs.shape[0]
    off, keys, vals = [0], [], []
    for b in range(B):
        r, c = np.nonzero(ctrs[b])
        keys.append(((r.astype(np.uint32) << 16) | c.astype(np.uint32)).astype(np.uint32))
        vals.append(ctrs[b][r, c])
        off.append(off[-1] + len(r))
    return (np.array(off, np.int64), np.concatenate(keys).astype(np.uint32) if keys else np.zeros(0, np.uint32),
            np.concatenate(vals).astype(np.float32) if vals else np.zeros(0, np.float32))
