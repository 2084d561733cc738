"""The cone build, restated (TEST INFRASTRUCTURE, numpy only).

Every kernel entry first turns the raw rows of an instance into the reduced cone the solvers read: build_cone with its
producers (cave_amd/csrc/cone_core.h, cone_instance.h), then compute_avg and a store writer.  `reduce_instance` below
restates that reduction in plain Python from the documented rules, one instance at a time, from a dense [m, d] float32
block; `decode_store` / `decode_lite` turn a slot of a cave_cone_store / cave_lite_store back into the same terms, and
`assert_same` compares the two EXACTLY (p, vkind, usign, n_valid, flag bit 0, every reduced row, every CSC column) and
`avg` against the bound derived below.

The rules
  * a row's non-zeros are its entries v != 0 (a -0.0 is no entry);  s1 = sum |v|,  s2 = sum v^2
  * dropped        iff not float32(s1) > float32(1e-7)
  * unit row       iff exactly one non-zero; every other row that is not dropped is a general row
  * counts in avg  iff sqrt(float32(s2)) > float32(1e-7)                      (n_avg = number of such rows)
  * n_valid        = number of rows not dropped
  * usign[k]       bit 0: a unit row with a positive entry at k; bit 1: one with a negative entry at k
  * general row i is PAIRED with general row j iff j is exactly -i (same columns, negated float32 values), no other
    general row equals i and no other general row equals -i.  The twin with the lower index is kept, vkind = 1 (free
    multiplier), the other is removed.  Every other general row is kept, vkind = 0.
  * reduced rows stand in original row order, their entries in column order; the CSC lists, per column, the entries in
    ascending reduced-row index
  * flag bit 0 iff every entry of the reduced rows is +-1 (unit rows do not matter; set for p = 0)
  * avg[k] = (sum of the signs of the unit rows at k + sum over the kept UNPAIRED rows that count in the average of
    row[k] / max(||row||_2, 1e-8)) / max(n_avg, 1);  paired rows add nothing, but both twins count in n_avg.

The lite slot (cave_lite_store, include/cave_hip.h; cone_core.h lite_build, cone_step.h write_lite_slot) keeps the
reduced rows IN REDUCED ORDER.  It is written only when that order already is [free rows | bound rows] (vkind 1 first):
a cone whose reduced order is anything else is refused (state -1), nothing is permuted.  So "free rows first, then
bound rows, each in reduced order" is the order of every slot that says 1, and it is the reduced order itself.

The avg bound (u = 2^-24, the unit round-off of float32; everything below is first order, the factor 1 + 2^-10 at the
end covers the products of two error terms)
  * norm of a kept row of n entries: s2 is a float32 sum of n squares of one sign, n products and n adds
    (relative n u; build_cone sums rows of more than 64 entries in double and rounds once: u), sqrtf halves a relative
    error and rounds (<= 1 ulp on the device: 2 u), the clamp 1e-8 is inactive for a row that counts (its norm exceeds
    1e-7), the reciprocal rounds once more (2 u with the device's division).  Relative error of vinv:
        e_i = (n_i / 2 + 4) u          with n_i = 2 for rows of more than 64 entries
  * compute_avg starts from (count of +e_k) - (count of -e_k), exact, and does one multiply-add per column entry:
    the product rounds (u) unless contracted, each of the c_k adds rounds relative to a partial sum of at most
    S_k = |unit sum| + sum |terms|
  * the final multiply by invn = fl(1 / n_avg) (2 u) rounds once (u): 3 u S_k
        |avg_k - ref_k| <= [ sum_i |t_ik| (e_i + u) + (c_k + 3) u S_k ] (1 + 2^-10) / max(n_avg, 1)  + (c_k + 3) 2^-149
    (the last term: a rounding in the subnormal range errs by up to the spacing 2^-149, not relatively).
"""

from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
T_DROP = np.float32(1e-7)
T_AVG = np.float32(1e-7)
NORM_CLAMP = 1e-8
K_LONG_ROW = 64
LITE_HDR, LITE_ROWPTR, LITE_CSR_WORDS, LITE_RL = 8, 33, 768, 32
LITE_MAX_ROWS, LITE_MAX_D, LITE_MAX_COL, LITE_MAX_NNZ, LITE_MAX_BOUND = 32, 256, 8, 1536, 8
LD = np.longdouble


def _key(row):
    """bytes that identify a row's (columns, float32 values): -0.0 is no entry"""
    r = np.array(row, np.float32)
    r[r == 0] = 0.0
    return r.tobytes()


def classify_rows(A):
    """-> (tag [m] in {"drop", "unit", "general"}, counts-in-avg [m] bool, s1 [m], norm [m]) with s1 / norm exact"""
    A = np.asarray(A, np.float32)
    m = A.shape[0]
    tags, cnt, s1s, norms = [], np.zeros(m, bool), np.zeros(m, LD), np.zeros(m, LD)
    for r in range(m):
        v = A[r][A[r] != 0].astype(LD)
        s1, s2 = np.abs(v).sum(dtype=LD), (v * v).sum(dtype=LD)
        s1s[r], norms[r] = s1, np.sqrt(s2)
        if not np.float32(s1) > T_DROP:
            tags.append("drop")
            continue
        tags.append("unit" if len(v) == 1 else "general")
        cnt[r] = bool(np.sqrt(np.float32(s2), dtype=np.float32) > T_AVG)
    return tags, cnt, s1s, norms


def csc_of(M):
    """per column: (reduced-row indices ascending, values)"""
    out = []
    for k in range(M.shape[1]):
        rows = np.flatnonzero(M[:, k] != 0)
        out.append((rows.astype(np.int64), M[rows, k].astype(np.float32)))
    return out


def reduce_instance(A):
    """The reduction of one instance A [m, d] -> dict (see the module text)."""
    A = np.array(A, np.float32)
    A[A == 0] = 0.0
    m, d = A.shape
    tags, cnt, _, norms = classify_rows(A)
    usign = np.zeros(d, np.uint8)
    unit_sum = np.zeros(d, LD)
    for r in range(m):
        if tags[r] == "unit":
            k = int(np.flatnonzero(A[r])[0])
            usign[k] |= 1 if A[r, k] > 0 else 2
            unit_sum[k] += 1 if A[r, k] > 0 else -1
    gen = [r for r in range(m) if tags[r] == "general"]
    keys = {r: _key(A[r]) for r in gen}
    nkeys = {r: _key(-A[r]) for r in gen}
    count, first = {}, {}
    for r in gen:
        count[keys[r]] = count.get(keys[r], 0) + 1
        first.setdefault(keys[r], r)
    kept, vkind, twin_of = [], [], {}
    for r in gen:
        paired = count[keys[r]] == 1 and count.get(nkeys[r], 0) == 1
        if paired:
            j = first[nkeys[r]]
            if j < r:
                continue  # the higher-indexed twin is removed
            twin_of[r] = j
        kept.append(r)
        vkind.append(1 if paired else 0)
    p = len(kept)
    M = A[kept] if p else np.zeros((0, d), np.float32)
    n_avg = int(cnt.sum())
    terms = np.zeros((p, d), LD)   # what each kept row adds to the sum of avg
    e_rel = np.zeros(p)
    for i, r in enumerate(kept):
        if vkind[i] == 0 and cnt[r]:
            terms[i] = A[r].astype(LD) / max(norms[r], LD(NORM_CLAMP))
            n = int((A[r] != 0).sum())
            e_rel[i] = ((n if n <= K_LONG_ROW else 2) / 2.0 + 4.0) * U32
    nn = max(n_avg, 1)
    avg = (unit_sum + terms.sum(0, dtype=LD)) / nn
    S = np.abs(unit_sum) + np.abs(terms).sum(0, dtype=LD)
    ck = (M != 0).sum(0)
    bound = ((np.abs(terms) * (e_rel[:, None] + U32)).sum(0, dtype=LD) + (ck + 3) * U32 * S) * (1 + 2.0 ** -10) / nn
    bound = bound + (ck + 3) * 2.0 ** -149
    return {"d": d, "p": p, "M": M, "vkind": np.array(vkind, np.uint8), "usign": usign,
            "n_valid": sum(t != "drop" for t in tags), "n_avg": n_avg, "pm1": bool((np.abs(M[M != 0]) == 1).all()),
            "avg": avg, "avg_bound": bound.astype(np.float64), "csc": csc_of(M), "kept": kept, "twin_of": twin_of,
            "tags": tags}


# ------------------------------------------------------------------------------------------------------- decoders
def _u(a, dt):
    """an integer array of the store reinterpreted as unsigned (torch has no uint16 / uint32: the host copies of the
    device stores arrive as int16 / int32)"""
    a = np.ascontiguousarray(a)
    return a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else a.astype(dt)


def decode_store(arrs, b):
    """Slot b of a cave_cone_store (dict of host arrays by field name) -> dict(p, M, vkind, usign, n_valid, flags, avg,
    csc).  Exact-fit stores take extents from row_off / nnz_off, slot-mode stores (n_rows / n_nnz present) from those.
    flags bit 1: the signs of a +-1 instance sit in bit 15 of ccol / cvar (ConeStore._fold_signs); the pack kernels
    themselves always write plain indices and the values (cone_instance.h run_pack_instance)."""
    n = len(arrs["n_valid"])
    d = len(arrs["usign"]) // n
    r0, z0 = int(arrs["row_off"][b]), int(arrs["nnz_off"][b])
    if arrs.get("n_rows") is not None:
        p, nnz = int(arrs["n_rows"][b]), int(arrs["n_nnz"][b])
        assert 0 <= p <= int(arrs["row_off"][b + 1]) - r0 and 0 <= nnz <= int(arrs["nnz_off"][b + 1]) - z0, (b, p, nnz)
    else:
        p, nnz = int(arrs["row_off"][b + 1]) - r0, int(arrs["nnz_off"][b + 1]) - z0
    flags = int(arrs["flags"][b])
    folded = bool(flags & 2)
    imask = 0x7fff if folded else 0xffff
    rlo, rhi = _u(arrs["rlo"], np.uint32)[r0:r0 + p].astype(np.int64), _u(arrs["rhi"], np.uint32)[r0:r0 + p].astype(np.int64)
    assert p == 0 or (rlo[0] == 0 and rhi[-1] == nnz and (rhi[:-1] == rlo[1:]).all() and (rhi > rlo).all()), (b, rlo, rhi)
    ccol, cvar = _u(arrs["ccol"], np.uint16)[z0:z0 + nnz].astype(np.int64), _u(arrs["cvar"], np.uint16)[z0:z0 + nnz].astype(np.int64)
    cval, cvalc = np.asarray(arrs["cval"], np.float32)[z0:z0 + nnz], np.asarray(arrs["cvalc"], np.float32)[z0:z0 + nnz]
    if folded:  # the sign bits must repeat what the value arrays say
        assert ((ccol >> 15 == 1) == (cval < 0)).all() and ((cvar >> 15 == 1) == (cvalc < 0)).all(), b
    M = np.zeros((p, d), np.float32)
    for i in range(p):
        cols = ccol[rlo[i]:rhi[i]] & imask
        assert (np.diff(cols) > 0).all() and (cols < d).all(), (b, i, cols)   # column order, no repeats
        M[i, cols] = cval[rlo[i]:rhi[i]]
    assert (cval != 0).all()
    cptr = _u(arrs["cptr"], np.uint32)[b * (d + 1):(b + 1) * (d + 1)].astype(np.int64)
    assert cptr[0] == 0 and cptr[d] == nnz and (np.diff(cptr) >= 0).all(), (b, cptr)
    csc = [((cvar[cptr[k]:cptr[k + 1]] & imask), cvalc[cptr[k]:cptr[k + 1]].copy()) for k in range(d)]
    assert all((rows < max(p, 1)).all() for rows, _ in csc), b
    if flags & 1:
        assert (np.abs(cval) == 1).all() and (np.abs(cvalc) == 1).all(), b
    return {"p": p, "M": M, "vkind": np.asarray(arrs["vkind"])[r0:r0 + p].astype(np.uint8),
            "usign": np.asarray(arrs["usign"])[b * d:(b + 1) * d].astype(np.uint8), "n_valid": int(arrs["n_valid"][b]),
            "flags": flags, "avg": np.asarray(arrs["avg"], np.float32)[b * d:(b + 1) * d].copy(), "csc": csc}


def decode_lite(arrs, b, d):
    """Slot b of a cave_lite_store -> dict(state, ...).  state != 1: only the header (which must then be zero).
    The redundant parts are checked against each other: rowptr against the row-end marks of csr16 against rl, ell
    against csr16 as transposes, the header's figures against what the arrays hold, and every unused word inside the
    cone's extent (csr16 entries [nnz, 64 chn8), ell slots behind a column's entries) against its dummy."""
    hdr = np.asarray(arrs["hdr"])[LITE_HDR * b:LITE_HDR * (b + 1)].astype(np.int64)
    state, p, nnz, nF, n_valid, cmax, chn8 = (int(x) for x in hdr[:7])
    if state != 1:
        assert state == -1 and (hdr[1:3] == 0).all() and hdr[4] == 0 and hdr[7] == 0, (b, hdr)
        return {"state": state}
    assert 0 <= nF <= p <= LITE_MAX_ROWS and hdr[7] == 0, (b, hdr)
    rowptr = _u(arrs["rowptr"], np.uint32)[LITE_ROWPTR * b:LITE_ROWPTR * b + p + 1].astype(np.int64)
    assert rowptr[0] == 0 and rowptr[p] == nnz and (np.diff(rowptr) > 0).all(), (b, rowptr)
    usign = np.asarray(arrs["usign"])[b * d:(b + 1) * d].astype(np.uint8)
    avg = np.asarray(arrs["avg"], np.float32)[b * d:(b + 1) * d].copy()
    M = np.zeros((p, d), np.float32)
    if p == 0:
        assert nnz == 0 and cmax == 0 and chn8 == 0, (b, hdr)
        return {"state": 1, "p": 0, "M": M, "vkind": np.zeros(0, np.uint8), "usign": usign, "n_valid": n_valid, "flags": 1,
                "avg": avg, "csc": csc_of(M), "nF": nF}
    assert chn8 == (8 if nnz <= 512 else (16 if nnz <= 1024 else 24)) and 0 < nnz <= LITE_MAX_NNZ, (b, hdr)
    c16 = _u(arrs["csr16"], np.uint32)[LITE_CSR_WORDS * b:LITE_CSR_WORDS * (b + 1)].view(np.uint16).astype(np.int64)
    rl = np.asarray(arrs["rl"])[LITE_RL * b:LITE_RL * b + p].astype(np.int64)
    e = np.arange(64 * chn8)
    lane, c = e // chn8, e % chn8
    w = c16[((c // 8) * 64 + lane) * 8 + c % 8]          # the entries in CSR order
    assert (w[nnz:] == d).all(), (b, "csr16 words behind the last entry must hold the dummy column")
    ends = rowptr[1:] - 1
    is_end = np.zeros(nnz, bool)
    is_end[ends] = True
    assert (((w[:nnz] >> 14) & 1) == is_end).all(), (b, "row-end flags")
    assert (((w[:nnz] >> 9) & 31)[ends] == np.arange(p)).all() and (((w[:nnz] >> 9) & 31)[~is_end] == 0).all(), (b, "row numbers")
    assert (rl == ends // chn8).all(), (b, rl, ends // chn8)
    cols = w[:nnz] & 0x1ff
    assert (cols < d).all(), b
    vals = np.where((w[:nnz] >> 15) & 1, 1.0, -1.0).astype(np.float32)   # the stored sign is that of -M
    for i in range(p):
        cc = cols[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(cc) > 0).all(), (b, i, cc)
        M[i, cc] = vals[rowptr[i]:rowptr[i + 1]]
    ell = _u(arrs["ell"], np.uint32)[4 * d * b:4 * d * (b + 1)].view(np.uint16).astype(np.int64).reshape(d, 8)
    Mt = np.zeros((p, d), np.float32)
    longest = 0
    for k in range(d):
        used = ell[k] != 32
        n = int(used.sum())
        assert used[:n].all(), (b, k, ell[k])            # the dummies stand behind the entries
        rows = ell[k, :n] & 0x7fff
        assert (rows < p).all() and (np.diff(rows) > 0).all(), (b, k, ell[k])
        Mt[rows, k] = np.where(ell[k, :n] >> 15, -1.0, 1.0)
        longest = max(longest, n)
    assert np.array_equal(M, Mt), (b, "ell is not the transpose of csr16")
    assert cmax == longest, (b, cmax, longest)
    vkind = (np.arange(p) < nF).astype(np.uint8)
    return {"state": 1, "p": p, "M": M, "vkind": vkind, "usign": usign, "n_valid": n_valid, "flags": 1, "avg": avg,
            "csc": csc_of(M), "nF": nF}


def lite_takes(ref, d, scratch_fits):
    """does the lite form take this reduced cone (include/cave_hip.h; `scratch_fits(d, p, nI)`: limit_cones.scratch_fits)"""
    p, vk = ref["p"], ref["vkind"]
    if not ref["pm1"] or p > LITE_MAX_ROWS or d > LITE_MAX_D:
        return False
    if p == 0:
        return True
    nF = int(vk.sum())
    nI = p - nF
    nnz = int((ref["M"] != 0).sum())
    return bool((vk[:nF] == 1).all() and nI <= LITE_MAX_BOUND and nnz <= LITE_MAX_NNZ
                and (ref["M"] != 0).sum(0).max() <= LITE_MAX_COL and (nI == 0 or scratch_fits(d, p, nI)))


# ----------------------------------------------------------------------------------------------------- comparisons
def avg_ratio(dec, ref):
    """max_k |avg_k - ref_k| / bound_k (0 where both vanish)"""
    err = np.abs(dec["avg"].astype(LD) - ref["avg"]).astype(np.float64)
    return float((err / ref["avg_bound"]).max(initial=0.0)) if len(err) else 0.0


def _same_csc(a, b):
    return len(a) == len(b) and all(np.array_equal(ra, rb) and np.array_equal(va, vb) for (ra, va), (rb, vb) in zip(a, b))


def assert_same(dec, ref, what=""):
    """exact equality of everything but avg, avg within its bound -> the ratio |avg - ref| / bound"""
    assert dec["p"] == ref["p"], (what, "p", dec["p"], ref["p"])
    assert np.array_equal(dec["vkind"], ref["vkind"]), (what, "vkind", dec["vkind"], ref["vkind"])
    assert np.array_equal(dec["usign"], ref["usign"]), (what, "usign")
    assert dec["n_valid"] == ref["n_valid"], (what, "n_valid", dec["n_valid"], ref["n_valid"])
    assert bool(dec["flags"] & 1) == ref["pm1"], (what, "flag bit 0", dec["flags"], ref["pm1"])
    assert np.array_equal(dec["M"], ref["M"]), (what, "reduced rows")
    assert _same_csc(dec["csc"], ref["csc"]), (what, "CSC")
    r = avg_ratio(dec, ref)
    assert r <= 1.0, (what, "avg", r)
    return r


def is_valid_reduction(A, dec, ref):
    """The property check for inputs where the build may legitimately leave twins unpaired (colliding signatures):
    every kept row is an original general row, in order; a row with vkind = 1 has its exact negation among the
    originals and is kept once; every general row is kept or is the negation of a kept free row; no row is kept twice
    over (a kept row stands for itself and, if free, for its negation -- nothing else may stand for either); usign,
    n_valid, the CSC as the transpose of the CSR are as the rules say; avg is within its bound of the value the rules
    give for THIS choice of pairs (an unpaired twin pair adds a/|a| - a/|a|: zero up to two roundings of the sum).
    -> (ok, reason)"""
    A = np.array(A, np.float32)
    A[A == 0] = 0.0
    gen = [r for r, t in enumerate(ref["tags"]) if t == "general"]
    M, vk = dec["M"], dec["vkind"]
    if len(M) != len(vk) or dec["p"] != len(M):
        return False, "p"
    pos, src = 0, []
    for i in range(len(M)):   # kept rows are original general rows, in order (greedy match on the earliest candidate)
        while pos < len(gen) and _key(A[gen[pos]]) != _key(M[i]):
            pos += 1
        if pos == len(gen):
            return False, f"reduced row {i} is no original general row in order"
        src.append(gen[pos])
        pos += 1
    orig = [_key(A[r]) for r in gen]
    stands = {}
    for i in range(len(M)):
        k, nk = _key(M[i]), _key(-M[i])
        if vk[i] == 1 and nk not in orig:
            return False, f"free row {i} has no exact negation among the originals"
        for key in ((k, nk) if vk[i] == 1 else (k,)):
            stands[key] = stands.get(key, 0) + 1
    for key in orig:
        if key not in stands:
            return False, "a general row is neither kept nor the negation of a kept free row"
    for i in range(len(M)):
        if vk[i] == 1 and (stands[_key(M[i])] != 1 or stands[_key(-M[i])] != 1 or orig.count(_key(M[i])) != 1
                           or orig.count(_key(-M[i])) != 1):
            return False, f"free row {i}: the row or its negation is kept twice over"
    if len(M) - int(vk.sum()) + 2 * int(vk.sum()) != len(gen):
        return False, "rows lost or invented"
    if not np.array_equal(dec["usign"], ref["usign"]) or dec["n_valid"] != ref["n_valid"]:
        return False, "usign / n_valid"
    if bool(dec["flags"] & 1) != ref["pm1"]:
        return False, "flag bit 0"
    if not _same_csc(dec["csc"], csc_of(M)):
        return False, "the CSC is not the transpose of the CSR"
    # avg: the unpaired twins cancel in exact arithmetic, so the rules' value stands; the bound is that of the rows kept
    alt = _avg_for(A, ref, src, vk)
    err = np.abs(dec["avg"].astype(LD) - alt["avg"]).astype(np.float64)
    if not (err <= alt["avg_bound"]).all():
        return False, f"avg off by {float((err / alt['avg_bound']).max()):.3g} bounds"
    return True, ""


def _avg_for(A, ref, src, vkind):
    """avg and its bound for the reduced rows `src` (original indices) with kinds `vkind`, everything else as in ref"""
    tags, cnt, _, norms = classify_rows(A)
    d = A.shape[1]
    unit_sum = np.zeros(d, LD)
    for r, t in enumerate(tags):
        if t == "unit":
            k = int(np.flatnonzero(A[r])[0])
            unit_sum[k] += 1 if A[r, k] > 0 else -1
    p = len(src)
    terms, e_rel = np.zeros((p, d), LD), np.zeros(p)
    for i, r in enumerate(src):
        if vkind[i] == 0 and cnt[r]:
            terms[i] = A[r].astype(LD) / max(norms[r], LD(NORM_CLAMP))
            n = int((A[r] != 0).sum())
            e_rel[i] = ((n if n <= K_LONG_ROW else 2) / 2.0 + 4.0) * U32
    nn = max(int(cnt.sum()), 1)
    S = np.abs(unit_sum) + np.abs(terms).sum(0, dtype=LD)
    ck = (A[src] != 0).sum(0) if p else np.zeros(d, np.int64)
    bound = ((np.abs(terms) * (e_rel[:, None] + U32)).sum(0, dtype=LD) + (ck + 3) * U32 * S) * (1 + 2.0 ** -10) / nn
    return {"avg": (unit_sum + terms.sum(0, dtype=LD)) / nn, "avg_bound": (bound + (ck + 3) * 2.0 ** -149).astype(np.float64)}


def no_false_pairs(A, dec):
    """no row is ever paired with a row that is not its exact negation: every free row's negation is an original row"""
    A = np.array(A, np.float32)
    A[A == 0] = 0.0
    orig = {_key(A[r]) for r in range(A.shape[0])}
    return all(_key(-dec["M"][i]) in orig for i in range(dec["p"]) if dec["vkind"][i] == 1)


# --------------------------------------------------------------------------------------------------------- margins
# worst |avg - ref| / bound per route; the GPU tier writes profiles/build_margins.json, the CPU tier only where the
# environment variable CAVE_BUILD_MARGINS names a JSON file (it also redirects the GPU tier)
MARGINS: dict = {}


def record(route, ratio):
    MARGINS[route] = max(MARGINS.get(route, 0.0), float(ratio))


def dump_margins(tier, default=None):
    import json
    import os

    path = os.environ.get("CAVE_BUILD_MARGINS", default)
    if not path or not MARGINS:
        return
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[tier] = {k: float("%.3g" % v) for k, v in sorted(MARGINS.items())}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")
