"""CPU tier: the fused step kernel (cave_amd/csrc/cone_step.h) under the SIMT emulation, at the lite solver's limits.

cave_hip_cone_step / cave_hip_cone_step_warm / cave_hip_lite_from_packed are what the benchmark metric is taken from,
and until now hipcc was the only compiler that saw their per-instance code: write_lite_slot, run_pack_lite_instance,
run_lite_from_packed and run_lite_instance<.., WARM> (the prologue that loads a slot into registers, the content
fingerprint, the cache probe / way choice / write-back, the scratch decision for lite_model_step,
CAVE_STEP_ZERO_FAILED).  tests/emul/simt_abi.cpp now runs them on host memory -- every lane a fiber, round-robin or
seeded shuffled schedules, LDS an exact-size heap block whose size comes from the product's own step_limits -- and
tests/limit_cones.py draws cones that sit ON the limits the header advertises (d = 256 / 255 / 193: the fourth
coordinate slot of a lane; 1536 / 1027 non-zeros: the third csr16 group; 32 rows; 8 bound rows; every column full),
where TSP-20 / TSP-12 / SP 5x5 never go.

Reference: oracle.cave_oracle in fp64 (batch_project, exact / inner / heuristic targets, average_ctrs, cone_loss,
cone_loss_grad), every projection of it KKT-certified (tests/certificate.py, 4e-6) before it is used.  Tolerances are
those of tests/golden_cases.py: proj 2e-6 max(1, |y|_inf), rnorm 2e-6 max(1, rnorm), loss 2e-6, target 8e-6, grad
8e-6 max(1, |grad|_inf); inside-the-cone decisions equal.

Not emulated (tests/emul/simt_abi.cpp says so too): the wave election of a solve block and the wave priorities.
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import ctypes as C
import functools
from unittest import mock

import numpy as np
import pytest

import limit_cones as LC
from certificate import kkt_certificate
from emul_lib import ST_BAD_INPUT, ST_TOO_LARGE, STEP_ZERO_FAILED, Emul, Simt, lite_store, warm_cache
from golden_cases import MODE_AVG, MODE_EXACT, MODE_HEURISTIC, MODE_INNER, MODE_PROJECT, TOL, check_case, check_regress
from oracle import cave_oracle as O

SEEDS = (11, 12)
MODES = (MODE_PROJECT, MODE_EXACT, MODE_INNER, MODE_HEURISTIC, MODE_AVG)
SOLVE_MODES = (MODE_PROJECT, MODE_EXACT, MODE_INNER)
RATIO = 0.2


@pytest.fixture(scope="module")
def emul():
    return Emul()


@pytest.fixture(scope="module")
def simt():
    return Simt()


# ------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def _batch(name, seed, m_max=0):
    case = {c.name: c for c in LC.IN_CASES + LC.SCRATCH_CASES + LC.OUT_CASES}[name]
    return LC.batch(case, seed, m_max=m_max)


@functools.lru_cache(maxsize=None)
def _projection(name, seed, sign):
    """oracle projection of sign * pred for every instance of the batch, each KKT-certified (no instance left out)"""
    bt = _batch(name, seed)
    y = np.float32(sign) * bt["pred"]
    proj, rnorm = O.batch_project(y, bt["ctrs"])
    for b in range(len(y)):
        c = kkt_certificate(bt["ctrs"][b], y[b], proj[b], 4e-6)
        assert c["dual"] <= 4e-6 and c["comp"] <= 4e-6 and c["member"], (name, seed, sign, b, c)
    return proj, rnorm


def reference(name, seed, mode, sign):
    """proj, rnorm, target, loss, grad of the oracle's own functions (the projection is computed once per batch and sign)"""
    bt = _batch(name, seed)
    ctrs, pred = bt["ctrs"], bt["pred"]
    y = np.float32(sign) * pred
    proj, rnorm = _projection(name, seed, sign)
    with mock.patch.object(O, "batch_project", lambda *_a: (proj, rnorm)):
        if mode == MODE_EXACT:
            target = O.exact_target(y, ctrs)[0]
        elif mode == MODE_INNER:
            target = O.inner_target(y, ctrs, RATIO)[0]
        elif mode == MODE_HEURISTIC:
            target = O.heuristic_target(y, ctrs, RATIO)
        elif mode == MODE_AVG:
            target = O.average_ctrs(ctrs)
        else:
            target = None
    ref = {"proj": proj, "rnorm": rnorm, "target": target}
    if target is not None and mode != MODE_AVG:
        ref["loss"], ref["grad"] = O.cone_loss(pred, target, sign), O.cone_loss_grad(pred, target, sign)
    return ref


def assert_matches(o, ref, mode, y, what, rows=None):
    rows = np.arange(len(y)) if rows is None else np.asarray(rows)
    sc = np.maximum(1.0, np.abs(y).max(axis=1))[rows, None]
    if mode in SOLVE_MODES:
        assert np.all(np.abs(o["proj"][rows] - ref["proj"][rows]) <= TOL * sc), (what, "proj")
        rn = ref["rnorm"][rows]
        assert np.all(np.abs(o["rnorm"][rows] - rn) <= TOL * np.maximum(1.0, rn)), (what, "rnorm")
        assert np.array_equal(o["rnorm"][rows] < np.float32(1e-7), rn < np.float32(1e-7)), (what, "inside-the-cone decision")
    if mode != MODE_PROJECT:
        assert np.all(np.abs(o["target"][rows] - ref["target"][rows]) <= 4 * TOL), (what, "target")
    if mode in (MODE_EXACT, MODE_INNER, MODE_HEURISTIC):
        assert np.all(np.abs(o["loss"][rows] - ref["loss"][rows]) <= TOL), (what, "loss")
        gs = max(1.0, float(np.abs(ref["grad"][rows]).max()))
        assert np.all(np.abs(o["grad"][rows] - ref["grad"][rows]) <= 4 * TOL * gs), (what, "grad")


# ------------------------------------------------------------------------------------------------ the two routes
def fused_limit(simt, m_of_d):
    """largest d with a fused launch (solve beside a pack of m_of_d(d) rows): asked of the product's own formula"""
    for d in range(256, 0, -1):
        if simt.step_lds_bytes(m_of_d(d), d) > 0:
            return d
    return 0


def hdr_of(arrs, b):
    return arrs["hdr"][8 * b: 8 * b + 8]


def slot_words(arrs, b, d):
    """the words of slot b a solve may read for the cone it holds: hdr, usign, rowptr[0..p], ell, csr16 up to the cone's
    own extent (32 * chn8 words), rl[0..p)"""
    h = hdr_of(arrs, b)
    p, chn8 = int(h[1]), int(h[6])
    return {
        "hdr": h.copy(), "usign": arrs["usign"][b * d:(b + 1) * d].copy(),
        "rowptr": arrs["rowptr"][33 * b: 33 * b + p + 1].copy(),
        "ell": (arrs["ell"][4 * d * b: 4 * d * (b + 1)].copy() if p > 0 else np.zeros(0, np.uint32)),
        "csr16": arrs["csr16"][768 * b: 768 * b + 32 * chn8].copy(),
        "rl": arrs["rl"][32 * b: 32 * b + p].copy(), "avg": arrs["avg"][b * d:(b + 1) * d].copy(),
    }


def store_route(emul, simt, ctrs, seed=0, fill=0):
    # (the default non-zero budget of the general pack is sized for structured cones: give it the batch's own count)
    st, arrs, mr, mn = emul.pack(ctrs, nnz_cap=LC.dense_nnz(ctrs) + 64, lds_bytes=160 * 1024)
    keep = (st, arrs)  # (the ctypes struct points into arrs)
    ls, la, status = simt.lite_from_packed(st, seed=seed, fill=fill)
    return ls, la, status, keep


def fused_ok(simt, ctrs):
    return simt.step_lds_bytes(ctrs.shape[1], ctrs.shape[2]) > 0


# ================================================================================================ D1: fixtures
@pytest.mark.parametrize("tag,n", [("sp5", 32), ("tsp20", 16)])
def test_step_kernel_on_the_reference_fixtures_under_emulation(simt, golden, tag, n):
    """structured.npz (outputs of the reference itself): emulated pack half -> emulated solve half, every check of
    golden_cases.check_case; then two shuffled lane schedules against the round-robin one, bit for bit; the path counter proves that the solve
    half's lite solver ran for every instance of every projecting call."""
    g = golden["structured"]
    ctrs = g[f"{tag}_ctrs"]
    assert fused_ok(simt, ctrs)
    st, arrs, status = simt.step_pack(ctrs)
    assert (status == 0).all() and (arrs["hdr"][0::8] == 1).all()
    simt.path_counters()
    calls = [0]

    def impl(c, costs, mode, sign, ratio):
        assert c.shape == ctrs.shape
        calls[0] += mode in SOLVE_MODES
        return simt.step_solve(st, costs, mode, sign=sign, inner_ratio=ratio, B=len(c), m_max=c.shape[1])

    check_case(impl, {"structured": g}, "structured", tag)
    assert simt.path_counters()[6] == calls[0] * len(ctrs) and calls[0] == 6
    # shuffled lane schedules: the same words in the slots, the same bits out (no result depends on the order in which
    # the lanes run between two ordering points)
    costs = g[f"{tag}_costs"]
    base = simt.step_solve(st, costs, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=ctrs.shape[1])
    for seed in (5, 23):
        st2, arrs2, status2 = simt.step_pack(ctrs, seed=seed)
        assert (status2 == 0).all()
        for b in range(len(ctrs)):
            wa, wb = slot_words(arrs, b, ctrs.shape[2]), slot_words(arrs2, b, ctrs.shape[2])
            assert all(np.array_equal(wa[k], wb[k]) for k in wa), (seed, b)
        o = simt.step_solve(st2, costs, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=ctrs.shape[1], seed=seed + 1)
        for k in ("proj", "rnorm", "target", "loss", "grad", "status", "iters"):
            assert np.array_equal(o[k], base[k]), (seed, k)


def test_step_kernel_on_the_regression_fixtures_under_emulation(emul, simt, golden):
    """regress.npz (cones that once hit the iteration cap, tiny-norm predictions): those the lite form takes go through
    pack -> solve of the step kernel, the others must be refused by BOTH halves (slot -1, TOO_LARGE) -- and then match
    the reference through the general one-wave solver as before."""
    took = []

    def impl(A, y, mode, sign, ratio):
        st, arrs, status = simt.step_pack(A, seed=len(took))
        o = simt.step_solve(st, y, mode, sign=sign, inner_ratio=ratio, m_max=A.shape[1], seed=len(took))
        took.append(int(arrs["hdr"][0]))
        if arrs["hdr"][0] == 1:
            assert status[0] == 0 and o["iters"][0] > 0
            return o
        assert status[0] == ST_TOO_LARGE and o["status"][0] == ST_TOO_LARGE and np.isnan(o["proj"]).all()
        return simt.cone_dense(A, y, mode, sign=sign, inner_ratio=ratio, waves=1)

    check_regress(impl, golden["regress"])
    assert took.count(1) >= 1, took


# ================================================================================================ D2: "in" cases
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", LC.IN_CASES, ids=lambda c: c.name)
def test_limit_cones_are_solved_by_the_lite_code(emul, simt, case, seed):
    """Every "in" case of tests/limit_cones.py: (store route) Emul.pack -> run_lite_from_packed -> solve half with
    shuffled ids; (fused route, where the product has such a launch for the shape) pack half -> solve half.  The slot
    header must show the case where it claims to be; all five modes, both signs, vs the certified oracle; status 0,
    <= 40 iterations; the lite solver ran (path counter); the slots of the two routes are equal word for word and the
    outputs bit for bit; a repeated id gives the same bits twice, an id out of range CAVE_ST_BAD_INPUT with NaN outputs
    and untouched neighbours."""
    bt = _batch(case.name, seed)
    ctrs, pred, d = bt["ctrs"], bt["pred"], case.d
    B = len(ctrs)
    ls, la, lstatus, keep = store_route(emul, simt, ctrs, seed=seed)
    assert (lstatus == 0).all(), lstatus
    for b in range(B):
        h = hdr_of(la, b)
        want = LC.header_of(case, bt["rows"][b])
        assert h[0] == 1 and (h[1], h[2], h[3], h[5], h[6]) == want, (b, h, want)
    assert LC.scratch_fits(d, case.p, case.n_bound)
    fused = None
    if fused_ok(simt, ctrs):
        fused = simt.step_pack(ctrs, seed=seed + 1, fill=0xA5)
        if (fused[2] == 0).all():
            for b in range(B):
                wa, wb = slot_words(la, b, d), slot_words(fused[1], b, d)
                for k in wa:
                    assert np.array_equal(wa[k], wb[k]), (b, k)
        else:  # the dense entries of the batch exceed the step's per-instance budget of 4 (m_max + d) + 128
            assert 4 * (ctrs.shape[1] + d) + 128 < LC.dense_nnz(ctrs) and set(fused[2]) <= {0, ST_TOO_LARGE}
            fused = None
    perm = np.random.default_rng(seed).permutation(B)
    ids = np.concatenate([perm, [perm[0], B + 3, -1]]).astype(np.int64)
    # bound rows tight at the oracle's answer: the active-set loop must be exercised (some, not all, for one instance)
    if case.n_bound >= 2:
        mixed = 0
        for sign in (-1.0, 1.0):
            proj, _ = _projection(case.name, seed, sign)
            y = np.float32(sign) * pred
            for b in range(B):
                slack = bt["rows"][b][case.n_free:].astype(np.float64) @ (y[b].astype(np.float64) - proj[b])
                tight = int((np.abs(slack) <= 1e-5).sum())
                mixed += 0 < tight < case.n_bound
        assert mixed >= 1, "no instance has some but not all of its bound rows tight"
    simt.path_counters()
    n_solved = 0
    for sign in (-1.0, 1.0):
        y = np.float32(sign) * pred
        for mode in MODES:
            ref = reference(case.name, seed, mode, sign)
            pin = None if mode == MODE_AVG else np.concatenate([pred[perm], pred[perm[:1]], pred[:2]])
            o = simt.step_solve(ls, pin, mode, sign=sign, inner_ratio=RATIO, ids=ids, seed=seed * (mode + 1))
            n_solved += (B + 1) * (mode in SOLVE_MODES)
            assert (o["status"][:B + 1] == 0).all(), (mode, sign, o["status"])
            assert o["iters"][:B + 1].max() <= 40 and (mode not in SOLVE_MODES or o["iters"][:B + 1].min() >= 0)
            back = {k: np.empty_like(v[:B]) for k, v in o.items()}
            for k in back:
                back[k][perm] = o[k][:B]
            assert_matches(back, ref, mode, y, (case.name, seed, mode, sign))
            for k in ("proj", "rnorm", "target", "loss", "grad"):   # the repeated id: the same bits
                assert np.array_equal(o[k][B], o[k][0]), k
            assert (o["status"][B + 1:] == ST_BAD_INPUT).all()
            assert np.isnan(o["proj"][B + 1:]).all() and np.isnan(o["loss"][B + 1:]).all() and (o["iters"][B + 1:] == 0).all()
            if fused is not None:
                f = simt.step_solve(fused[0], None if mode == MODE_AVG else pred, mode, sign=sign, inner_ratio=RATIO,
                                    B=B, m_max=ctrs.shape[1], seed=seed + 7)
                n_solved += B * (mode in SOLVE_MODES)
                for k in ("proj", "rnorm", "target", "loss", "grad", "status", "iters"):
                    assert np.array_equal(f[k], back[k], equal_nan=True), (mode, sign, k)
    assert simt.path_counters()[6] == n_solved   # (every limit cone keeps rows: none is the empty cone)


FUSED_FAMILIES = [
    # (free, bound, non-zeros, share of unit rows, smallest d the fused form must reach)
    (16, 8, 1032, 0.1, 193),   # 8 bound rows, third csr16 group, fourth coordinate slot -- all in the FUSED form
    (27, 5, 1100, 0.5, 0),     # 32 rows: its dense entries (free rows arrive twice) need m_max ~ 290: NO fused launch at any d
]


@pytest.mark.parametrize("fam", FUSED_FAMILIES, ids=lambda f: f"{f[0]}f{f[1]}b_{f[2]}")
def test_fused_launch_limit_and_a_cone_at_it(emul, simt, fam):
    """Which launch form a shape can take.  At d = 256 (from d = 229 on, whatever m_max) six workgroups do not fit a
    compute unit: no fused launch; such cones reach the lite solver through the lite slots of a store only (m_max = 0:
    four workgroups per compute unit).  The largest d at which a family of limit cones still has a fused launch is
    asked of the product's formula, downwards from 256, with the dense block padded with zero rows until the step's
    budget of 4 (m_max + d) + 128 non-zeros per instance holds its entries.  Found here: 24 rows (16 free + 8 bound) with
    1032 non-zeros go fused up to d = 228 (the limit of the fused form itself) -- the fourth coordinate slot (d >= 193) IS covered in the fused form; 32 rows
    with more than 1024 non-zeros are NOT, at any d: their dense entries need m_max of about 290, and a pack half of that
    many rows does not keep six workgroups on a compute unit at any d that holds 1100 entries in columns of 8.  That
    class meets the lite solver on the store route only (asserted as found).  At the d found: both routes, slots equal
    word for word, outputs equal bit for bit and vs the oracle; and the same batch NOT padded: pack status
    CAVE_ST_TOO_LARGE, slots -1."""
    assert simt.step_lds_bytes(0, 256) == 28672 and simt.step_lds_bytes(0, 190) == 25344 and simt.step_lds_bytes(232, 190) == 26624
    for m in (1, 190, 400, 1000):
        assert simt.step_lds_bytes(m, 256) < 0 and simt.step_lds_bytes(m, 229) < 0
    assert simt.step_lds_bytes(64, 228) > 0
    assert simt.step_lds_bytes(0, 257) < 0 and simt.step_lds_bytes(100, 257) < 0
    n_free, n_bound, nnz, share, d_min = fam
    dlim = m_pad = 0
    for d in range(256, (nnz + 7) // 8 - 1, -1):   # (columns hold at most 8 entries)
        probe = LC.batch(LC.Case("probe", d, n_free, n_bound, nnz, unit_share=share), 3, B=4)
        m = LC.m_max_for_fused(probe["ctrs"], d)
        if simt.step_lds_bytes(m, d) > 0:
            dlim, m_pad = d, m
            break
    if d_min == 0:
        assert dlim == 0, dlim   # (the finding of the docstring: if this class ever gets a fused launch, say so there)
        return
    assert d_min <= dlim < 256, dlim
    p = n_free + n_bound
    case = LC.Case(f"d{dlim}_fused", dlim, n_free, n_bound, nnz, unit_share=share)
    bt0 = LC.batch(case, 3, B=4)
    assert 4 * (bt0["ctrs"].shape[1] + dlim) + 128 < LC.dense_nnz(bt0["ctrs"])   # as drawn, the dense entries do not fit
    assert simt.step_lds_bytes(bt0["ctrs"].shape[1], dlim) > 0
    _, a0, s0 = simt.step_pack(bt0["ctrs"])
    assert (s0 == ST_TOO_LARGE).all() and (a0["hdr"][0::8] == -1).all()
    bt = LC.batch(case, 3, B=4, m_max=m_pad)
    ctrs, pred = bt["ctrs"], bt["pred"]
    fs, fa, fstatus = simt.step_pack(ctrs, seed=9)
    assert (fstatus == 0).all()
    ls, la, lstatus, keep = store_route(emul, simt, ctrs)
    proj, rnorm = O.batch_project(-pred, ctrs)
    for b in range(4):
        c = kkt_certificate(ctrs[b], -pred[b], proj[b], 4e-6)
        assert c["dual"] <= 4e-6 and c["comp"] <= 4e-6 and c["member"], c
        assert tuple(hdr_of(fa, b)[[0, 1, 2, 3, 6]]) == (1, p, nnz, n_free, 24)
        wa, wb = slot_words(la, b, dlim), slot_words(fa, b, dlim)
        assert all(np.array_equal(wa[k], wb[k]) for k in wa)
    simt.path_counters()
    a = simt.step_solve(fs, pred, MODE_PROJECT, sign=-1.0, m_max=m_pad, seed=4)
    b_ = simt.step_solve(ls, pred, MODE_PROJECT, sign=-1.0, m_max=0)
    assert simt.path_counters()[6] == 8
    for o in (a, b_):
        assert (o["status"] == 0).all() and o["iters"].max() <= 40
        assert_matches(o, {"proj": proj, "rnorm": rnorm}, MODE_PROJECT, -pred, "fused limit")
    assert np.array_equal(a["proj"], b_["proj"]) and np.array_equal(a["iters"], b_["iters"])


# ================================================================================================ D3: "out" cases
OUT_SEEDS = (21, 22)


@pytest.mark.parametrize("seed", OUT_SEEDS)
@pytest.mark.parametrize("case", LC.OUT_CASES + LC.SCRATCH_CASES, ids=lambda c: c.name)
def test_cones_beyond_a_limit_are_refused_by_both_halves(emul, simt, case, seed):
    """A cone beyond a documented limit (33 rows, 9 bound rows, a column of 9, 1568 non-zeros, rows not [free | bound],
    an entry 2.0) -- or within them but with an active-set scratch the solve half's arena cannot hold ("scratch" cases:
    lite_scratch_fits) -- is marked -1 by the pack half and by run_lite_from_packed (pack status CAVE_ST_TOO_LARGE); the
    solve half reports CAVE_ST_TOO_LARGE with NaN outputs for it, loss 0 / zero gradient under CAVE_STEP_ZERO_FAILED;
    the other instances of the batch are solved as if it were not there."""
    bt = _batch(case.name, seed)
    ctrs, pred, d = bt["ctrs"], bt["pred"], case.d
    B = len(ctrs)
    bad = np.arange(B) if case.kind == "scratch" else np.array([1])
    good = np.setdiff1d(np.arange(B), bad)
    if case.kind == "scratch":
        assert not LC.scratch_fits(d, case.p, case.n_bound) and not simt.lite_scratch_fits(d, case.p, case.n_bound)
    routes = [store_route(emul, simt, ctrs)[:3]]
    if fused_ok(simt, ctrs) and 4 * (ctrs.shape[1] + d) + 128 >= LC.dense_nnz(ctrs):
        routes.append(simt.step_pack(ctrs, seed=3))
    ref = None
    if len(good):
        proj, rnorm = O.batch_project(-pred, ctrs)
        ref = {"proj": proj, "rnorm": rnorm}
    for ls, la, status in routes:
        assert (status[bad] == ST_TOO_LARGE).all() and (status[good] == 0).all(), status
        for b in bad:
            assert hdr_of(la, b)[0] == -1 and (hdr_of(la, b)[[1, 2, 4]] == 0).all()
        for m_max in (0, ctrs.shape[1]):
            if simt.step_lds_bytes(m_max, d) < 0:
                continue
            o = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=m_max, seed=m_max)
            assert (o["status"][bad] == ST_TOO_LARGE).all() and (o["status"][good] == 0).all(), o["status"]
            for k in ("proj", "rnorm", "target", "loss", "grad"):
                assert np.isnan(o[k][bad]).all(), k
            z = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=m_max, flags=STEP_ZERO_FAILED)
            assert (z["status"] == o["status"]).all()
            assert (z["loss"][bad] == 0).all() and (z["grad"][bad] == 0).all() and np.isnan(z["proj"][bad]).all()
            if len(good):
                assert_matches(o, ref, MODE_PROJECT, -pred, (case.name, m_max), rows=good)
                for k in ("proj", "rnorm", "target", "loss", "grad"):
                    assert np.array_equal(z[k][good], o[k][good]), k


# ================================================================================================ D4: a slot that says 1 is solved
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", LC.IN_CASES, ids=lambda c: c.name)
def test_a_slot_that_says_one_is_solved_by_every_launch_form(emul, simt, case, seed):
    """The header word and the solve half must agree: write_lite_slot says 1 for a cone only if run_lite_instance finds
    its arrays AND the scratch of lite_model_step in the smallest arena a launch can have -- that of a solve-only launch
    (m_max = 0: the lite slots of a ConeStore, whose LDS is step_solve_lds_bytes(d) alone).  Before lite_scratch_fits,
    a cone with p = 32 and 6 - 8 bound rows (scratch of 259 - 361 doubles, more than d and more than the 160 bytes the
    arena has left at d = 256) was marked 1 and then reported CAVE_ST_TOO_LARGE by every solve-only launch.  Here: status
    CAVE_ST_OK with the LDS of a solve-only and of a fused launch, cold, on a warm miss and on a warm hit, with and
    without the warm variant's extra LDS block.  The cases include the accepted side of the rule's boundary at d = 256
    (28 rows with 7 bound rows, 27 with 8), whose scratch block is the last thing that fits the solve-only arena."""
    bt = _batch(case.name, seed)
    ctrs, pred, d = bt["ctrs"], bt["pred"], case.d
    assert simt.lite_scratch_fits(d, case.p, case.n_bound)
    ls, la, status, keep = store_route(emul, simt, ctrs)
    assert (status == 0).all() and (la["hdr"][0::8] == 1).all()
    forms = [0] + ([ctrs.shape[1]] if fused_ok(simt, ctrs) else [])
    assert simt.step_lds_bytes(0, d) > 0
    cold = None
    for m_max in forms:
        o = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=m_max)
        assert (o["status"] == 0).all(), (m_max, o["status"])
        cold = cold or o
        for extra in (0, 256):
            wc, wa = warm_cache(64)
            miss = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=m_max, warm=wc, lds_extra=extra)
            hit = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=m_max, warm=wc, lds_extra=extra)
            assert (miss["status"] == 0).all() and (hit["status"] == 0).all(), (m_max, extra, miss["status"], hit["status"])
            assert (miss["warm_hit"] == 0).all()
            for k in ("proj", "rnorm", "target", "loss", "grad", "iters"):   # a miss computes what the cold kernel computes
                assert np.array_equal(miss[k], cold[k], equal_nan=True), (m_max, extra, k)
            # (with no extra block the hit's multipliers need 128 bytes of the arena: no room = a miss, never a failure)
            if extra:
                assert (hit["warm_hit"] == 1).all(), (m_max, hit["warm_hit"])


# ================================================================================================ D5: warm cache
def _warm_case():
    return "d256_16f8b_1536"


KEY_CASE = "d193_19f8b_1027"   # 24 entries per lane, the third csr16 group partly dummy entries (column d, residual 0)


def test_warm_cache_hits_and_keeps_the_results(emul, simt):
    """Second solve of the same cones: every instance hits, results within the solver tolerance of the cold ones (vs the
    oracle), no more iterations in total; caller keys and content keys; HEURISTIC / AVG leave the cache untouched."""
    name = _warm_case()
    bt = _batch(name, SEEDS[0])
    ctrs, pred = bt["ctrs"], bt["pred"]
    B = len(ctrs)
    ls, la, status, keep = store_route(emul, simt, ctrs)
    ref = reference(name, SEEDS[0], MODE_INNER, -1.0)
    cold = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO)
    for keys in (None, np.arange(B) + 100):
        wc, wa = warm_cache(16)
        for mode in (MODE_HEURISTIC, MODE_AVG):
            o = simt.step_solve(ls, pred, mode, sign=-1.0, inner_ratio=RATIO, warm=wc, keys=keys)
            assert (o["warm_hit"] == 0).all() and not wa["key"].any() and not wa["theta"].any()
        first = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, warm=wc, keys=keys, seed=3)
        assert (first["warm_hit"] == 0).all() and np.array_equal(first["proj"], cold["proj"])
        filled = np.count_nonzero(wa["key"])
        # (the zero prediction of instance 3 is inside every cone: solved, written back like the others)
        assert filled == B, wa["key"]
        second = simt.step_solve(ls, pred * np.float32(1.01), MODE_INNER, sign=-1.0, inner_ratio=RATIO, warm=wc, keys=keys, seed=5)
        assert (second["warm_hit"] == 1).all() and (second["status"] == 0).all()
        again = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, warm=wc, keys=keys)
        assert (again["warm_hit"] == 1).all() and (again["status"] == 0).all()
        assert_matches(again, ref, MODE_INNER, -pred, ("warm", keys is None))
        assert (again["iters"] <= cold["iters"]).all(), (again["iters"], cold["iters"])   # fewer or equal, per instance
        # a negative caller key: no cache for that instance
        if keys is not None:
            k2 = keys.copy()
            k2[1] = -1
            o = simt.step_solve(ls, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, warm=wc, keys=k2)
            assert o["warm_hit"][1] == 0 and o["warm_hit"][[0, 2]].all() and np.array_equal(o["proj"][1], cold["proj"][1])


def _content_key_after(simt, ls, pred, b, n=4):
    """the key the solve half forms for slot b (a one-instance batch through an empty cache leaves exactly one key)"""
    wc, wa = warm_cache(n)
    o = simt.step_solve(ls, pred[b:b + 1], MODE_PROJECT, sign=-1.0, ids=np.array([b]), warm=wc)
    assert o["status"][0] == 0 and np.count_nonzero(wa["key"]) == 1
    return int(wa["key"][wa["key"] != 0][0])


def test_content_key_names_the_cone_and_nothing_else(emul, simt):
    """The content key of a cone is the same at another batch position and with another zero padding (m_max), and differs
    for a cone that differs in one sign byte, in one csr16 word of the THIRD group (entries 16 - 23 of a lane: more than
    1024 non-zeros) or in the count of rows the projection keeps."""
    name = KEY_CASE
    bt = _batch(name, SEEDS[0])
    ctrs, pred, d = bt["ctrs"], bt["pred"], 193
    ls, la, status, keep = store_route(emul, simt, ctrs)
    k0 = _content_key_after(simt, ls, pred, 0)
    assert k0 >> 63 == 1 and (k0 >> 20) & 63 == 27 and (k0 >> 14) & 63 == 19 and k0 & 0x3fff == 1027
    # the same cone in slot 2 of a batch with 50 more rows of padding
    moved = np.zeros((3, ctrs.shape[1] + 50, d), np.float32)
    moved[2, :ctrs.shape[1]] = ctrs[0]
    moved[0, :ctrs.shape[1]] = ctrs[1]
    ls2, la2, st2, keep2 = store_route(emul, simt, moved)
    assert _content_key_after(simt, ls2, np.repeat(pred[:1], 3, 0), 2) == k0
    assert _content_key_after(simt, ls, pred, 1) != k0
    # one sign byte / one csr16 word of the third group / n_valid: each alone changes the key
    for what in ("usign", "csr16", "n_valid"):
        st3, a3 = lite_store(1, d)
        for k in a3:
            per = len(la[k]) // len(ctrs)
            a3[k][:] = la[k][:per]
        if what == "usign":
            k = int(np.flatnonzero(a3["usign"] == 0)[-1])   # a coordinate without a unit row gains one (in the last slot of a lane)
            a3["usign"][k] = 1
        elif what == "csr16":
            # last word of the third group: entries 22 and 23 of lane 63, dummies of this cone (column d, whose
            # residual is always 0: the sign bit of one changes the slot, not the solve)
            w = 4 * (2 * 64 + 63) + 3
            assert a3["hdr"][6] == 24 and a3["csr16"][w] == (d | d << 16)
            a3["csr16"][w] ^= 0x80000000
        else:
            a3["hdr"][4] += 1
        assert _content_key_after(simt, st3, pred, 0) != k0, what


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_small_and_poisoned_caches_change_iterations_never_results(emul, simt, n):
    """A cache of 1, 2 and 4 entries (ways = min(4, n): one set) and of 8 (two sets): more cones than entries evict each
    other and everything still matches the cold kernel's answers to the solver tolerance.  A poisoned cache -- every
    key the right one, multipliers NaN / huge / negative / random -- changes iterations, never results.  A NaN
    prediction clears only its own entry."""
    name = "d64_8f8b_512"
    bt = _batch(name, SEEDS[1])
    ctrs, pred = bt["ctrs"], bt["pred"]
    B = len(ctrs)
    ls, la, status, keep = store_route(emul, simt, ctrs)
    ref = reference(name, SEEDS[1], MODE_PROJECT, 1.0)
    wc, wa = warm_cache(n)
    for rep in range(3):
        o = simt.step_solve(ls, pred, MODE_PROJECT, sign=1.0, warm=wc, seed=rep)
        assert (o["status"] == 0).all()
        assert_matches(o, ref, MODE_PROJECT, pred, ("small cache", n, rep))
        assert np.count_nonzero(wa["key"]) <= n and (rep == 0 or n < 4 or o["warm_hit"].any())
    if n < 4:
        return
    keys = np.arange(B)
    rng = np.random.default_rng(n)
    for poison in ("nan", "huge", "negative", "random"):
        wc, wa = warm_cache(8)
        simt.step_solve(ls, pred, MODE_PROJECT, sign=1.0, warm=wc, keys=keys)
        assert np.count_nonzero(wa["key"]) == B
        wa["theta"][:] = {"nan": np.nan, "huge": 3e37, "negative": -5.0}.get(poison, 0.0)
        if poison == "random":
            wa["theta"][:] = rng.standard_normal(wa["theta"].shape) * 10
        o = simt.step_solve(ls, pred, MODE_PROJECT, sign=1.0, warm=wc, keys=keys)
        assert (o["status"] == 0).all(), (poison, o["status"])
        assert_matches(o, ref, MODE_PROJECT, pred, ("poisoned", poison))
    # a NaN prediction: that instance fails (BAD_INPUT / NOT_CONVERGED, NaN or its own status), clears ITS entry only
    wc, wa = warm_cache(8)
    simt.step_solve(ls, pred, MODE_PROJECT, sign=1.0, warm=wc, keys=keys)
    before = wa["key"].copy()
    bad = pred.copy()
    bad[2, 5] = np.nan
    o = simt.step_solve(ls, bad, MODE_PROJECT, sign=1.0, warm=wc, keys=keys)
    assert o["status"][2] != 0 and (np.delete(o["status"], 2) == 0).all(), o["status"]
    changed = np.flatnonzero(wa["key"] != before)
    assert len(changed) == 1 and wa["key"][changed[0]] == 0 and before[changed[0]] == (2 | (1 << 62))


# ================================================================================================ D6: edges
def test_empty_cone_unpacked_store_single_instance_and_null_prediction(emul, simt):
    d = 40
    ctrs = np.zeros((3, 12, d), np.float32)
    ctrs[1] = _batch("d40_0f1b_2", SEEDS[0])["ctrs"][0][:12]
    pred = np.random.default_rng(0).standard_normal((3, d)).astype(np.float32)
    for route in ("store", "fused"):
        if route == "store":
            ls, la, status, keep = store_route(emul, simt, ctrs)
        else:
            ls, la, status = simt.step_pack(ctrs)
        assert (status == 0).all() and (la["hdr"][0::8] == 1).all() and la["hdr"][4] == 0 and la["hdr"][8 + 4] > 0
        simt.path_counters()
        o = simt.step_solve(ls, pred, MODE_EXACT, sign=1.0)
        assert (o["status"] == 0).all() and simt.path_counters()[6] == 1     # the empty cones solve nothing
        assert np.array_equal(o["proj"][0], pred[0]) and o["rnorm"][0] == 0  # empty cone: proj = y (the reference's rule)
        proj, rnorm = O.batch_project(pred, ctrs)
        assert np.abs(o["proj"] - proj).max() <= TOL * max(1.0, float(np.abs(pred).max()))
        # B = 1
        o1 = simt.step_solve(ls, pred[1:2], MODE_EXACT, sign=1.0, ids=np.array([1]))
        for k in ("proj", "loss", "grad"):
            assert np.array_equal(o1[k][0], o[k][1])
        # pred = NULL with AVG
        a = simt.step_solve(ls, None, MODE_AVG, sign=1.0, B=3)
        assert (a["status"] == 0).all() and np.abs(a["target"] - O.average_ctrs(ctrs)).max() <= TOL
    # a store that was never packed (state 0): CAVE_ST_TOO_LARGE, NaN, for every instance; ZERO_FAILED zeroes loss / grad
    st0, a0 = lite_store(3, d)
    o = simt.step_solve(st0, pred, MODE_INNER, sign=1.0, flags=STEP_ZERO_FAILED)
    assert (o["status"] == ST_TOO_LARGE).all() and np.isnan(o["proj"]).all() and (o["loss"] == 0).all() and (o["grad"] == 0).all()


def test_scratch_rule_of_the_kernel_matches_its_restatement(simt):
    """lite_scratch_fits (cone_step.h, what write_lite_slot asks; exported by the emulation build) against
    tests/limit_cones.scratch_fits, an independent restatement (its own copy of the LDS figure and of the allocation list
    of run_lite_instance), over the whole grid d = 1 .. 256, p = 0 .. 32, nI = 0 .. min(p, 8) -- and the LDS figure itself
    against the product's.  The kernel's rule is a hand-kept replay of the allocations of run_lite_instance: if the two
    drift, the accepted boundary cases of test_a_slot_that_says_one_is_solved... stop being solved in the solve-only arena
    (IN_CASES d256_21f7b / d256_19f8b: the scratch block is the last thing that fits), and the refused ones just beyond
    (SCRATCH_CASES d256_20f8b / d256_22f7b) are what test_cones_beyond_a_limit... expects to be refused.  Documented
    corner at d = 256 (include/cave_hip.h): 32 rows with <= 5 bound rows, 31 with 6, 28 with 7, 27 with 8."""
    for d in range(1, 257):
        assert simt.lib.cave_simt_step_solve_lds_bytes(C.c_int64(d)) == LC.solve_lds_bytes(d) == simt.step_lds_bytes(0, d), d
        for p in range(0, 33):
            for nI in range(0, min(p, 8) + 1):
                assert simt.lite_scratch_fits(d, p, nI) == LC.scratch_fits(d, p, nI), (d, p, nI)
    for nI, pmax in ((0, 32), (5, 32), (6, 31), (7, 28), (8, 27)):
        assert simt.lite_scratch_fits(256, pmax, nI) and (pmax == 32 or not simt.lite_scratch_fits(256, pmax + 1, nI)), (nI, pmax)
    for c in LC.IN_CASES:
        assert simt.lite_scratch_fits(c.d, c.p, c.n_bound), c.name
    for c in LC.SCRATCH_CASES:
        assert not simt.lite_scratch_fits(c.d, c.p, c.n_bound) and c.p <= 32 and c.n_bound <= 8 and c.nnz <= 1536, c.name
