"""CPU tier: the cone build ALONE -- build_cone with its producers, compute_avg and the store writers -- against the
plain restatement of the reduction in tests/build_ref.py.

Every other test of the build compares route with route (both share build_cone) or a whole solve with the oracle (which
cannot see a reduction that is wrong but spans the same cone).  Here every producer's store is decoded on the host and
compared with the restated rules: p, vkind, usign, n_valid, flag bit 0, every reduced row and every CSC column EXACTLY,
avg within the bound derived in build_ref.  Inputs: tests/build_cases.py families A (random mixes), B (pairing), D
(thresholds and values) and E (the lite limits).  Family C -- rows whose 12-entry signatures collide -- is where the
build may leave exact twins unpaired (p = 4 where the rule gives 2, outputs unchanged); it is held to
build_ref.is_valid_reduction, to "never pairs rows that are not exact negations", and to the oracle's projection.

Producers: the serial build (Emul.pack, Emul.pack_large), the sparse packs (EmulSparse), run_pack_instance under the
SIMT emulation on WaveCtx, BlockCtx<2> and BlockCtx<4> (Simt.pack: round robin and one shuffled schedule -- the
team-shared signature scan, compact_mask_u8, the one-wave-per-row pass and the atomic CSC fill with its sort write
these stores), and the lite slot writers (Simt.step_pack, SimtStepSparse.step_pack_sparse, Simt.lite_from_packed)
through build_ref.decode_lite.  The worst |avg - ref| / bound per route goes to the file the environment variable
CAVE_BUILD_MARGINS names, tier "emulation" (profiles/build_margins.json is written from such a run and the GPU tier's).
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import os
import sys

import numpy as np
import pytest

import build_cases as BC
import build_ref as BR
import limit_cones as LC
from build_check import FULL_LDS, SEEDS, cases_of, check_lite, check_store, lite_must_pack, nnz_cap, refs_of
from emul_lib import ST_TOO_LARGE, Emul
from emul_sparse_lib import EmulSparse
from emul_step_sparse_lib import SimtStepSparse
from golden_cases import MODE_PROJECT, TOL

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cave_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def emul():
    yield Emul()
    BR.dump_margins("emulation")


@pytest.fixture(scope="module")
def simt():
    yield SimtStepSparse()
    BR.dump_margins("emulation")


@pytest.fixture(scope="module")
def sparse():
    return EmulSparse()


# ------------------------------------------------------------------------------------------------ the inputs
def test_case_lists_are_what_the_issue_names():
    a = cases_of("A")
    assert {(c["ctrs"].shape[2], c["ctrs"].shape[1]) for c in a} == {(d, m) for d in BC.A_DIMS for m in BC.A_ROWS}
    assert len(a) == 2 * len(BC.A_DIMS) * len(BC.A_ROWS)
    for fam in "ABCD":
        for c in cases_of(fam):
            assert 2 <= len(c["ctrs"]) <= 8 and c["ctrs"].shape[1] <= 130 and c["ctrs"].shape[2] <= 256, c["name"]
    praw = [c for c in cases_of("B") if c["name"] == "B_praw"][0]
    got = [sum(t == "general" for t in r["tags"]) for r in refs_of(praw)]
    assert got == [1, 16, 17, 32, 33, 64, 65], got          # NT / TEAM and NT / TEAM + 1 of the 1-, 2- and 4-wave shapes
    forty = [c for c in cases_of("B") if c["name"] == "B_40pairs"][0]
    assert all(r["p"] == 40 and r["vkind"].all() for r in refs_of(forty))
    # the restated rule on the instance the issue measured: two free rows
    assert [(r["p"], r["vkind"].tolist()) for r in refs_of(cases_of("C")[0])] == [(2, [1, 1])] * 3
    # the threshold rows fall where they are meant to: dropped below and at 1e-7, kept above; counted only above
    for name in ("D_thresholds_short", "D_thresholds_long"):
        r = refs_of([c for c in cases_of("D") if c["name"] == name][0])
        assert [x["tags"][1] for x in r] == ["drop", "drop", "general"] + ["general"] * 3, name
        assert [x["n_avg"] for x in r] == [2, 2, 2, 2, 2, 3], name


# ------------------------------------------------------------------------------------------------ packed stores
@pytest.mark.parametrize("fam", "ABCD")
def test_serial_pack(emul, fam):
    for c in cases_of(fam):
        _, arrs, _, _ = emul.pack(c["ctrs"], nnz_cap=nnz_cap(c["ctrs"]), lds_bytes=FULL_LDS)
        check_store(c, arrs, "serial pack")


@pytest.mark.parametrize("fam", "ABCD")
def test_serial_pack_large(emul, fam):
    for c in cases_of(fam):
        _, arrs, _, _ = emul.pack_large(c["ctrs"])
        check_store(c, arrs, "serial pack_large")


@pytest.mark.parametrize("fam", "ABCD")
def test_sparse_packs(sparse, emul, fam):
    for c in cases_of(fam):
        B, m, d = c["ctrs"].shape
        off, key, val = BC.sparse_of(c["ctrs"])
        cap = nnz_cap(c["ctrs"])
        arrs, _, _, st1, st2 = sparse.pack(off, key, val, m, d, nnz_cap=cap, lds_bytes=FULL_LDS)
        assert (st1 == 0).all() and (st2 == 0).all(), (c["name"], st1, st2)
        check_store(c, arrs, "sparse pack")
        arrs, _, _, st1, st2 = sparse.pack_large(off, key, val, m, d, cap, emul.large_slice_bytes(m, d, cap, 1))
        assert (st1 == 0).all() and (st2 == 0).all(), (c["name"], st1, st2)
        check_store(c, arrs, "sparse pack_large")


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("fam", "ABCD")
def test_simt_pack(simt, fam, waves):
    """run_pack_instance on WaveCtx / BlockCtx<2> / BlockCtx<4>, every lane a fiber"""
    for c in cases_of(fam):
        for seed in SEEDS:
            _, arrs, st1, st2 = simt.pack(c["ctrs"], nnz_cap=nnz_cap(c["ctrs"]), lds_bytes=FULL_LDS, waves=waves, seed=seed)
            assert (st1 == 0).all() and (st2 == 0).all(), (c["name"], waves, seed, st1, st2)
            check_store(c, arrs, f"simt pack w{waves}")


# ------------------------------------------------------------------------------------------------ lite slots
def fused_cases(simt, fam):
    """the cases of a family at shapes with a fused launch (step_lds_bytes > 0); m = 0 has no pack half"""
    return [c for c in cases_of(fam) if c["ctrs"].shape[1] > 0 and simt.step_lds_bytes(*c["ctrs"].shape[1:]) > 0]


@pytest.mark.parametrize("fam", "ABCD")
def test_lite_pack_halves(simt, fam):
    """run_pack_lite_instance and run_pack_sparse_lite_instance (BlockCtx<2, true>, poisoned exact-size LDS)"""
    cs = fused_cases(simt, fam)
    assert cs, fam
    for c in cs:
        B, m, d = c["ctrs"].shape
        must = [lite_must_pack(r, c["ctrs"][b], m, d) for b, r in enumerate(refs_of(c))]
        off, key, val = BC.sparse_of(c["ctrs"])
        for seed in SEEDS:
            _, arrs, status = simt.step_pack(c["ctrs"], seed=seed)
            check_lite(c, arrs, status, "simt step_pack", must)
            _, arrs, status = simt.step_pack_sparse(off, key, val, m, d, seed=seed)
            check_lite(c, arrs, status, "simt step_pack_sparse", must)


@pytest.mark.parametrize("fam", "ABCD")
def test_lite_from_packed(emul, simt, fam):
    """run_lite_from_packed over a store of the serial pack, d <= 256 (the d = 256 cases run here only)"""
    for c in cases_of(fam):
        store, keep, _, _ = emul.pack(c["ctrs"], nnz_cap=nnz_cap(c["ctrs"]), lds_bytes=FULL_LDS)   # (keep: the store's arrays)
        for seed in SEEDS:
            _, arrs, status = simt.lite_from_packed(store, seed=seed)
            check_lite(c, arrs, status, "simt lite_from_packed")


# ------------------------------------------------------------------------------------------------ E: the lite limits
@pytest.mark.parametrize("case", BC.family_e(), ids=lambda c: c["name"])
def test_lite_limit_cones_decode_to_the_restated_reduction(emul, simt, case):
    ctrs = case["ctrs"]
    B, m, d = ctrs.shape
    lc = case["limit_case"]
    refs = refs_of(case)
    assert all(r["p"] == lc.p and int(r["vkind"].sum()) == lc.n_free and BR.lite_takes(r, d, LC.scratch_fits) for r in refs)
    store, parrs, _, _ = emul.pack(ctrs, nnz_cap=nnz_cap(ctrs), lds_bytes=FULL_LDS)
    check_store(case, parrs, "serial pack")
    _, arrs, status = simt.lite_from_packed(store, seed=17)
    check_lite(case, arrs, status, "simt lite_from_packed")
    if d <= 228:   # the shapes with a fused launch
        mm = LC.m_max_for_fused(ctrs, d)
        padded = dict(case, name=case["name"] + "_padded", ctrs=LC.batch(lc, 11, B=2, m_max=mm)["ctrs"])
        assert simt.step_lds_bytes(mm, d) > 0
        off, key, val = BC.sparse_of(padded["ctrs"])
        _, arrs, status = simt.step_pack(padded["ctrs"], seed=17)
        assert (status == 0).all()
        check_lite(padded, arrs, status, "simt step_pack")
        _, arrs, status = simt.step_pack_sparse(off, key, val, mm, d, seed=17)
        assert (status == 0).all()
        check_lite(padded, arrs, status, "simt step_pack_sparse")


def assert_projection_is_the_oracles(emul, ctrs, seed):
    B, m, d = ctrs.shape
    y = np.random.default_rng(seed).standard_normal((B, d)).astype(np.float32)
    o = emul.cone_dense(ctrs, y, MODE_PROJECT, sign=1.0, nnz_cap=nnz_cap(ctrs), lds_bytes=FULL_LDS)
    po, ro = O.batch_project(y, ctrs)
    assert (o["status"] == 0).all(), o["status"]
    sc = np.maximum(1.0, np.abs(y).max(axis=1))
    assert np.all(np.abs(o["proj"] - po) <= TOL * sc[:, None]), float(np.abs(o["proj"] - po).max())
    assert np.all(np.abs(o["rnorm"] - ro) <= TOL * np.maximum(1.0, ro)), float(np.abs(o["rnorm"] - ro).max())


def test_collisions_project_as_the_oracle_does(emul):
    for i, c in enumerate(cases_of("C")):
        assert_projection_is_the_oracles(emul, c["ctrs"], 100 + i)


def test_missed_pairs_beyond_the_lite_limit(emul, simt):
    """Five colliding rows with their negations: the rules give five free rows, the build keeps ten bound rows (ten
    entries in the twelve shared columns: both beyond what a lite slot takes).  Every lite producer says state -1 and
    CAVE_ST_TOO_LARGE for that instance alone, and the general path still projects as the oracle does."""
    case = BC.e_missed_pairs()
    ctrs = case["ctrs"]
    B, m, d = ctrs.shape
    ref = refs_of(case)
    assert ref[1]["p"] == 5 and ref[1]["vkind"].all() and BR.lite_takes(ref[1], d, LC.scratch_fits)
    store, parrs, _, _ = emul.pack(ctrs, nnz_cap=nnz_cap(ctrs), lds_bytes=FULL_LDS)
    dec = BR.decode_store(parrs, 1)
    ok, why = BR.is_valid_reduction(ctrs[1], dec, ref[1])
    assert ok and BR.no_false_pairs(ctrs[1], dec), why
    assert dec["p"] == 10 and not dec["vkind"].any()       # the measured deviation: every pair missed
    BR.assert_same(BR.decode_store(parrs, 0), ref[0], "the neighbour")
    assert simt.step_lds_bytes(m, d) > 0
    off, key, val = BC.sparse_of(ctrs)
    for name, (arrs, status) in {
        "step_pack": simt.step_pack(ctrs, seed=17)[1:],
        "step_pack_sparse": simt.step_pack_sparse(off, key, val, m, d, seed=17)[1:],
        "lite_from_packed": simt.lite_from_packed(store, seed=17)[1:],
    }.items():
        assert status.tolist() == [0, ST_TOO_LARGE], (name, status)
        assert BR.decode_lite(arrs, 1, d)["state"] == -1, name
        BR.assert_same(BR.decode_lite(arrs, 0, d), ref[0], name)
    assert_projection_is_the_oracles(emul, ctrs, 7)
