"""CPU tier: the INTERIOR-POINT solve half of the fused step kernel (cone_step.h run_lite_instance<SoloCtx<32, 4>, false,
IPM>, cone_core.h lite_solve_ipm) under the SIMT emulation, one 64-lane wave per instance, LDS an exact-size poisoned
heap block (tests/emul/simt_step_ipm.cpp), round-robin and one shuffled lane schedule.

At max_iter 1 and 3 it is compared with the EXISTING general kernel in the same mode on the same inputs (the serial
build, Emul().cone_dense) at the tolerances of tests/golden_cases.py; the general kernel's own spread between one wave
and four waves per instance is measured beside it (tests/step_ipm_cases.py says what "agree" means).  The properties of
tests/test_ipm_mode.py -- strictly interior by LP at three steps, rnorm is the iterate's residual, at 40 steps within
4e-6 of the oracle's projection -- are checked with that file's own functions.

Inputs: structured.npz tsp20 (all 16) and sp5[:8]; the cones of tests/limit_cones.py on the lite solver's limits (d =
256 / 255 / 193, 32 rows, 8 bound rows, 1536 and 1027 non-zeros, every column full), each with a zero prediction and
predictions of size 1e-6 and 1e3; the empty cone, a cone of unit rows only, a batch of one.  No instance is left out:
every one comes back CAVE_ST_OK with iters == max_iter (0 where there is no reduced row).
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import os
import subprocess
import sys

import numpy as np
import pytest

import limit_cones as LC
import step_ipm_cases as SC
from emul_lib import ST_BAD_INPUT, ST_TOO_LARGE, STEP_ZERO_FAILED, Emul, lite_store
from emul_step_ipm_lib import SimtStepIpm, build
from test_ipm_mode import MODE_IPM, check_ipm_properties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 17)   # round robin, one shuffled schedule
OUT = ("proj", "rnorm", "target", "loss", "grad", "status", "iters")
RECORD = {}   # figures of this run (tools/diag/ipm_margins.py writes them to profiles/step_ipm_margins.json)


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    """after the last test of this file: the figures the comparisons recorded, written where CAVE_IPM_MARGINS_OUT says"""
    yield
    SC.write_record(RECORD)


@pytest.fixture(scope="module")
def simt():
    return SimtStepIpm()


@pytest.fixture(scope="module")
def emul():
    return Emul()


def store_route(emul, simt, ctrs, seed=0):
    """Emul.pack -> run_lite_from_packed: how a device-resident store gets its lite slots (any d <= 256)"""
    st, arrs, mr, mn = emul.pack(ctrs, nnz_cap=LC.dense_nnz(ctrs) + 64, lds_bytes=160 * 1024)
    ls, la, status = simt.lite_from_packed(st, seed=seed)
    assert (status == 0).all() and (la["hdr"][0::8] == 1).all()
    return ls, la, (st, arrs)


def assert_same_bits(a, b, what):
    for k in OUT:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


@pytest.mark.parametrize("name", ["tsp20", "sp5"])
def test_fixtures_agree_with_the_general_kernel(simt, emul, golden, name):
    ctrs, costs = SC.fixture_inputs(golden)[name]
    B, m, d = ctrs.shape
    assert (B, m, d) == {"tsp20": (16, 235, 190), "sp5": (8, 90, 40)}[name]
    st, arrs, status = simt.step_pack(ctrs)
    assert (status == 0).all() and (arrs["hdr"][0::8] == 1).all()
    outs = {}
    for k in (1, 3):
        ref = emul.cone_dense(ctrs, costs, MODE_IPM, sign=SC.SIGN, max_iter=k)
        g1, g4 = simt.general_ipm(ctrs, costs, k, 1), simt.general_ipm(ctrs, costs, k, 4)
        assert (ref["status"] == 0).all() and (g1["status"] == 0).all() and (g4["status"] == 0).all()
        for seed in SEEDS:
            o = simt.step_solve_ipm(st, costs, sign=SC.SIGN, max_iter=k, m_max=m, seed=seed)
            assert (o["status"] == 0).all() and (o["iters"] == k).all(), (name, k, seed, o["status"], o["iters"])
            SC.compare(o, ref, g1, g4, SC.SIGN * costs, f"cpu/{name}/max_iter={k}/seed={seed}", RECORD)
            if seed:
                assert_same_bits(o, outs[k], (name, k, "schedule"))   # the lane schedule changes nothing
            outs[k] = o
    assert np.abs(outs[1]["loss"] - outs[3]["loss"]).max() > 1e-4   # max_iter is honoured
    # max_iter <= 0 means 3; the solve-only launch's smaller arena gives the same bits
    o = simt.step_solve_ipm(st, costs, sign=SC.SIGN, max_iter=0, m_max=0, seed=3)
    assert_same_bits(o, outs[3], (name, "default steps, solve-only arena"))


@pytest.mark.parametrize("name", SC.LIMIT_NAMES)
def test_limit_cones_agree_with_the_general_kernel(simt, emul, name):
    """store route (any d), solve-only launch: the LDS block is step_solve_lds_bytes(d) exactly"""
    bt = SC.limit_batch(name)
    ctrs, pred = bt["ctrs"], bt["pred"]
    d = ctrs.shape[2]
    assert (pred[3] == 0).all()
    ls, la, keep = store_route(emul, simt, ctrs)
    for b in range(len(ctrs)):
        h = la["hdr"][8 * b: 8 * b + 8]
        assert (h[1], h[2], h[3], h[5], h[6]) == LC.header_of(bt["case"], bt["rows"][b]), (b, h)
    cap, lds = LC.dense_nnz(ctrs) + 64, 160 * 1024
    for k in (1, 3):
        ref = emul.cone_dense(ctrs, pred, MODE_IPM, sign=SC.SIGN, max_iter=k, nnz_cap=cap, lds_bytes=lds)
        g1 = simt.general_ipm(ctrs, pred, k, 1, nnz_cap=cap, lds_bytes=lds)
        g4 = simt.general_ipm(ctrs, pred, k, 4, nnz_cap=cap, lds_bytes=lds)
        assert (ref["status"] == 0).all() and (g1["status"] == 0).all() and (g4["status"] == 0).all()
        prev = None
        for seed in SEEDS:
            o = simt.step_solve_ipm(ls, pred, sign=SC.SIGN, max_iter=k, lds_bytes=LC.solve_lds_bytes(d), seed=seed)
            assert (o["status"] == 0).all() and (o["iters"] == k).all(), (name, k, seed, o["status"], o["iters"])
            SC.compare(o, ref, g1, g4, SC.SIGN * pred, f"cpu/{name}/max_iter={k}/seed={seed}", RECORD)
            if prev is not None:
                assert_same_bits(o, prev, (name, k, "schedule"))
            prev = o


def test_empty_cone_unit_rows_only_zero_prediction_and_a_batch_of_one(simt, emul):
    ctrs, pred, p_want = SC.edge_batch()
    B, m, d = ctrs.shape
    st, arrs, status = simt.step_pack(ctrs)
    assert (status == 0).all() and (arrs["hdr"][0::8] == 1).all()
    assert np.array_equal(arrs["hdr"][1::8], p_want) and arrs["hdr"][4] == 0 and arrs["hdr"][8 + 4] > 0   # rows kept
    for k in (1, 3):
        ref = emul.cone_dense(ctrs, pred, MODE_IPM, sign=SC.SIGN, max_iter=k)
        g1, g4 = simt.general_ipm(ctrs, pred, k, 1), simt.general_ipm(ctrs, pred, k, 4)
        assert (ref["status"] == 0).all()
        for seed in SEEDS:
            o = simt.step_solve_ipm(st, pred, sign=SC.SIGN, max_iter=k, m_max=m, seed=seed)
            assert (o["status"] == 0).all(), o["status"]
            assert np.array_equal(o["iters"], np.where(p_want > 0, k, 0)), o["iters"]
            SC.compare(o, ref, g1, g4, SC.SIGN * pred, f"cpu/edge/max_iter={k}/seed={seed}", RECORD)
        # a batch of one, through ids: slot 3 alone gives the bits it gives in the batch
        one = simt.step_solve_ipm(st, pred[3:4], sign=SC.SIGN, max_iter=k, ids=[3], m_max=m, seed=SEEDS[1])
        for f in OUT:
            assert np.array_equal(one[f][0], o[f][3]), (k, f)
    # the empty cone returns the prediction itself (src/cave.py:304-305)
    assert np.array_equal(o["proj"][0], SC.SIGN * pred[0]) and o["rnorm"][0] == 0


def test_statuses_of_slots_the_kernel_does_not_solve(simt, golden):
    """a never-packed store: CAVE_ST_TOO_LARGE and NaN; an id out of range: CAVE_ST_BAD_INPUT and NaN, zeros under
    CAVE_STEP_ZERO_FAILED; permuted and repeated ids give the rows of the plain launch"""
    ctrs, costs = SC.fixture_inputs(golden)["sp5"]
    B, m, d = ctrs.shape
    blank, keep = lite_store(B, d)
    o = simt.step_solve_ipm(blank, costs, sign=SC.SIGN, max_iter=3, m_max=m)
    assert (o["status"] == ST_TOO_LARGE).all() and (o["iters"] == 0).all()
    assert np.isnan(o["loss"]).all() and np.isnan(o["grad"]).all() and np.isnan(o["proj"]).all()
    st, arrs, status = simt.step_pack(ctrs)
    plain = simt.step_solve_ipm(st, costs, sign=SC.SIGN, max_iter=3, m_max=m)
    ids = np.array([5, 2, 2, 99, 0, 7, -1, 5], np.int64)
    pred = costs[np.clip(ids, 0, B - 1)]
    for flags in (0, STEP_ZERO_FAILED):
        o = simt.step_solve_ipm(st, pred, sign=SC.SIGN, max_iter=3, ids=ids, flags=flags, m_max=m, seed=9)
        bad = (ids < 0) | (ids >= B)
        assert np.array_equal(o["status"], np.where(bad, ST_BAD_INPUT, 0))
        for f in OUT:
            assert np.array_equal(o[f][~bad], plain[f][ids[~bad]]), (flags, f)
        assert np.isnan(o["proj"][bad]).all()
        if flags:
            assert (o["loss"][bad] == 0).all() and (o["grad"][bad] == 0).all()
        else:
            assert np.isnan(o["loss"][bad]).all() and np.isnan(o["grad"][bad]).all()


def test_properties_of_the_interior_point_mode(simt, golden):
    """tests/test_ipm_mode.py check_ipm_properties: steps 1, 3, 6, 12, 40; at 3 strictly interior by LP and rnorm the
    iterate's residual; at 40 within 4e-6 of the ORACLE's projection (not of the general kernel: the late systems are
    ill-conditioned)"""
    def run(c, y, k):
        st, arrs, status = simt.step_pack(c)
        assert (status == 0).all()
        return simt.step_solve_ipm(st, y, sign=SC.SIGN, max_iter=k, m_max=c.shape[1])
    check_ipm_properties(run, SC.property_golden(golden))


def test_ipm_solve_half_is_asan_ubsan_clean():
    """tsp20 (arena of the fused launch) and three limit cones (store route; the LDS block is step_solve_lds_bytes(d)
    exactly, no slack behind it) under AddressSanitizer + UBSan, one shuffled schedule"""
    import emul_lib

    emul_lib.build(asan=True)
    emul_lib.build_simt(asan=True)
    build(asan=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    code = (
        "import sys; sys.path[:0]=[%r,%r]\n"
        "import numpy as np\n"
        "import emul_lib, emul_step_ipm_lib as L, limit_cones as LC, step_ipm_cases as SC\n"
        "S, E = L.SimtStepIpm(asan=True), emul_lib.Emul(asan=True)\n"
        "g = np.load(%r)\n"
        "c, y = g['tsp20_ctrs'], g['tsp20_costs']\n"
        "st, arrs, status = S.step_pack(c, seed=2)\n"
        "o = S.step_solve_ipm(st, y, max_iter=3, m_max=c.shape[1], seed=4)\n"
        "assert (o['status'] == 0).all() and (o['iters'] == 3).all()\n"
        "for name in ('d256_16f8b_1536', 'd256_27f5b_1536', 'd193_19f8b_1027'):\n"
        "    bt = SC.limit_batch(name)\n"
        "    c, y = bt['ctrs'], bt['pred']\n"
        "    ps, pa, mr, mn = E.pack(c, nnz_cap=LC.dense_nnz(c) + 64, lds_bytes=160 * 1024)\n"
        "    ls, la, status = S.lite_from_packed(ps, seed=2)\n"
        "    assert (status == 0).all()\n"
        "    o = S.step_solve_ipm(ls, y, max_iter=3, lds_bytes=LC.solve_lds_bytes(c.shape[2]), seed=4)\n"
        "    assert (o['status'] == 0).all() and (o['iters'] == 3).all()\n"
        "print('asan-ok')\n" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "structured.npz")))
    pre = os.environ.get("LD_PRELOAD")
    env = dict(os.environ, LD_PRELOAD=libasan + (" " + pre if pre else ""),
               ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "asan-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])

