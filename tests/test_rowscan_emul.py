"""CPU tier: the ROW scan of the step kernel's dense pack half (BlockCtx::scan_rows, ctx_block.h; build_cone<C, true>,
cone_core.h) under the SIMT emulation.

The scan classifies the rows with one non-zero while they are in registers and stores only the rows with two or more;
the claim is an identity: the lite slot and `status` hold the bits they held when every non-zero was stored and
classified afterwards.  The reference is the SPARSE route (load_sparse_and_build -> build_cone without the flag), an
untouched producer of the same slot from the same non-zeros in the same arena: every array of the store and the pack
status must be equal byte for byte, under the round-robin lane schedule and a shuffled one.  The sparse wire format
refuses NaN / Inf entries, so the instances that carry one are compared with the third producer instead, the general pack
(serial scan_dense -> build_cone) -> run_lite_from_packed, word for word over the cone's extent.  For every instance
the lite solver takes, the fused-step outputs (mode INNER) are held against oracle.cave_oracle at the tolerances of
tests/golden_cases.py -- every instance with finite entries, none left out.

Shapes are the smallest that reach each path of the scan: d on both sides of every multiple of 64 (one to four loads
per row), m below, at and above the 16 rows of a round of two waves, every 4-byte residue of the instance base with an
odd d (rows then start at every alignment), rows of 64 and 65 entries (kLongRow), and the non-zero capacity met exactly.
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import os
import subprocess
import sys

import numpy as np
import pytest

import limit_cones as LC
from emul_lib import ST_TOO_LARGE, Emul
from emul_step_sparse_lib import SimtStepSparse, build, shifted, sparse_of
from golden_cases import MODE_INNER, TOL
from oracle import cave_oracle as O
from rowscan_cases import batch_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("hdr", "usign", "avg", "rowptr", "ell", "csr16", "rl")
SEEDS = (0, 17)   # round robin, one shuffled schedule
RATIO = 0.2
DS = (1, 3, 5, 63, 64, 65, 190, 255, 256)   # the issue's list
MS = (1, 2, 9, 235)
# d = 255 and 256 have no fused launch at any m (step_limits: six workgroups of the solve arena do not fit a compute unit
# beyond d = 228), so the product never runs the dense pack half there and the emulation refuses to.  193 and 228 -- the
# first and the last d of a fused launch with FOUR loads per row -- stand in for them.  128 and 192: the last load of a row
# is a full one (no clamped lane) with two and three loads per row; with four that is d = 256 alone, which has no launch.
DS_RUN = tuple(d for d in DS if d <= 228) + (128, 192, 193, 228)
LIMIT_CASES = [c for c in LC.IN_CASES + LC.OUT_CASES + LC.SCRATCH_CASES if c.d <= 228]
DROP = np.float32(1e-7)   # kDropRowAbsSum = kAvgRowNorm (cone_common.h)


@pytest.fixture(scope="module")
def simt():
    return SimtStepSparse()


@pytest.fixture(scope="module")
def emul():
    return Emul()


# ------------------------------------------------------------------------------------------------------ the checks
def assert_stores_equal(a, b, what):
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def both_routes(simt, ctrs, seed):
    """dense route (the row scan) and sparse route on the same instances: equal status, equal store bytes"""
    assert ctrs.dtype == np.float32 and ctrs.flags.c_contiguous   # used where it lies (the alignment tests place it)
    B, m, d = ctrs.shape
    assert simt.step_lds_bytes(m, d) > 0, (m, d)   # the shape has a fused launch: asserted, not skipped
    off, key, val = sparse_of(ctrs)
    st, da, ds = simt.step_pack(ctrs, seed=seed)
    _, sa, ss = simt.step_pack_sparse(off, key, val, m, d, seed=seed)
    assert np.array_equal(ds, ss), (ds, ss)
    assert_stores_equal(da, sa, seed)
    return st, da, ds


def assert_oracle(simt, st, ctrs, rows, seed, what):
    """mode INNER, sense min, of the solve half on the packed store against the oracle's own functions, instances `rows`"""
    B, m, d = ctrs.shape
    rng = np.random.default_rng([seed, 31, m, d])
    pred = rng.standard_normal((B, d)).astype(np.float32)
    o = simt.step_solve(st, pred, MODE_INNER, sign=-1.0, inner_ratio=RATIO, m_max=m, seed=seed)
    rows = np.asarray(rows)
    assert (o["status"][rows] == 0).all(), (what, o["status"])
    c, y, p = ctrs[rows], -pred[rows], pred[rows]
    proj, rnorm = O.batch_project(y, c)
    target = O.inner_target(y, c, RATIO)[0]
    loss, grad = O.cone_loss(p, target, -1.0), O.cone_loss_grad(p, target, -1.0)
    sc = np.maximum(1.0, np.abs(y).max(axis=1))[:, None]
    assert np.all(np.abs(o["proj"][rows] - proj) <= TOL * sc), (what, "proj")
    assert np.all(np.abs(o["rnorm"][rows] - rnorm) <= TOL * np.maximum(1.0, rnorm)), (what, "rnorm")
    assert np.all(np.abs(o["target"][rows] - target) <= 4 * TOL), (what, "target")
    assert np.all(np.abs(o["loss"][rows] - loss) <= TOL), (what, "loss")
    assert np.all(np.abs(o["grad"][rows] - grad) <= 4 * TOL * max(1.0, float(np.abs(grad).max()))), (what, "grad")


def slot_words(arrs, b, d):
    """the words of slot b that belong to the cone it holds (what lies beyond is left as it was by either producer)"""
    h = arrs["hdr"][8 * b: 8 * b + 8]
    p, chn8 = int(h[1]), int(h[6])
    return {"hdr": h.copy(), "usign": arrs["usign"][b * d:(b + 1) * d].copy(), "avg": arrs["avg"][b * d:(b + 1) * d].copy(),
            "rowptr": arrs["rowptr"][33 * b: 33 * b + p + 1].copy(),
            "ell": arrs["ell"][4 * d * b: 4 * d * (b + 1)].copy() if p > 0 else np.zeros(0, np.uint32),
            "csr16": arrs["csr16"][768 * b: 768 * b + 32 * chn8].copy(), "rl": arrs["rl"][32 * b: 32 * b + p].copy()}


# ========================================================================================================= shapes
def test_shape_list_is_what_the_issue_names(simt):
    have = {(m, d) for d in DS + DS_RUN for m in MS if simt.step_lds_bytes(m, d) > 0}
    assert have == {(m, d) for d in DS_RUN for m in MS} - {(235, 228)}   # (235, 228): the pack arena is the larger one there
    assert max(d for d in range(1, 257) if simt.step_lds_bytes(9, d) > 0) == 228


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("d", DS_RUN)
def test_every_shape_on_both_routes_and_against_the_oracle(simt, d, seed):
    for m in MS:
        if (m, d) == (235, 228):
            continue  # no fused launch (test_shape_list_is_what_the_issue_names)
        ctrs = batch_of(seed, m, d)
        st, arrs, status = both_routes(simt, ctrs, seed)
        assert (status == 0).all() and (arrs["hdr"][0::8] == 1).all(), (m, d, status)
        assert_oracle(simt, st, ctrs, range(len(ctrs)), seed, (m, d))


@pytest.mark.parametrize("m,d", [(9, 5), (20, 65)])
def test_every_residue_of_the_instance_base(simt, m, d):
    """the batch at each of the four 4-byte residues of a 16-byte line; d is odd, so the rows of an instance start at
    every residue too.  Each placement gives the store of the aligned one."""
    ctrs = batch_of(3, m, d, B=3)
    _, base, bstatus = both_routes(simt, shifted(ctrs.ravel(), 0).reshape(ctrs.shape), 0)
    assert (bstatus == 0).all()
    starts = set()
    for o in range(4):
        c = shifted(ctrs.ravel(), o).reshape(ctrs.shape)
        assert c.ctypes.data % 16 == 4 * o
        starts |= {((c.ctypes.data + 4 * (b * m + r) * d) % 16) // 4 for b in range(3) for r in range(m)}
        _, arrs, status = simt.step_pack(c, seed=o)
        assert np.array_equal(status, bstatus)
        assert_stores_equal(base, arrs, o)
    assert starts == {0, 1, 2, 3}


# =================================================================================================== special rows
D_SP, M_SP = 70, 24   # two loads per row, the second one partial; a round and a half of rows


def special_batch():
    """-> (ctrs [B, 24, 70], names, finite [B], takes [B]): one instance per special row, on a common qualifying cone
    (two free rows + one bound row).  takes: the lite solver takes the instance (state 1)."""
    rng = np.random.default_rng(70)
    base = np.zeros((M_SP, D_SP), np.float32)
    a = np.zeros(D_SP, np.float32); a[[1, 9, 40, 66, 69]] = [1, -1, 1, 1, -1]
    b = np.zeros(D_SP, np.float32); b[[2, 3, 63, 64]] = [1, 1, -1, -1]
    base[0], base[1], base[2], base[3] = a, b, -a, -b
    base[4, [10, 65]] = [1.0, 1.0]
    for i, k in enumerate((5, 20, 41, 68)):
        base[5 + i, k] = 1.0 if i % 2 else -1.0
    free_row = 9   # rows 9 .. 23 are zero in the base

    def with_rows(*rows):
        c = base.copy()
        for i, (cols, vals) in enumerate(rows):
            c[free_row + i, cols] = vals
        return c

    below, above = np.nextafter(DROP, np.float32(0)), np.nextafter(DROP, np.float32(1))
    items = [
        ("all_zero", np.zeros_like(base), True, True),
        ("padding_middle_and_end", with_rows(([], []), ([], []), ([30], [1.0])), True, True),
        ("plus_e_k_twice", with_rows(([30], [1.0]), ([30], [1.0])), True, True),
        ("plus_and_minus_e_k", with_rows(([67], [1.0]), ([67], [-1.0])), True, True),
        ("unit_value_2p5", with_rows(([30], [2.5]), ([67], [-0.25])), True, True),
        ("unit_at_the_drop_threshold", with_rows(([30], [DROP]), ([31], [-DROP])), True, True),
        ("unit_just_under_the_threshold", with_rows(([30], [below]), ([66], [-below])), True, True),
        ("unit_just_over_the_threshold", with_rows(([30], [above]), ([66], [-above])), True, True),
        ("unit_nan", with_rows(([30], [np.nan]), ([67], [1.0])), False, True),
        ("unit_plus_inf", with_rows(([30], [np.inf])), False, True),
        ("unit_minus_inf", with_rows(([67], [-np.inf])), False, True),
        ("unit_minus_zero", with_rows(([30], [-0.0]), ([31], [1.0])), True, True),
        ("two_entries_in_one_16_bytes", with_rows(([4, 5], [1.0, -1.0])), True, True),
        ("row_of_64", with_rows((list(range(3, 67)), rng.choice(np.array([-1.0, 1.0], np.float32), 64))), True, True),
        ("row_of_65", with_rows((list(range(2, 67)), rng.choice(np.array([-1.0, 1.0], np.float32), 65))), True, True),
        ("one_entry_2_among_pm1", with_rows(([7, 8, 50], [1.0, 2.0, -1.0])), True, False),
        ("general_valued", (base * rng.uniform(0.5, 1.5, base.shape)).astype(np.float32), True, False),
    ]
    names = [n for n, *_ in items]
    return np.stack([c for _, c, *_ in items]), names, np.array([f for *_, f, _ in items]), np.array([t for *_, t in items])


@pytest.mark.parametrize("seed", SEEDS)
def test_special_rows(simt, emul, seed):
    """instances with finite entries: both routes, byte for byte; an instance the lite solver does not take says -1 and
    CAVE_ST_TOO_LARGE on both.  NaN / Inf unit rows (the sparse wire format refuses them): the slot of the general
    pack -> run_lite_from_packed, word for word -- a NaN row is dropped, an Inf row is a unit row."""
    ctrs, names, finite, takes = special_batch()
    assert ctrs[names.index("unit_minus_zero"), 9, 30] == 0 and np.signbit(ctrs[names.index("unit_minus_zero"), 9, 30])
    fin = np.flatnonzero(finite)
    st, arrs, status = both_routes(simt, ctrs[fin], seed)
    state = arrs["hdr"][0::8]
    assert np.array_equal(state == 1, takes[fin]) and np.array_equal(status == 0, takes[fin]), (state, status)
    assert (status[~takes[fin]] == ST_TOO_LARGE).all() and (state[~takes[fin]] == -1).all()
    assert_oracle(simt, st, ctrs[fin], np.flatnonzero(takes[fin]), seed, "special")
    # what the rows did: dropped rows do not count, the others do (hdr[4] = rows kept by the projection)
    kept = {n: int(arrs["hdr"][8 * i + 4]) for i, n in enumerate(np.array(names)[fin])}
    assert kept["all_zero"] == 0 and kept["padding_middle_and_end"] == 10 and kept["plus_e_k_twice"] == 11
    assert kept["unit_at_the_drop_threshold"] == 9 and kept["unit_just_under_the_threshold"] == 9
    assert kept["unit_just_over_the_threshold"] == 11 and kept["unit_minus_zero"] == 10 and kept["row_of_65"] == 10
    # non-finite unit rows
    nf = np.flatnonzero(~finite)
    c = np.ascontiguousarray(ctrs[nf])
    _, da, ds = simt.step_pack(c, seed=seed)
    pst, parrs, _, _ = emul.pack(c, nnz_cap=LC.dense_nnz(c) + 64, lds_bytes=160 * 1024)
    _, la, ls = simt.lite_from_packed(pst, seed=seed)
    assert (ds == 0).all() and (ls == 0).all()
    for b in range(len(nf)):
        wa, wb = slot_words(da, b, D_SP), slot_words(la, b, D_SP)
        assert all(np.array_equal(wa[k].view(np.uint8), wb[k].view(np.uint8)) for k in wa), names[nf[b]]
    kept = {names[i]: int(da["hdr"][8 * b + 4]) for b, i in enumerate(nf)}
    assert kept == {"unit_nan": 10, "unit_plus_inf": 10, "unit_minus_inf": 10}
    assert da["usign"][1 * D_SP + 30] == 1 and da["usign"][2 * D_SP + 67] == 2 and da["usign"][0 * D_SP + 30] == 0


# ======================================================================================================= capacity
def capacity_batch(simt):
    """(100, 40): cap = 4 (100 + 40) + 128 = 688.  20 free rows of 16 entries (every column full: 8 entries) arrive
    twice = 640 non-zeros in 40 rows; 48 unit rows make it 688 = cap in instance 0, a 49th makes it cap + 1 in 1."""
    m, d = 100, 40
    cap = simt.step_nnz_cap(m, d)
    assert cap == 4 * (m + d) + 128 == 688
    rows = LC.draw_rows(np.random.default_rng(5), d, 20, 320, 8)
    ctrs = np.zeros((2, m, d), np.float32)
    for b in range(2):
        ctrs[b, :20], ctrs[b, 20:40] = rows, -rows
        for i in range(48 + b):
            ctrs[b, 40 + i, i % d] = 1.0 if i < d else -1.0
    assert [int((c != 0).sum()) for c in ctrs] == [cap, cap + 1]
    assert ((ctrs != 0).sum(2) == 1).sum(1).tolist() == [48, 49]   # the rows are mostly unit rows
    return ctrs


@pytest.mark.parametrize("seed", SEEDS)
def test_capacity_counts_the_unit_rows_that_are_not_stored(simt, seed):
    ctrs = capacity_batch(simt)
    st, arrs, status = both_routes(simt, ctrs, seed)
    assert status.tolist() == [0, ST_TOO_LARGE] and arrs["hdr"][0::8].tolist() == [1, -1]
    assert_oracle(simt, st, ctrs, [0], seed, "cap")


# ==================================================================================================== limit cones
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", LIMIT_CASES, ids=lambda c: c.name)
def test_limit_cones(simt, case, seed):
    """tests/limit_cones.py, B = 2 (instance 1 is the spoiled one of an "out" case): taken, or refused, on both routes alike"""
    bt0 = LC.batch(case, 11 + seed, B=2)
    bt = LC.batch(case, 11 + seed, B=2, m_max=LC.m_max_for_fused(bt0["ctrs"], case.d))
    st, arrs, status = both_routes(simt, bt["ctrs"], seed)
    state = arrs["hdr"][0::8]
    if case.kind == "in":
        assert (status == 0).all() and (state == 1).all()
        assert_oracle(simt, st, bt["ctrs"], [0, 1], seed, case.name)
    elif case.kind == "out":
        assert status.tolist() == [0, ST_TOO_LARGE] and state.tolist() == [1, -1]
        assert_oracle(simt, st, bt["ctrs"], [0], seed, case.name)
    else:
        assert (status == ST_TOO_LARGE).all() and (state == -1).all()


# ====================================================================================================== sanitizers
def test_row_scan_is_asan_ubsan_clean():
    """one to four loads per row, every base residue with an odd d, the special rows and the capacity pair under
    AddressSanitizer + UBSan: the LDS block has no slack behind the arena and the batch none behind its last row"""
    import emul_lib

    emul_lib.build_simt(asan=True)
    build(asan=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    code = (
        "import sys; sys.path[:0]=[%r,%r]\n"
        "import numpy as np\n"
        "import emul_step_sparse_lib as L, test_rowscan_emul as T\n"
        "S = L.SimtStepSparse(asan=True)\n"
        "def run(ctrs, seed, residues=range(4)):\n"
        "    B, m, d = ctrs.shape\n"
        "    off, key, val = L.sparse_of(ctrs)\n"
        "    for o in residues:\n"
        "        exact = np.empty(ctrs.size + o, np.float32)   # (heap block: the last row ends where the block ends)\n"
        "        c = exact[o:].reshape(ctrs.shape); c[...] = ctrs\n"
        "        _, da, ds = S.step_pack(c, seed=seed)\n"
        "        if o == 0:\n"
        "            _, sa, ss = S.step_pack_sparse(off, key, val, m, d, seed=seed)\n"
        "            assert np.array_equal(ds, ss) and all(np.array_equal(da[k], sa[k]) for k in da)\n"
        "            base = da\n"
        "        assert all(np.array_equal(da[k], base[k]) for k in da)\n"
        "for m, d in ((9, 1), (9, 5), (20, 65), (9, 193), (20, 228)):\n"
        "    run(T.batch_of(1, m, d, B=1), 4)\n"
        "run(T.batch_of(1, 235, 190, B=1), 4, residues=(0, 3))\n"
        "ctrs, names, finite, takes = T.special_batch()\n"
        "run(np.ascontiguousarray(ctrs[finite]), 2)\n"
        "S.step_pack(np.ascontiguousarray(ctrs[~finite]), seed=2)\n"
        "run(T.capacity_batch(S), 0)\n"
        "print('asan-ok')\n" % (ROOT, os.path.join(ROOT, "tests")))
    pre = os.environ.get("LD_PRELOAD", "")
    env = dict(os.environ, LD_PRELOAD=(libasan + " " + pre).strip(), ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "asan-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
