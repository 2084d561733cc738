"""CPU tier: the SPARSE pack half of the fused step kernel (cone_step.h run_pack_sparse_lite_instance) under the SIMT
emulation, against the dense pack half on the densified batch.

The claim of the feature is an identity, not a tolerance: from the same non-zeros, load_sparse_and_build<C, false, true>
hands build_cone the same input in the same arena (the LDS and the non-zero capacity of step_limits, no dump slots) as
scan_and_build<C, false, true>, so the lite store gets the same bits and pack_status the same verdicts.  Both routes run
here on BlockCtx<2, true>, LDS an exact-size poisoned heap block (tests/emul/simt_step_sparse.cpp), round-robin and one
shuffled lane schedule, into freshly zeroed stores: all seven arrays of the store must be equal element for element.

Inputs: the reference's own fixtures (structured.npz tsp20, sp5), every tests/limit_cones.py case with d <= 228 (the
fused form's limit) -- cones ON the lite solver's limits, refused ones included -- buffers sliced at every 16-byte
residue (the loader's 16-byte path with head and tail, and its single-entry path), and a batch of malformed instances.
The solve half then runs on a sparse-packed store against the golden outputs at the tolerances of golden_cases.py.
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import os
import subprocess
import sys

import numpy as np
import pytest

import limit_cones as LC
from emul_lib import ST_BAD_INPUT, ST_TOO_LARGE
from emul_step_sparse_lib import SimtStepSparse, build, shifted, sparse_of
from golden_cases import MODE_INNER, TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAYS = ("hdr", "usign", "avg", "rowptr", "ell", "csr16", "rl")
SEEDS = (0, 17)   # round robin, one shuffled schedule
LIMIT_CASES = [c for c in LC.IN_CASES + LC.OUT_CASES + LC.SCRATCH_CASES if c.d <= 228]


@pytest.fixture(scope="module")
def simt():
    return SimtStepSparse()


def assert_stores_equal(a, b, what):
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def slot_bytes(arrs, b, d):
    """every byte of slot b, array by array"""
    per = {"hdr": 8, "usign": d, "avg": d, "rowptr": 33, "ell": 4 * d, "csr16": 768, "rl": 32}
    return {k: arrs[k][per[k] * b: per[k] * (b + 1)].view(np.uint8).copy() for k in ARRAYS}


def both_routes(simt, ctrs, seed):
    ctrs = np.ascontiguousarray(ctrs, np.float32)
    B, m, d = ctrs.shape
    assert simt.step_lds_bytes(m, d) > 0, (m, d)   # the shape qualifies for the fused form: asserted, not skipped
    off, key, val = sparse_of(ctrs)
    _, da, ds = simt.step_pack(ctrs, seed=seed)
    _, sa, ss = simt.step_pack_sparse(off, key, val, m, d, seed=seed)
    assert np.array_equal(ds, ss), (ds, ss)
    assert_stores_equal(da, sa, seed)
    return sa, ss


def test_case_lists_are_what_the_issue_names():
    names = {c.name for c in LIMIT_CASES}
    assert {"d193_19f8b_1027", "d64_8f8b_512", "d40_0f1b_2", "d40_1f0b_2"} == {c.name for c in LC.IN_CASES if c.d <= 228}
    assert {c.name for c in LC.OUT_CASES if c.d <= 228} <= names and len([c for c in LC.OUT_CASES if c.d <= 228]) == 5
    assert {c.name for c in LC.SCRATCH_CASES if c.d <= 228} == {"d120_24f8b_960"}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("tag,shape", [("tsp20", (16, 235, 190)), ("sp5", (32, 90, 40))])
def test_fixture_stores_are_equal_on_both_routes(simt, golden, tag, shape, seed):
    ctrs = golden["structured"][f"{tag}_ctrs"]
    assert ctrs.shape == shape
    arrs, status = both_routes(simt, ctrs, seed)
    assert (status == 0).all() and (arrs["hdr"][0::8] == 1).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", LIMIT_CASES, ids=lambda c: c.name)
def test_limit_cone_stores_are_equal_on_both_routes(simt, case, seed):
    """B = 6, the dense block padded with zero rows until the pack half's budget of 4 (m_max + d) + 128 non-zeros holds
    the batch's entries: "in" cases are taken (state 1, the header the case claims), the spoiled instance of an "out"
    case and every instance of a "scratch" case are refused (state -1, CAVE_ST_TOO_LARGE) -- on both routes alike."""
    bt0 = LC.batch(case, 11 + seed, B=6)
    m = LC.m_max_for_fused(bt0["ctrs"], case.d)
    bt = LC.batch(case, 11 + seed, B=6, m_max=m)
    arrs, status = both_routes(simt, bt["ctrs"], seed)
    state = arrs["hdr"][0::8]
    if case.kind == "in":
        assert (status == 0).all() and (state == 1).all()
        for b in range(6):
            h = arrs["hdr"][8 * b: 8 * b + 8]
            assert (h[1], h[2], h[3], h[5], h[6]) == LC.header_of(case, bt["rows"][b]), (b, h)
    elif case.kind == "out":
        assert status[1] == ST_TOO_LARGE and state[1] == -1
        assert (np.delete(status, 1) == 0).all() and (np.delete(state, 1) == 1).all()
    else:
        assert (status == ST_TOO_LARGE).all() and (state == -1).all()


def test_loader_alignment(simt, golden):
    """key / val at every 16-byte residue: o_v = o_k (bases congruent modulo 16: 16-byte groups with a head and a tail) and
    o_v = o_k + 1 (not congruent: one entry at a time).  Eight combinations, each the store of the unshifted batch."""
    ctrs = golden["structured"]["tsp20_ctrs"]
    B, m, d = ctrs.shape
    off, key, val = sparse_of(ctrs)
    _, base, bstatus = simt.step_pack_sparse(off, shifted(key, 0), shifted(val, 0), m, d)
    assert (bstatus == 0).all()
    starts, heads = set(), set()
    for ok in range(4):
        for ov in (ok, (ok + 1) % 4):
            k, v = shifted(key, ok), shifted(val, ov)
            for b in range(B):
                a = k.ctypes.data + 4 * int(off[b])
                starts.add((a % 16) // 4)
                if ov == ok:
                    heads.add(min(((16 - a % 16) % 16) // 4, int(off[b + 1] - off[b])))
            _, arrs, status = simt.step_pack_sparse(off, k, v, m, d, seed=ok + 1)
            assert np.array_equal(status, bstatus), (ok, ov)
            assert_stores_equal(base, arrs, (ok, ov))
    # the precondition of this test: instance start addresses at all four residues, heads of 0 .. 3 entries
    assert starts == {0, 1, 2, 3} and heads == {0, 1, 2, 3}, (starts, heads)


def test_per_instance_outcomes(simt, golden):
    """one batch: an instance without entries (the empty cone), one with nnz_cap + 1 entries, six malformed ones -- every
    other slot keeps the bits of the clean batch"""
    ctrs = golden["structured"]["tsp20_ctrs"]
    B, m, d = ctrs.shape
    off, key, val = sparse_of(ctrs)
    _, clean, cstatus = simt.step_pack_sparse(off, key, val, m, d)
    assert (cstatus == 0).all()
    cap = simt.step_nnz_cap(m, d)
    assert cap == 4 * (m + d) + 128
    parts = [(key[off[b]:off[b + 1]].copy(), val[off[b]:off[b + 1]].copy()) for b in range(B)]
    parts[0] = (np.zeros(0, np.uint32), np.zeros(0, np.float32))
    flat = np.arange(cap + 1, dtype=np.int64)
    parts[1] = ((((flat // d) << 16) | (flat % d)).astype(np.uint32), np.ones(cap + 1, np.float32))
    assert (flat // d).max() < m

    def spoil(b, f):
        k, v = parts[b]
        assert len(k) > 8
        f(k, v)

    def unsorted(k, v): k[[3, 4]] = k[[4, 3]]
    def repeated(k, v): k[5] = k[4]
    def row_out(k, v): k[-1] = (m << 16) | (k[-1] & 0xffff)
    def col_out(k, v): k[-1] = (k[-1] & 0xffff0000) | d
    def zero(k, v): v[2] = 0.0
    def nan(k, v): v[len(v) // 2] = np.nan
    bad = {2: unsorted, 3: repeated, 4: row_out, 5: col_out, 6: zero, 7: nan}
    for b, f in bad.items():
        spoil(b, f)
    off2 = np.concatenate([[0], np.cumsum([len(k) for k, _ in parts])]).astype(np.int64)
    key2, val2 = np.concatenate([k for k, _ in parts]), np.concatenate([v for _, v in parts])
    for seed in SEEDS:
        _, arrs, status = simt.step_pack_sparse(off2, key2, val2, m, d, seed=seed)
        state = arrs["hdr"][0::8]
        assert status[0] == 0 and state[0] == 1 and arrs["hdr"][1] == 0 and arrs["hdr"][4] == 0   # empty cone: no rows
        assert status[1] == ST_TOO_LARGE and state[1] == -1
        for b in bad:
            assert status[b] == ST_BAD_INPUT and state[b] == -1, (b, status[b], state[b])
        for b in range(8, B):
            assert status[b] == 0
            sa, sb = slot_bytes(clean, b, d), slot_bytes(arrs, b, d)
            assert all(np.array_equal(sa[k], sb[k]) for k in ARRAYS), b


@pytest.mark.parametrize("tag", ["tsp20", "sp5"])
def test_solve_half_on_a_sparse_packed_store(simt, golden, tag):
    """mode INNER, both senses, against the reference's outputs (tolerances of tests/golden_cases.py)"""
    g = golden["structured"]
    ctrs, costs = g[f"{tag}_ctrs"], g[f"{tag}_costs"]
    B, m, d = ctrs.shape
    off, key, val = sparse_of(ctrs)
    st, arrs, status = simt.step_pack_sparse(off, key, val, m, d, seed=3)
    assert (status == 0).all()
    for sense, sign in (("min", -1.0), ("max", 1.0)):
        ok = g[f"{tag}_{sense}_consistent"]
        sc = np.maximum(1.0, np.abs(costs).max(axis=1))[:, None]
        o = simt.step_solve(st, costs, MODE_INNER, sign=sign, inner_ratio=0.2, m_max=m, seed=5)
        assert (o["status"] == 0).all()
        assert np.all(np.abs(o["proj"] - g[f"{tag}_{sense}_proj"])[ok] <= (TOL * sc * np.ones_like(o["proj"]))[ok])
        rn = g[f"{tag}_{sense}_rnorm"]
        assert np.all(np.abs(o["rnorm"] - rn)[ok] <= TOL * np.maximum(1.0, rn)[ok])
        assert np.all(np.abs(o["loss"] - g[f"{tag}_{sense}_inner_loss"])[ok] <= TOL)
        assert np.all(np.abs(o["target"] - g[f"{tag}_{sense}_inner_target"])[ok] <= TOL * 4)
        gs = np.maximum(1.0, np.abs(g[f"{tag}_{sense}_inner_grad"]).max())
        assert np.all(np.abs(o["grad"] - g[f"{tag}_{sense}_inner_grad"])[ok] <= TOL * 4 * gs)


def test_sparse_pack_half_is_asan_ubsan_clean():
    """tsp20 and the d = 193 limit case under AddressSanitizer + UBSan: the LDS block has no slack behind the arena, so a
    store past the `cap` entries the DEEP form reserves (it has no dump slots) would be reported here"""
    import emul_lib

    emul_lib.build_simt(asan=True)
    build(asan=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    code = (
        "import sys; sys.path[:0]=[%r,%r]\n"
        "import numpy as np, ctypes as C\n"
        "import emul_step_sparse_lib as L, limit_cones as LC\n"
        "S = L.SimtStepSparse(asan=True)\n"
        "g = np.load(%r)\n"
        "case = [c for c in LC.IN_CASES if c.name == 'd193_19f8b_1027'][0]\n"
        "bt0 = LC.batch(case, 11, B=6)\n"
        "bt = LC.batch(case, 11, B=6, m_max=LC.m_max_for_fused(bt0['ctrs'], case.d))\n"
        "for ctrs in (g['tsp20_ctrs'], bt['ctrs']):\n"
        "    B, m, d = ctrs.shape\n"
        "    off, key, val = L.sparse_of(ctrs)\n"
        "    _, da, ds = S.step_pack(ctrs, seed=2)\n"
        "    for ok, ov in ((0, 0), (3, 3), (1, 2)):\n"
        "        _, sa, ss = S.step_pack_sparse(off, L.shifted(key, ok), L.shifted(val, ov), m, d, seed=4)\n"
        "        assert (ss == 0).all() and np.array_equal(ds, ss)\n"
        "        assert all(np.array_equal(da[k], sa[k]) for k in da)\n"
        "print('asan-ok')\n" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden", "structured.npz")))
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "asan-ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
