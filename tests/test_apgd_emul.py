"""CPU tier of the APGD projector (cave_amd/csrc/apgd.h): the kernel code under the SIMT emulation with shuffled
schedules, behind the plan function the library calls, against the long-double restatement (tests/apgd_ref.py) within the
derived bounds, and the reference's own fp32 / fp64 runs (tests/golden/apgd.npz, written by tests/golden/make_apgd.py
from the unmodified reference).  The stand-alone sanitizer build runs a selection of the same cases."""

import numpy as np
import pytest

import apgd_cases as AC
import apgd_ref as R
import emul_apgd_lib as E


MARGINS = {}  # with CAVE_APGD_MARGINS=<path>: the largest ratio each check reached, as JSON (profiles/apgd_margins.json)


@pytest.fixture(scope="module")
def simt():
    yield E.SimtApgd()
    import json
    import os

    if os.environ.get("CAVE_APGD_MARGINS"):
        with open(os.environ["CAVE_APGD_MARGINS"], "w") as fh:
            json.dump({"what": "largest deviation / bound reached per check of tests/test_apgd_emul.py (1 = at the bound)",
                       "ratios": MARGINS}, fh, indent=1, sort_keys=True)


CPU_ROWS = {"tsp20": 4}  # instances of a fixture input the CPU tier runs (the GPU tier runs them all)


@pytest.mark.parametrize("name", ["tsp20", "tsp10", "sp5", "randn", "setup"])
def test_fixture_inputs_at_every_stored_count(simt, name):
    """one trajectory through the continuation state, stopped at every stored iteration count (a chain equals the single
    launches bit for bit: test_continuation)"""
    A, y, sign = AC.fixture_inputs()[name]
    n = CPU_ROWS.get(name, A.shape[0])
    cap = AC.max_nnz(A)
    state, k0 = None, 0
    for k in AC.SNAP:
        rc, o = simt.run(A[:n], y[:n], sign=sign, n_iter=k - k0, k_start=k0, cap=cap, state=state, seed=5 + k)
        assert rc == 0, simt.last_error()
        state, k0 = (o["x_curr"], o["x_prev"], o["step"]), k
        MARGINS[f"fixture/{name}/{k}"] = AC.check_fixture_floats(o, name, k, tag="emul", rows=slice(0, n))
    if name == "setup":  # the projection is exactly zero: target 0, loss 1
        assert not o["proj"].any() and not o["target"].any() and (o["loss"] == 1.0).all() and (o["rnorm"] > 0).all()


@pytest.mark.parametrize("name", sorted(AC.shape_cases()))
def test_shapes_against_restatement(simt, name):
    A, y, sign = AC.shape_cases()[name]
    B, m, d = A.shape
    ref, S = AC.reference(name, 20)
    cap = AC.max_nnz(A)
    rc, o = simt.run(A, y, sign=sign, n_iter=20, cap=cap, seed=11)
    assert rc == 0, simt.last_error()
    AC.check_against(o, ref, S, tag=f"shape/{name}", margins=MARGINS)
    # format agreement, workgroup sizes, relaunch: the same bits
    rc, s = simt.run(AC.to_sparse(A), y, sign=sign, n_iter=20, cap=cap, seed=12)
    assert rc == 0
    AC.same_bits(o, s)
    other = 4 if simt.waves(m, d, cap) == 1 else 1
    rc, w = simt.run(A, y, sign=sign, n_iter=20, cap=cap, seed=13, waves=other)
    assert rc == 0
    AC.same_bits(o, w)
    rc, again = simt.run(A, y, sign=sign, n_iter=20, cap=cap, seed=0)
    AC.same_bits(o, again)


@pytest.mark.parametrize("name", ["m65_d70", "m1_d2", "pairs_repeats"])
def test_power_iter_zero_and_project_mode(simt, name):
    A, y, sign = AC.shape_cases()[name]
    ref, S = AC.reference(name, 20, 0)
    rc, o = simt.run(A, y, sign=sign, n_iter=20, power_iter=0, seed=3)
    assert rc == 0
    AC.check_against(o, ref, S, tag=f"power0/{name}", margins=MARGINS)
    rc, p = simt.run(A, y, mode=0, sign=sign, n_iter=20, power_iter=0, seed=4)
    assert rc == 0
    AC.same_bits(o, p, ("proj", "rnorm", "x_curr", "x_prev", "step", "pgrad", "status", "iters"))
    for n in ("target", "loss", "grad"):  # mode PROJECT leaves them alone
        assert (p[n] == 77.0).all()


def test_workgroup_size_rule(simt):
    assert simt.waves(90, 40, 256) == 1 and simt.waves(235, 190, 1200) == 4 and simt.waves(257, 70, 300) == 1
    assert simt.waves(513, 4, 16) == 4 and simt.waves(4, 513, 16) == 4 and simt.waves(64, 64, 513) == 4
    # the shapes that must fit with more than one workgroup per compute unit
    assert 0 < simt.lds_bytes(90, 40, 256) * 2 <= 160 * 1024 and 0 < simt.lds_bytes(235, 190, 1200) * 2 <= 160 * 1024
    assert simt.lds_bytes(235, 190, 235 * 190) == -1 and simt.lds_bytes(0, 4, 1) == -1 and simt.lds_bytes(4, 4, 17) == -1


def test_capacity_exact_and_one_over(simt):
    rng = np.random.default_rng(3)
    A = np.zeros((3, 9, 12), np.float32)
    for b, nnz in enumerate((20, 21, 7)):
        idx = rng.choice(9 * 12, nnz, replace=False)
        A[b].reshape(-1)[idx] = rng.standard_normal(nnz).astype(np.float32)
    y = rng.standard_normal((3, 12)).astype(np.float32)
    for cones, rest in ((A, A[[0, 2]]), (AC.to_sparse(A), AC.to_sparse(A[[0, 2]]))):
        rc, o = simt.run(cones, y, n_iter=10, cap=20, seed=2)
        assert rc == 0 and list(o["status"]) == [0, AC.ST_TOO_LARGE, 0] and o["iters"][1] == 0
        for n in AC.FLOAT_OUT + ("pgrad",):
            assert np.isnan(o[n][1]).all(), n
        assert (o["x_curr"][1] == 77.0).all() and o["step"][1] == 77.0  # its state is left alone
        rc, r = simt.run(rest, y[[0, 2]], n_iter=10, cap=20, seed=9)
        AC.same_bits(o, r, rows=([0, 2], [0, 1]))
        rc, full = simt.run(cones, y, n_iter=10, cap=21, seed=2)
        assert rc == 0 and (full["status"] == 0).all()
        AC.same_bits(o, full, rows=([0, 2], [0, 2]))


def test_bad_input_per_instance(simt):
    A, y, sign = AC.shape_cases()["empty_padding_nocol"]
    m, d, off, key, val = AC.to_sparse(A)
    rc, good = simt.run((m, d, off, key, val), y, n_iter=5)
    assert rc == 0 and (good["status"] == 0).all()
    lo = int(off[0])

    def expect_bad(cones, pred, b):
        rc, o = simt.run(cones, pred, n_iter=5, seed=7)
        assert rc == 0 and o["status"][b] == AC.ST_BAD_INPUT and np.isnan(o["proj"][b]).all() and np.isnan(o["pgrad"][b])
        keep = [i for i in range(len(o["status"])) if i != b]
        AC.same_bits(o, good, AC.FLOAT_OUT + ("pgrad", "status"), rows=(keep, keep))

    k2 = key.copy(); k2[lo + 1] = (m << 16) | 0          # a row out of range
    expect_bad((m, d, off, k2, val), y, 0)
    k2 = key.copy(); k2[lo] = (int(key[lo]) & 0xffff0000) | d  # a column out of range
    expect_bad((m, d, off, k2, val), y, 0)
    k2 = key.copy(); k2[lo + 1], k2[lo + 2] = key[lo + 2], key[lo + 1]  # unsorted
    expect_bad((m, d, off, k2, val), y, 0)
    k2 = key.copy(); k2[lo + 1] = key[lo]                # a repeated key
    expect_bad((m, d, off, k2, val), y, 0)
    for bad in (np.inf, np.nan, 0.0):                    # a value that is not finite and non-zero
        v2 = val.copy(); v2[int(off[2])] = bad
        expect_bad((m, d, off, key, v2), y, 2)
    y2 = y.copy(); y2[3, 1] = np.nan
    expect_bad((m, d, off, key, val), y2, 3)
    expect_bad(A, y2, 3)
    A2 = A.copy(); A2[0, 0, 0] = -np.inf
    expect_bad(A2, y, 0)


def test_argument_errors_and_their_texts(simt):
    A = np.ones((2, 3, 4), np.float32)
    y = np.ones((2, 4), np.float32)
    out = [np.zeros(24) for _ in range(3)] + [None] * 8

    def err(text, cones=A, pred=y, dims=(2, 3, 4), mode=1, sign=1.0, k_start=0, n_iter=5, power_iter=8, cap=12, ptrs=out):
        rc = simt.raw(cones, pred, dims, mode, sign, k_start, n_iter, power_iter, cap, ptrs)
        assert rc == -1 and text in simt.last_error(), (text, rc, simt.last_error())

    assert simt.raw(None, None, (0, 0, 0), 9, 0.0, -1, -1, -1, -1, [None] * 11) == 0  # B == 0 before anything else
    err("bad B", dims=(-1, 3, 4))
    err("bad shape", dims=(2, 0, 4)); err("bad shape", dims=(2, 3, 65536))
    for mode in (2, 3, 4, 5, 6, -1):
        err("bad mode", mode=mode)
    err("sign must be", sign=0.5)
    err("bad k_start", k_start=-1); err("bad k_start", k_start=2 ** 30 + 1)
    err("bad n_iter", n_iter=-1); err("bad n_iter", n_iter=100001)
    err("bad power_iter", power_iter=-1); err("bad power_iter", power_iter=65)
    err("bad nnz_cap", cap=0); err("bad nnz_cap", cap=13)
    err("exceeds 160 KiB", dims=(2, 235, 190), cap=235 * 190)
    err("null or misaligned pred", pred=None)
    err("null or misaligned ctrs", cones=None)
    err("go together", ptrs=[out[0], None, out[2]] + [None] * 8)
    err("continuation", k_start=3, ptrs=[None] * 11)
    err("batch too large", dims=(2 ** 31, 3, 4))  # (refused before anything is read or launched)
    mis = np.zeros(25)[1:].view(np.uint8)[4:-4].view(np.float64)  # 4 bytes off
    if mis.ctypes.data % 8:
        err("misaligned x_curr", ptrs=[mis, out[1], out[2]] + [None] * 8)
        err("misaligned pgrad", ptrs=[None] * 10 + [mis])
    assert simt.raw(None, y, None, 1, 1.0, 0, 5, 8, 12, [None] * 11) == -1 and "cones is null" in simt.last_error()
    from cave_amd._lib import SparseConesC

    err("null or misaligned ent_off", cones=SparseConesC(B=2, m_max=3, d=4, ent_off=0, key=8, val=8), dims=None)
    assert simt.raw(A, y, (2, 3, 4), 1, 1.0, 0, 0, 0, 12, [None] * 11) == 0  # every output may be null


def test_batch_independence(simt):
    A, y, sign = AC.fixture_inputs()["tsp10"]
    rc, o = simt.run(A[:6], y[:6], sign=sign, n_iter=30, cap=AC.max_nnz(A), seed=1)
    perm = [4, 0, 5]
    rc, p = simt.run(A[perm], y[perm], sign=sign, n_iter=30, cap=AC.max_nnz(A), seed=2)
    AC.same_bits(o, p, rows=(perm, [0, 1, 2]))
    rc, one = simt.run(A[3:4], y[3:4], sign=sign, n_iter=30, cap=AC.max_nnz(A), seed=3)
    AC.same_bits(o, one, rows=([3], [0]))
    # another m_max for the same rows changes the step size only through 1/sqrt(m_max) at power_iter = 0 and the clamp;
    # another capacity changes nothing
    rc, c2 = simt.run(A[3:4], y[3:4], sign=sign, n_iter=30, cap=AC.max_nnz(A) + 100, seed=3)
    AC.same_bits(one, c2)


@pytest.mark.parametrize("name,split", [("sp5", (1, 199)), ("sp5", (200, 200)), ("tsp10", (1, 199))])
def test_continuation(simt, name, split):
    A, y, sign = AC.fixture_inputs()[name]
    A, y = A[:3], y[:3]
    cap = AC.max_nnz(A)
    rc, whole = simt.run(A, y, sign=sign, n_iter=sum(split), cap=cap, seed=1)
    rc, a = simt.run(A, y, sign=sign, n_iter=split[0], cap=cap, seed=2)
    rc, b = simt.run(A, y, sign=sign, n_iter=split[1], k_start=split[0], cap=cap, state=(a["x_curr"], a["x_prev"], a["step"]), seed=3)
    assert rc == 0
    AC.same_bits(whole, b, AC.FLOAT_OUT + AC.STATE_OUT + ("status",))
    assert (b["iters"] == split[1]).all()


def test_no_state_given_single_launch(simt):
    A, y, sign = AC.shape_cases()["m63_d2"]
    rc, o = simt.run(A, y, sign=sign, n_iter=7, seed=1)
    rc2, n = simt.run(A, y, sign=sign, n_iter=7, seed=1, want_state=False)
    assert rc == 0 and rc2 == 0
    AC.same_bits(o, n, AC.FLOAT_OUT + ("pgrad", "status", "iters"))


def test_under_the_sanitizers(tmp_path):
    """the stand-alone program (AddressSanitizer + UBSan, exact-size heap blocks) on a selection: both workgroup sizes,
    both loaders, the failure paths"""
    sc = AC.shape_cases()
    rng = np.random.default_rng(1)
    cases, want = [], []
    for name, waves in (("m65_d70", 1), ("m257_d1", 4), ("empty_padding_nocol", 0), ("dense_row_units", 4), ("m1_d1", 1)):
        A, y, sign = sc[name]
        for cones in (A, AC.to_sparse(A)):
            cases.append(dict(cones=cones, pred=y, sign=sign, n_iter=6, waves=waves, cap=AC.max_nnz(A)))
            want.append(name)
    A, y, sign = sc["empty_padding_nocol"]
    cases.append(dict(cones=A, pred=y, sign=sign, n_iter=3, cap=AC.max_nnz(A) - 1))  # one over: TOO_LARGE
    m, d, off, key, val = AC.to_sparse(A)
    k2 = key.copy(); k2[0] = 0xffffffff
    cases.append(dict(cones=(m, d, off, k2, val), pred=y, sign=sign, n_iter=3))       # a bad key
    res = E.run_asan(cases, str(tmp_path))
    lib = E.SimtApgd()
    for (rc, o), k, name in zip(res, cases, want):
        assert rc == 0
        rc2, ref = lib.run(k["cones"], k["pred"], sign=k["sign"], n_iter=6, cap=k["cap"], seed=0)
        AC.same_bits(o, ref, AC.FLOAT_OUT + AC.STATE_OUT + ("status", "iters"))
    assert (res[-2][1]["status"] == AC.ST_TOO_LARGE).any() and res[-1][1]["status"][0] == AC.ST_BAD_INPUT


def _doc_stub():
    """INTEGRATION.md §17 is tested text: its stub continues the first stub of §1"""
    import os
    import re

    from cave_amd import _lib

    _lib.load_library()  # (ImportError if the library has not been built; nothing is compiled from a test here)
    os.environ["CAVE_HIP_LIB"] = _lib.LIB_PATH
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    first = re.findall(r"^```python\n(.*?)^```", text[text.index("## 1. "):text.index("## 2. ")], flags=re.S | re.M)[0]
    sec = text[text.index("## 17. "):]
    stub = re.findall(r"^```python3\n(.*?)^```", sec, flags=re.S | re.M)
    assert len(stub) == 1
    ns = {}
    for b in (first, stub[0]):
        exec(compile(b, "INTEGRATION.md", "exec"), ns)  # noqa: S102 - the document is the test subject
    return ns, stub[0], sec, root


def test_integration_doc_stub_matches_header_prototypes():
    import re

    from test_integration_doc import _header_param_counts

    ns, src, sec, root = _doc_stub()
    counts = _header_param_counts()
    assert counts["cave_hip_cone_apgd"] == 23 and counts["cave_hip_cone_apgd_sparse"] == 20 and counts["cave_hip_apgd_lds_bytes"] == 3
    lib = ns["_lib"]
    for name in ("cave_hip_cone_apgd", "cave_hip_apgd_lds_bytes"):
        assert len(getattr(lib, name).argtypes) == counts[name], name
    src = re.sub(r"#[^\n]*", "", src)
    for name in ("cave_hip_cone_apgd", "cave_hip_apgd_lds_bytes"):
        calls = list(re.finditer(rf"_lib\.{name}\(", src))
        assert calls, name
        for m in calls:
            depth, i, args = 1, m.end(), 1
            while depth:
                ch = src[i]
                depth += ch in "(["
                depth -= ch in ")]"
                args += (ch == "," and depth == 1)
                i += 1
            assert args == counts[name], (name, args, counts[name])
    # the C block repeats the header's prototypes
    hdr = re.sub(r"/\*.*?\*/", "", open(f"{root}/include/cave_hip.h").read(), flags=re.S)
    squash = lambda s: re.sub(r"\s+", " ", s).strip()
    protos = re.findall(r"int32_t cave_hip_\w+\([^;]*\);", re.search(r"^```c\n(.*?)^```", sec, flags=re.S | re.M).group(1))
    assert len(protos) == 3
    for p in protos:
        assert squash(p) in squash(hdr), p
