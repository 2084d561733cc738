"""CPU tier of the sparse wire format (cave_amd/sparse.py, cone_instance.h load_sparse_and_build).

The correctness argument of the sparse route is "same build_cone, same input, different producer": the store the
sparse count + fill writes must be BIT-identical, array by array, to the one the dense scan writes for the densified
batch.  Here on the serial emulation of the kernels' per-instance code (tests/emul/emul_sparse.cpp beside
emul_abi.cpp); on the device in tests/test_gpu_sparse.py.
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cave_amd import _lib, synth
from cave_amd.sparse import SparseCones, collate_sparse
from emul_lib import Emul
from emul_sparse_lib import EmulSparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_TOO_LARGE, ST_BAD_INPUT = 0, 2, 3


@pytest.fixture(scope="module")
def emul():
    return Emul()


@pytest.fixture(scope="module")
def semul():
    return EmulSparse()


def _same(a: SparseCones, b: SparseCones) -> bool:
    return (a.B, a.m_max, a.d) == (b.B, b.m_max, b.d) and torch.equal(a.ent_off, b.ent_off) and \
        torch.equal(a.key, b.key) and torch.equal(a.val, b.val)


def _host(sc: SparseCones):
    return sc.ent_off.numpy(), sc.key.numpy().view(np.uint32), sc.val.numpy()


# ------------------------------------------------------------------ 1. canonicalisation
@pytest.mark.parametrize("kind,size,d", [("tsp", 20, 190), ("sp", (5, 5), 40), ("tsp", 50, 1225)])
def test_constructors_agree(kind, size, d):
    items, _, _ = synth.coo_batch(kind, size, 4, seed=0)
    r, c = items[0][0], items[0][1]
    assert not bool(np.all(np.diff((r << 16) | c) > 0))  # coo_batch entries are NOT sorted: from_coo has to
    a = SparseCones.from_coo(items, d)
    dense = synth.densify_on(items, d, "cpu")
    b = SparseCones.from_dense(dense)
    ragged = [dense[i, :items[i][3]] for i in range(len(items))]
    c3 = SparseCones.from_ragged(ragged)
    c4 = SparseCones.from_ragged([x.numpy() for x in ragged])
    assert _same(a, b) and _same(a, c3) and _same(a, c4)
    assert a.m_max == max(it[3] for it in items) and len(a) == 4
    assert int(a.nnz_per_instance.sum()) == a.nnz == sum(len(it[0]) for it in items)
    assert a.nbytes == 8 * a.nnz + 8 * 5
    k = a.key.numpy().view(np.uint32).astype(np.int64)
    off = a.ent_off.numpy()
    for i in range(4):
        assert np.all(np.diff(k[off[i]:off[i + 1]]) > 0)
    assert torch.equal(a.densify(), dense)


def test_scipy_sparse_input():
    sp = pytest.importorskip("scipy.sparse")
    ctrs, _, _ = synth.sp_batch(5, 5, 3, seed=2)
    a = SparseCones.from_ragged([sp.csr_matrix(x) for x in ctrs])
    assert _same(a, SparseCones.from_dense(ctrs))


def test_densify_round_trips_dense_batches():
    for ctrs in (synth.tsp_batch(20, 5, seed=3)[0], synth.sp_batch(5, 5, 5, seed=3)[0], synth.generic_batch(6)[0]):
        sc = SparseCones.from_dense(ctrs)
        assert np.array_equal(sc.densify().numpy(), ctrs)
        assert _same(SparseCones.from_dense(sc.densify()), sc)


def test_duplicates_raise_and_zeros_vanish():
    with pytest.raises(ValueError, match="more than once"):
        SparseCones.from_coo([([0, 1, 0], [2, 3, 2], [1.0, 1.0, 2.0], 2)], d=4)
    with pytest.raises(ValueError, match="outside"):
        SparseCones.from_coo([([0, 2], [2, 3], [1.0, 1.0], 2)], d=4)
    with pytest.raises(ValueError, match="outside"):
        SparseCones.from_coo([([0], [4], [1.0], 2)], d=4)
    a = SparseCones.from_coo([([1, 0, 0], [3, 2, 1], [1.0, 0.0, -2.0], 2), ([], [], [], 3)], d=4)
    assert a.ent_off.tolist() == [0, 2, 2] and a.key.tolist() == [1, (1 << 16) | 3] and a.val.tolist() == [-2.0, 1.0]
    assert a.m_max == 3
    # non-finite values are left for the device to reject
    b = SparseCones.from_coo([([0], [1], [float("nan")], 1)], d=4)
    assert b.nnz == 1 and bool(torch.isnan(b.val[0]))
    # rows beyond 65535 do not fit the key
    with pytest.raises(ValueError):
        SparseCones.from_coo([([70000], [0], [1.0])], d=4)


def test_slicing_and_collate_reproduce_the_batch():
    items, _, _ = synth.coo_batch("tsp", 20, 7, seed=1)
    a = SparseCones.from_coo(items, 190)
    pieces = [a[i] for i in range(len(a))]
    assert all(len(p) == 1 for p in pieces)
    fields = [(torch.full((3,), float(i)), torch.zeros(2), torch.ones(1), torch.zeros(1), p) for i, p in enumerate(pieces)]
    x, c, w, z, cones = collate_sparse(fields)
    assert x.shape == (7, 3) and _same(cones, a)
    assert _same(SparseCones.cat([a[0:3], a[3:7]]), a)
    assert _same(a[2:5], SparseCones.from_coo(items[2:5], 190, m_max=a.m_max))
    assert _same(a[[5, 0, 5]], SparseCones.from_coo([items[5], items[0], items[5]], 190, m_max=a.m_max))
    assert _same(a[torch.tensor([6, 1])], SparseCones.from_coo([items[6], items[1]], 190, m_max=a.m_max))
    assert _same(a[::3], a[[0, 3, 6]])
    assert len(a[4:4]) == 0 and a[4:4].nnz == 0
    with pytest.raises(IndexError):
        a[[7]]


# ------------------------------------------------------------------ 2. bit-identical stores (serial emulation)
def _assert_same_store(dense_arrs, sparse_arrs, what):
    assert set(dense_arrs) == set(sparse_arrs)
    for k in dense_arrs:
        x, y = dense_arrs[k], sparse_arrs[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)


def _with_edge_instances(ctrs):
    """+ an instance without entries and one whose only general row sums below the drop threshold (src/cave.py:303)."""
    B, m, d = ctrs.shape
    extra = np.zeros((2, m, d), np.float32)
    extra[1, 0, 0] = 1.0
    extra[1, 1, 1] = 3e-8
    extra[1, 1, 2] = 4e-8
    return np.concatenate([ctrs[:B // 2], extra[:1], ctrs[B // 2:], extra[1:]])


def _lds_cases(golden):
    g, s = golden["generic"], golden["structured"]
    yield "generic", _with_edge_instances(g["generic_ctrs"]), {}
    yield "sp5", _with_edge_instances(s["sp5_ctrs"]), {}
    yield "tsp20", _with_edge_instances(s["tsp20_ctrs"]), {}
    # TSP-50: the second tier of the store builders (the full 160 KiB arena, cave_amd.qpsolver._grow_limits)
    yield "tsp50", synth.tsp_batch(50, 4, seed=0)[0], dict(nnz_cap=int(160 * 1024 * 0.55) // 8 - 256, lds_bytes=160 * 1024)


def test_serial_store_bits_equal_dense_route(emul, semul, golden):
    for what, ctrs, lim in _lds_cases(golden):
        assert np.abs(ctrs).max() > 0 and (what != "generic" or not np.all(np.abs(ctrs[ctrs != 0]) == 1.0))
        _, darrs, mr, mz = emul.pack(ctrs, **lim)
        sc = SparseCones.from_dense(ctrs)
        sarrs, n_rows, n_nnz, st1, st2 = semul.pack(*_host(sc), sc.m_max, sc.d, **lim)
        assert (st1 == ST_OK).all() and (st2 == ST_OK).all(), what
        assert int(n_rows.max()) == mr and int(n_nnz.max()) == mz, what
        _assert_same_store(darrs, sarrs, what)


@pytest.mark.parametrize("what", ["sp12", "tsp100"])
def test_serial_store_bits_equal_dense_route_large(emul, semul, what):
    ctrs = synth.sp_batch(12, 12, 2, seed=0)[0] if what == "sp12" else synth.tsp_batch(100, 2, seed=0)[0]
    B, m, d = ctrs.shape
    _, darrs, mr, mz = emul.pack_large(ctrs)
    sc = SparseCones.from_dense(ctrs)
    cap = max(64, int(sc.nnz_per_instance.max()))   # what Emul.pack_large derives from the dense form
    slice_bytes = emul.large_slice_bytes(m, d, cap, 1)
    sarrs, n_rows, n_nnz, st1, st2 = semul.pack_large(*_host(sc), m, d, cap, slice_bytes)
    assert (st1 == ST_OK).all() and (st2 == ST_OK).all()
    assert int(n_rows.max()) == mr and int(n_nnz.max()) == mz
    _assert_same_store(darrs, sarrs, what)


def test_serial_capacity_is_a_status_not_an_overrun(semul, golden):
    sc = SparseCones.from_dense(golden["structured"]["tsp20_ctrs"][:3])
    _, n_rows, n_nnz, st1, st2 = semul.pack(*_host(sc), sc.m_max, sc.d, nnz_cap=int(sc.nnz_per_instance.max()) - 1, lds_bytes=64 * 1024)
    assert ST_TOO_LARGE in st1 and ((st1 == ST_OK) | (st1 == ST_TOO_LARGE)).all()
    assert np.all(n_rows[st1 == ST_TOO_LARGE] == 0)


# ------------------------------------------------------------------ 3. malformed input (serial emulation)
def malformed_batch(ctrs):
    """(ent_off, key, val, bad indices): the cones of `ctrs` with instances 1, 3, 5, 7, 9, 11 broken, one way each:
    swapped pair, repeated key, row = m_max, col = d, zero value, NaN.  Shared with the device tests."""
    sc = SparseCones.from_dense(ctrs)
    assert len(sc) >= 13
    off, key, val = (x.copy() for x in _host(sc))
    m, d = sc.m_max, sc.d

    def at(i, j=3):
        assert off[i + 1] - off[i] > j + 2
        return off[i] + j

    e = at(1); key[e], key[e + 1] = key[e + 1], key[e]; val[e], val[e + 1] = val[e + 1], val[e]
    e = at(3); key[e + 1] = key[e]
    e = off[6] - 1; key[e] = (m << 16) | (key[e] & 0xffff)          # last entry of instance 5: order stays valid
    e = at(7); key[e] = (key[e] & 0xffff0000) | d
    # (col = d only keeps the order if the next key is in a later row; either way the instance is bad)
    e = at(9); val[e] = 0.0
    e = at(11); val[e] = np.nan
    return off, key, val, [1, 3, 5, 7, 9, 11]


def _check_malformed(packer, ctrs, lim):
    off, key, val, bad = malformed_batch(ctrs)
    B, m, d = ctrs.shape
    good = [i for i in range(B) if i not in bad]
    arrs, n_rows, n_nnz, st1, st2 = packer(off, key, val, m, d, **lim)
    for st in (st1, st2):
        assert np.all(st[bad] == ST_BAD_INPUT) and np.all(st[good] == ST_OK), st
    assert np.all(n_rows[bad] == 0) and np.all(n_nnz[bad] == 0)
    # the neighbours: exactly the store of the good cones alone
    sub = SparseCones.from_dense(ctrs[good])
    ref, _, _, s1, s2 = packer(*_host(sub), m, d, **lim)
    assert (s1 == ST_OK).all() and (s2 == ST_OK).all()
    for k in ("vkind", "rlo", "rhi", "ccol", "cval", "cvar", "cvalc"):
        assert arrs[k].tobytes() == ref[k].tobytes(), k
    for k, w in (("usign", d), ("avg", d), ("cptr", d + 1), ("n_valid", 1), ("flags", 1)):
        assert np.array_equal(arrs[k].reshape(B, w)[good], ref[k].reshape(len(good), w)), k
        assert not arrs[k].reshape(B, w)[bad].any(), k   # a rejected instance writes nothing


def test_serial_malformed_instances_are_rejected_alone(semul, golden):
    ctrs = np.concatenate([golden["structured"]["tsp20_ctrs"], golden["structured"]["tsp20_ctrs"]])[:14]
    _check_malformed(semul.pack, ctrs, {})
    cap = 2000
    sl = Emul().large_slice_bytes(ctrs.shape[1], ctrs.shape[2], cap, 1)
    _check_malformed(lambda *a, **k: semul.pack_large(*a, nnz_cap=cap, slice_bytes=sl), ctrs, {})


def test_serial_misaligned_arrays_take_the_same_answer(semul, golden):
    """key / val that start off a 16-byte boundary (congruent, then not congruent): head, groups of four and tail of the
    loader against the aligned run."""
    sc = SparseCones.from_dense(golden["structured"]["tsp20_ctrs"][:4])
    off, key, val = _host(sc)
    ref = semul.pack(off, key, val, sc.m_max, sc.d)[0]
    for sk, sv in ((1, 1), (3, 3), (1, 2)):
        kb = np.zeros(key.size + 8, np.uint32); vb = np.zeros(val.size + 8, np.float32)
        kb[sk:sk + key.size] = key; vb[sv:sv + val.size] = val
        s, keep = semul._batch(off, key, val, sc.m_max, sc.d)
        s.key, s.val = kb.ctypes.data + 4 * sk, vb.ctypes.data + 4 * sv
        import ctypes as C
        from emul_lib import _p
        from emul_sparse_lib import empty_store
        n_rows = np.zeros(4, np.int32); n_nnz = np.zeros(4, np.int32); st = np.zeros(4, np.int32)
        assert semul.lib.cave_emul_pack_count_sparse(C.byref(s), 0, 0, _p(n_rows), _p(n_nnz), _p(st)) == 0 and not st.any()
        store, arrs = empty_store(n_rows, n_nnz, sc.d)
        assert semul.lib.cave_emul_pack_fill_sparse(C.byref(s), 0, 0, C.byref(store), C.c_int64(0), _p(st)) == 0 and not st.any()
        _assert_same_store(ref, arrs, (sk, sv))


def test_sparse_asan_ubsan_clean():
    """The malformed batch and the capacity case under AddressSanitizer / UBSan (host sanitizers on the serial build)."""
    import emul_sparse_lib

    so = emul_sparse_lib.build(asan=True)
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    code = (
        "import sys; sys.path[:0]=[%r,%r]\n"
        "import numpy as np, ctypes as C, emul_sparse_lib, emul_lib\n"
        "import test_sparse_cpu as T\n"
        "from cave_amd import synth\n"
        "from cave_amd.sparse import SparseCones\n"
        "E = emul_sparse_lib.EmulSparse.__new__(emul_sparse_lib.EmulSparse); E.lib = C.CDLL(%r)\n"
        "g = np.load(%r)\n"
        "ctrs = np.concatenate([g['tsp20_ctrs'], g['tsp20_ctrs']])[:14]\n"
        "T._check_malformed(E.pack, ctrs, {})\n"
        "sl = emul_lib.Emul().large_slice_bytes(ctrs.shape[1], ctrs.shape[2], 2000, 1)\n"
        "T._check_malformed(lambda *a, **k: E.pack_large(*a, nnz_cap=2000, slice_bytes=sl), ctrs, {})\n"
        "sc = SparseCones.from_dense(ctrs[:3])\n"
        "E.pack(*T._host(sc), sc.m_max, sc.d, nnz_cap=500, lds_bytes=64 * 1024)\n"   # over capacity: a status
        "E.pack(*T._host(sc), sc.m_max, sc.d, nnz_cap=4000, lds_bytes=8 * 1024)\n"   # arena too small: a status
        "c2 = synth.sp_batch(9, 9, 2, 1)[0]; s2 = SparseCones.from_dense(c2)\n"
        "E.pack_large(*T._host(s2), s2.m_max, s2.d, 2000, 20000)\n"                  # slice too small: a status
        "print('asan-ok')\n" % (ROOT, os.path.join(ROOT, "tests"), so, os.path.join(ROOT, "tests", "golden", "structured.npz")))
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "asan-ok" in r.stdout, r.stderr[-3000:]


# ------------------------------------------------------------------ 4. header / binding
def test_sparse_symbols_exported_and_bound():
    _lib.build()
    lib = _lib.load_library()
    import ctypes as C

    for name in ("cave_hip_pack_count_sparse", "cave_hip_pack_fill_sparse", "cave_hip_pack_large_sparse"):
        assert name in _lib.ABI_SYMBOLS and getattr(lib, name).argtypes and getattr(lib, name).restype is C.c_int32
    assert lib.cave_hip_version() == 10   # additive: no bump
    assert C.sizeof(_lib.SparseConesC) == 40
    # argument validation happens before any launch (no GPU here)
    s = _lib.SparseConesC(B=1, m_max=4, d=0, ent_off=None, key=None, val=None)
    assert lib.cave_hip_pack_count_sparse(C.byref(s), 0, 0, 0, None, None, None, None) == -1
    assert b"bad batch" in lib.cave_hip_last_error()
    s = _lib.SparseConesC(B=1, m_max=70000, d=4, ent_off=None, key=None, val=None)
    assert lib.cave_hip_pack_fill_sparse(C.byref(s), 0, 0, 0, None, 0, None, None) == -1
    s = _lib.SparseConesC(B=1, m_max=4, d=4, ent_off=None, key=None, val=None)
    assert lib.cave_hip_pack_large_sparse(C.byref(s), 64, None, 1 << 20, 4, None, None, None, 0, None, None) == -1
    assert b"null" in lib.cave_hip_last_error()
    s = _lib.SparseConesC(B=0, m_max=4, d=4, ent_off=None, key=None, val=None)
    assert lib.cave_hip_pack_count_sparse(C.byref(s), 0, 0, 0, None, None, None, None) == 0   # B == 0
    # no one-wave sparse pack shape
    buf = (C.c_int64 * 4)()
    s = _lib.SparseConesC(B=1, m_max=4, d=4, ent_off=C.addressof(buf), key=C.addressof(buf), val=C.addressof(buf))
    assert lib.cave_hip_pack_count_sparse(C.byref(s), 0, 0, 1, C.addressof(buf), C.addressof(buf), None, None) == -1
    assert b"waves" in lib.cave_hip_last_error()


def test_public_names():
    import cave_amd

    for name in ("SparseCones", "collate_sparse", "cone_op_sparse", "project_hip_sparse"):
        assert hasattr(cave_amd, name), name
    assert hasattr(cave_amd.ConeStore, "from_sparse") and hasattr(cave_amd.ConeStore, "from_sparse_shard")
