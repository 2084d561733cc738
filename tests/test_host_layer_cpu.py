"""CPU tier: what the Python host layer hands to the C ABI, pinned without a device.

Layout: the arrays behind `struct cave_cone_store` (the slot form of qpsolver._SlotStore and the exact-fit form of
ConeStore._allocate) and `struct cave_lite_store` (qpsolver._LiteSlots) have the element widths of include/cave_hip.h and
the extents its comments document, and the struct fields point at them.

Dispatch: `_launch_step` / `_launch_step_sparse`, called through a recording stand-in for the library, pick the entry point
and build the argument list written down in EXPECTED below -- recorded from the code as it stood before the two
launchers became one, so a change of the host layer that moves an argument shows here.
"""

import ctypes as C
import os
import re

import pytest
import torch

from cave_amd import _lib
from cave_amd import qpsolver as Q
from cave_amd.dataset import ConeStore
from cave_amd.sparse import SparseCones
from cave_amd.warm import WarmCache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
WIDTH = {"int64_t": 8, "int32_t": 4, "uint32_t": 4, "float": 4, "uint16_t": 2, "uint8_t": 1}


def _header_pointers(struct):
    """pointer fields of a struct block of the header -> width of the pointee in bytes"""
    hdr = open(os.path.join(ROOT, "include", "cave_hip.h")).read()
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = {}
    for decl in body.split(";"):
        m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*\*\s*(\w+)\s*", decl)
        if m:
            out[m.group(2)] = WIDTH[m.group(1)]
    return out


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load_library()  # (_SlotStore asks it for an LDS figure; no device is touched)


def _check_arrays(t, c, widths, extents):
    """every array in `t`: the header's element width, the documented extent, and the struct field is its address"""
    assert set(t) == set(extents)
    for name, n in extents.items():
        assert t[name].element_size() == widths[name], name
        assert t[name].numel() == n, (name, t[name].numel(), n)
        assert t[name].is_contiguous() and getattr(c, name) == t[name].data_ptr(), name
    assert (c.reserved, c.n, c.d) == (0, extents["usign"] // c.d, c.d)


def _store_extents(n, d, R, Z, slot):
    e = {"row_off": n + 1, "nnz_off": n + 1, "n_valid": n, "flags": n, "usign": n * d, "avg": n * d,
         "vkind": max(R, 1), "rlo": max(R, 1), "rhi": max(R, 1), "ccol": max(Z, 1), "cval": max(Z, 1),
         "cptr": n * (d + 1), "cvar": max(Z, 1), "cvalc": max(Z, 1)}
    if slot:
        e["n_rows"] = e["n_nnz"] = n
    return e


def test_slot_store_layout(lib):
    widths = _header_pointers("cave_cone_store")
    assert len(widths) == 19
    B, d = 3, 5
    ss = Q._SlotStore(CPU, B, d)
    _check_arrays(ss.t, ss.c, widths, _store_extents(B, d, B * Q.SPLIT_ROWS, B * Q.SPLIT_NNZ, slot=True))
    assert (Q.SPLIT_ROWS, Q.SPLIT_NNZ) == (32, 1536)
    assert ss.t["row_off"].tolist() == [0, 32, 64, 96] and ss.t["nnz_off"].tolist() == [0, 1536, 3072, 4608]
    assert ss.c.n_rows is not None and ss.c.n_nnz is not None
    assert ss.c.warm_theta is None and ss.c.warm_state is None and ss.c.rb_cache is None and ss.c.rb_stride == 0
    assert (ss.B, ss.d, ss.gen) == (B, d, 0)
    assert ss.pack_status.shape == (B,) and ss.pack_status.dtype == torch.int32
    assert ss.lds_bytes == int(lib.cave_hip_packed_lds_bytes(d, 32, 1536, 1))
    assert C.cast(ss.ref, C.POINTER(_lib.Store)).contents.n == B  # `ref` is byref(c)
    assert all(bool((v == 0).all()) for k, v in ss.t.items() if k not in ("row_off", "nnz_off"))


def test_lite_slots_layout():
    widths = _header_pointers("cave_lite_store")
    assert len(widths) == 7
    B, d = 3, 5
    ls = Q._LiteSlots(CPU, B, d)
    _check_arrays(ls.t, ls.c, widths, {"hdr": B * 8, "usign": B * d, "avg": B * d, "rowptr": B * 33, "ell": B * 4 * d,
                                       "csr16": B * 768, "rl": B * 32})
    assert (ls.B, ls.d, ls.gen) == (B, d, 0)
    assert ls.pack_status.shape == (B,) and ls.pack_status.dtype == torch.int32
    assert all(bool((v == 0).all()) for v in ls.t.values())


@pytest.mark.parametrize("rows,nnz", [([2, 0, 3], [4, 0, 7]), ([0, 0], [0, 0])], ids=["empty-in-the-middle", "all-empty"])
def test_exact_fit_store_layout(rows, nnz):
    widths = _header_pointers("cave_cone_store")
    d, n = 5, len(rows)
    st = ConeStore(d, CPU)
    # the count pass hands over one (n_rows, n_nnz) pair per chunk: here two chunks
    counts = [(torch.tensor(rows[:1], dtype=torch.int32), torch.tensor(nnz[:1], dtype=torch.int32)),
              (torch.tensor(rows[1:], dtype=torch.int32), torch.tensor(nnz[1:], dtype=torch.int32))]
    st._allocate(counts)
    R, Z = sum(rows), sum(nnz)
    _check_arrays(st.t, st._c, widths, _store_extents(n, d, R, Z, slot=False))
    off = lambda v: [sum(v[:i]) for i in range(len(v) + 1)]
    assert st.t["row_off"].tolist() == off(rows) and st.t["nnz_off"].tolist() == off(nnz)
    assert st._c.n_rows is None and st._c.n_nnz is None      # NULL: what makes the store exact-fit for the kernels
    assert st._c.warm_theta is None and st._c.warm_state is None and st._c.rb_cache is None and st._c.rb_stride == 0
    assert (st.n, st.max_rows, st.max_nnz) == (n, max(rows), max(nnz))
    assert all(bool((v == 0).all()) for k, v in st.t.items() if k not in ("row_off", "nnz_off"))


# ------------------------------------------------------------------ step dispatch through a fake library
class _Recorder:
    """stands in for the loaded library: every entry point records its arguments and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


D, M = 6, 4
PROJECT, IPM = _lib.MODE_PROJECT, _lib.MODE_INNER_IPM


def _run_case(monkeypatch, kind, B, mode, with_warm):
    """-> (entry point, [label or scalar per argument], out) of one launch.  Pointers are named after what they point
    at ("NULL" for a null pointer however it is spelled: None or a zero c_void_p)."""
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda: rec)
    monkeypatch.setattr(_lib, "current_stream", lambda: C.c_void_p(0x5700))
    monkeypatch.setattr(SparseCones, "is_cuda", property(lambda self: True))  # (c_struct refuses a host batch)
    solve, nstore = Q._LiteSlots(CPU, max(B, 1), D), Q._LiteSlots(CPU, 3, D)
    pred = torch.zeros(max(B, 1), D)
    out = {"loss": torch.zeros(max(B, 1)), "grad": torch.zeros(max(B, 1), D)}
    status, iters = torch.zeros(max(B, 1), dtype=torch.int32), torch.zeros(max(B, 1), dtype=torch.int32)
    ids = torch.arange(max(B, 1), dtype=torch.int64)
    keys = ids.clone()
    warm = WarmCache(8, CPU) if with_warm else None
    named = {pred.data_ptr(): "pred", out["loss"].data_ptr(): "loss", out["grad"].data_ptr(): "grad",
             status.data_ptr(): "status", iters.data_ptr(): "iters", ids.data_ptr(): "ids", keys.data_ptr(): "keys",
             nstore.pack_status.data_ptr(): "next_pack_status", Q._tickets_for(CPU).data_ptr(): "tickets", 0x5700: "stream"}
    refs = {id(solve.c): "solve", id(nstore.c): "next_store"}
    if warm is not None:
        refs[id(warm.c)] = "warm"
    if kind == "sparse":
        nxt = SparseCones.from_coo([([0, 1], [0, 2], [1.0, -1.0]), ([0], [5], [1.0]), ([], [], [])], D, m_max=M)
        Q._launch_step_sparse(solve, pred, B, mode, -1.0, 0.25, 7, out, status, iters, nxt, nstore,
                              zero_failed=True, warm=warm, keys=keys)
        refs[id(nxt._c)] = "next_cones"
        assert (nxt._c.B, nxt._c.m_max, nxt._c.d) == (3, M, D)
    else:
        nxt = torch.zeros(3, M, D) if kind == "dense" else None
        if nxt is not None:
            named[nxt.data_ptr()] = "next_ctrs"
        Q._launch_step(solve, pred, B, mode, -1.0, 0.25, 7, out, status, iters, nxt, nstore if nxt is not None else None,
                       ids=ids, zero_failed=True, warm=warm, keys=keys)
    assert len(rec.calls) == 1
    name, args = rec.calls[0]
    if "warm_hit" in out:
        named[out["warm_hit"].data_ptr()] = "warm_hit"
    desc = []
    for a in args:
        if a is None or (isinstance(a, C.c_void_p) and not a.value):
            desc.append("NULL")
        elif isinstance(a, C.c_void_p):
            desc.append(named[a.value])
        elif isinstance(a, (int, float)):
            desc.append(a)
        else:
            desc.append(refs[id(a._obj)])  # a byref(...)
    return name, desc, out


OUT7 = ["NULL", "NULL", "NULL", "loss", "grad", "status", "iters"]           # proj, rnorm, target, loss, grad, status, iters
PACK_DENSE = ["next_ctrs", 3, M, D, "next_store", "next_pack_status"]
PACK_NONE = ["NULL", 0, 0, D, "NULL", "NULL"]
PACK_SPARSE = ["next_cones", "next_store", "next_pack_status"]
END = ["tickets", "stream"]


def _head(B, mode=None):
    h = ["solve", "ids", "pred", B]
    return h + ([mode, -1.0, 0.25, 7, 1] if mode is not None else [-1.0, 7, 1]) + OUT7


def _head_sparse(B, mode=None):
    h = _head(B, mode)
    h[1] = "NULL"  # the sparse launcher has no `ids`
    return h


# (kind, B, mode, warm cache given) -> entry point, argument list, whether out["warm_hit"] exists
# (an empty tensor has no storage: the [0] warm_hit of a dense pack-only launch goes over as a null pointer)
EXPECTED = {
    ("dense", 0, PROJECT, False): ("cave_hip_cone_step", _head(0, PROJECT) + PACK_DENSE + END, False),
    ("dense", 2, PROJECT, False): ("cave_hip_cone_step", _head(2, PROJECT) + PACK_DENSE + END, False),
    ("dense", 0, PROJECT, True): ("cave_hip_cone_step_warm", _head(0, PROJECT) + PACK_DENSE + ["warm", "keys", "NULL"] + END, True),
    ("dense", 2, PROJECT, True): ("cave_hip_cone_step_warm", _head(2, PROJECT) + PACK_DENSE + ["warm", "keys", "warm_hit"] + END, True),
    ("dense", 0, IPM, False): ("cave_hip_cone_step", _head(0, IPM) + PACK_DENSE + END, False),
    ("dense", 2, IPM, False): ("cave_hip_cone_step_ipm", _head(2) + PACK_DENSE + END, False),
    ("dense", 0, IPM, True): ("cave_hip_cone_step_warm", _head(0, IPM) + PACK_DENSE + ["warm", "keys", "NULL"] + END, True),
    ("dense", 2, IPM, True): ("cave_hip_cone_step_ipm", _head(2) + PACK_DENSE + END, False),
    ("none", 2, PROJECT, False): ("cave_hip_cone_step", _head(2, PROJECT) + PACK_NONE + END, False),
    ("none", 2, PROJECT, True): ("cave_hip_cone_step_warm", _head(2, PROJECT) + PACK_NONE + ["warm", "keys", "warm_hit"] + END, True),
    ("none", 2, IPM, False): ("cave_hip_cone_step_ipm", _head(2) + PACK_NONE + END, False),
    ("none", 2, IPM, True): ("cave_hip_cone_step_ipm", _head(2) + PACK_NONE + END, False),
    ("sparse", 0, PROJECT, False): ("cave_hip_cone_step_sparse", _head_sparse(0, PROJECT) + PACK_SPARSE + ["NULL", "keys", "NULL"] + END, False),
    ("sparse", 2, PROJECT, False): ("cave_hip_cone_step_sparse", _head_sparse(2, PROJECT) + PACK_SPARSE + ["NULL", "keys", "NULL"] + END, False),
    ("sparse", 0, PROJECT, True): ("cave_hip_cone_step_sparse", _head_sparse(0, PROJECT) + PACK_SPARSE + ["NULL", "keys", "NULL"] + END, False),
    ("sparse", 2, PROJECT, True): ("cave_hip_cone_step_sparse", _head_sparse(2, PROJECT) + PACK_SPARSE + ["warm", "keys", "warm_hit"] + END, True),
    ("sparse", 0, IPM, False): ("cave_hip_cone_step_sparse", _head_sparse(0, IPM) + PACK_SPARSE + ["NULL", "keys", "NULL"] + END, False),
    ("sparse", 2, IPM, False): ("cave_hip_cone_step_sparse_ipm", _head_sparse(2) + PACK_SPARSE + END, False),
    ("sparse", 0, IPM, True): ("cave_hip_cone_step_sparse", _head_sparse(0, IPM) + PACK_SPARSE + ["NULL", "keys", "NULL"] + END, False),
    ("sparse", 2, IPM, True): ("cave_hip_cone_step_sparse_ipm", _head_sparse(2) + PACK_SPARSE + END, False),
}
ARGC = {"cave_hip_cone_step": 24, "cave_hip_cone_step_warm": 27, "cave_hip_cone_step_ipm": 22,
        "cave_hip_cone_step_sparse": 24, "cave_hip_cone_step_sparse_ipm": 19}


@pytest.mark.parametrize("case", sorted(EXPECTED), ids=lambda c: f"{c[0]}-B{c[1]}-mode{c[2]}-{'warm' if c[3] else 'cold'}")
def test_step_dispatch(monkeypatch, case):
    kind, B, mode, with_warm = case
    name, desc, out = _run_case(monkeypatch, kind, B, mode, with_warm)
    want_name, want_args, want_hit = EXPECTED[case]
    assert name == want_name
    assert len(desc) == ARGC[name]
    assert desc == want_args
    assert ("warm_hit" in out) == want_hit
    if want_hit:
        assert out["warm_hit"].shape == (B,) and out["warm_hit"].dtype == torch.uint8
    assert set(out) - {"warm_hit"} == {"loss", "grad"}


def test_recorded_argument_counts_are_the_bound_ones(lib):
    for name, n in ARGC.items():
        assert len(getattr(lib, name).argtypes) == n
