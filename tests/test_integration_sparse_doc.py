"""INTEGRATION.md §8 (the sparse wire format) is tested text, to the standard tests/test_integration_doc.py holds §1 and
§6 to: its fenced ctypes stub is executed verbatim, after the first stub of §1 it continues.

CPU tier: every `argtypes` list it declares has as many entries as the prototype in include/cave_hip.h has parameters,
the structs have the layout of the package's own binding, and the C block repeats the header's struct.
GPU tier: `cone_op_sparse_hip` as the document writes it, against the reference's own outputs."""

import ctypes
import os
import re

import numpy as np
import pytest

from test_integration_doc import _header_param_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sections():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    return text[text.index("## 1. "):text.index("## 2. ")], text[text.index("## 8. "):]


def _exec_doc():
    from cave_amd import _lib

    _lib.build()
    os.environ["CAVE_HIP_LIB"] = _lib.LIB_PATH
    sec1, sec8 = _sections()
    blocks = re.findall(r"^```python\n(.*?)^```", sec1, flags=re.S | re.M)[:1] + re.findall(r"^```python\n(.*?)^```", sec8, flags=re.S | re.M)
    assert len(blocks) == 2, "INTEGRATION.md §8 must hold one python stub"
    ns = {}
    for b in blocks:
        exec(compile(b, "INTEGRATION.md", "exec"), ns)  # noqa: S102 - the document is the test subject
    return ns, blocks[1]


def test_sparse_doc_stub_matches_header_and_binding():
    from cave_amd import _lib

    ns, src = _exec_doc()
    counts = _header_param_counts()
    assert counts["cave_hip_pack_fill_sparse"] == 8 and counts["cave_hip_pack_count_sparse"] == 8 and counts["cave_hip_pack_large_sparse"] == 11
    lib = ns["_lib"]
    for name in ("cave_hip_pack_fill_sparse", "cave_hip_packed_lds_bytes", "cave_hip_cone_packed"):
        assert len(getattr(lib, name).argtypes) == counts[name], name
    # the calls written in the document pass as many arguments as they declare
    src = re.sub(r"#[^\n]*", "", src)
    for name in ("cave_hip_pack_fill_sparse", "cave_hip_packed_lds_bytes", "cave_hip_cone_packed"):
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
    # struct layouts: the document's against the package's own binding
    for doc, pkg in ((ns["cave_sparse_cones"], _lib.SparseConesC), (ns["cave_cone_store"], _lib.Store)):
        assert ctypes.sizeof(doc) == ctypes.sizeof(pkg)
        assert [(n, getattr(doc, n).offset) for n, _ in doc._fields_] == [(n, getattr(pkg, n).offset) for n, _ in pkg._fields_]
    # the C block is the header's struct, member for member
    hdr = open(os.path.join(ROOT, "include", "cave_hip.h")).read()
    members = lambda s: re.findall(r"(?:const\s+)?\w+\s*\*?\s*(\w+(?:\s*,\s*\w+)*)\s*;", re.sub(r"/\*.*?\*/", "", s, flags=re.S))
    doc_c = re.search(r"typedef struct cave_sparse_cones \{(.*?)\} cave_sparse_cones;", _sections()[1], flags=re.S).group(1)
    hdr_c = re.search(r"typedef struct cave_sparse_cones \{(.*?)\} cave_sparse_cones;", hdr, flags=re.S).group(1)
    assert members(doc_c) == members(hdr_c) and len(members(hdr_c)) == 5


@pytest.mark.gpu
def test_sparse_doc_cone_op_matches_reference_outputs(golden):
    import torch

    from cave_amd.sparse import SparseCones

    ns, _ = _exec_doc()
    g = golden["structured"]
    for tag in ("tsp20", "sp5"):
        sc = SparseCones.from_dense(g[f"{tag}_ctrs"]).cuda()
        costs = torch.tensor(g[f"{tag}_costs"], device="cuda")
        loss, grad, status = ns["cone_op_sparse_hip"](sc.ent_off, sc.key, sc.val, sc.m_max, costs)
        torch.cuda.synchronize()
        assert bool((status == 0).all())
        assert np.abs(loss.cpu().numpy() - g[f"{tag}_min_inner_loss"]).max() <= 2e-6
        gs = max(1.0, float(np.abs(g[f"{tag}_min_inner_grad"]).max()))
        assert np.abs(grad.cpu().numpy() - g[f"{tag}_min_inner_grad"]).max() <= 8e-6 * gs
    # a broken entry is that instance's status, nothing else
    val = sc.val.clone()
    val[int(sc.ent_off[1]) + 2] = 0.0
    loss2, grad2, status = ns["cone_op_sparse_hip"](sc.ent_off, sc.key, val, sc.m_max, costs)
    assert status.tolist() == [0, 3] + [0] * (len(status) - 2)
    keep = torch.arange(len(status), device="cuda") != 1
    assert torch.equal(loss2[keep], loss[keep]) and torch.equal(grad2[keep], grad[keep])
