"""GPU tier: the row scan of the step kernel's dense pack half (BlockCtx::scan_rows) through cave_hip_cone_step.

A fused chain of three steps over two alternating batches (A, B, A: the pack half of step i builds the store step i + 1
solves from) on the dense route against the same chain on the sparse route -- an untouched producer of the same lite
slots: losses, gradients, statuses and iteration counts bit for bit, the prepared stores byte for byte; the outputs
within the golden tolerances (tests/golden_cases.py) of the general operator cone_op_dense; two runs give the same bits.
B <= 8.  Shapes: one to four loads per row, fewer rows than a round of two waves and many rounds.  (40, 256), which the
issue names, has no fused launch in the product (step_limits stops at d = 228): asserted, and (40, 228) runs in its place."""

import numpy as np
import pytest

from golden_cases import TOL
from rowscan_cases import batch_of

pytestmark = pytest.mark.gpu

ARRAYS = ("hdr", "usign", "avg", "rowptr", "ell", "csr16", "rl")
OUTS = ("loss", "grad")
MODE_INNER = 2
SHAPES = [(7, 5), (13, 10), (40, 228), (235, 190)]


def _fresh(m, d):
    import torch

    from cave_amd import cave, qpsolver

    torch.cuda.synchronize()
    cave._pending_checks.clear()
    qpsolver.forget_shape(int(m), int(d))
    qpsolver._step_pool.clear()


def _sparse(ctrs):
    from cave_amd.sparse import SparseCones

    return SparseCones.from_dense(ctrs).cuda()


def _pack_only(x):
    """a pack-only launch into a freshly zeroed store: -> ({array: host copy}, pack status)"""
    import torch

    from cave_amd import qpsolver as Q

    sparse = not isinstance(x, torch.Tensor)
    B, d = (len(x), x.d) if sparse else (x.shape[0], x.shape[2])
    ss = Q._LiteSlots(x.device, B, d)
    ss.pack_status.fill_(-7)
    (Q._launch_step_sparse if sparse else Q._launch_step)(None, None, 0, 0, 1.0, 0.0, 0, {}, None, None, x, ss)
    torch.cuda.synchronize()
    return {k: ss.t[k].cpu().numpy() for k in ARRAYS}, ss.pack_status.cpu().numpy()


def _chain(pieces, preds):
    from cave_amd.qpsolver import PreparedCones, cone_op_prepared, prepare_cones

    prep = prepare_cones(pieces[0])
    outs = []
    for i, pred in enumerate(preds):
        assert isinstance(prep, PreparedCones), i
        if i + 1 < len(pieces):
            prep.then(pieces[i + 1])
        o = cone_op_prepared(prep, pred, MODE_INNER, -1.0, 0.2, outputs=OUTS)
        outs.append({k: o[k].cpu().numpy() for k in OUTS + ("status", "iters")})
        prep = prep.next
    return outs


def test_the_issues_256_column_shape_has_no_fused_launch():
    from cave_amd.qpsolver import step_lds_bytes

    assert step_lds_bytes(40, 256) <= 0 and step_lds_bytes(40, 229) <= 0 and step_lds_bytes(40, 228) > 0


@pytest.mark.parametrize("m,d", SHAPES)
def test_fused_chain_dense_equals_sparse_and_the_general_operator(m, d):
    import torch

    from cave_amd.qpsolver import cone_op_dense, step_lds_bytes

    assert step_lds_bytes(m, d) > 0
    _fresh(m, d)
    A, B = batch_of(5, m, d, B=8), batch_of(6, m, d, B=7)
    rng = np.random.default_rng([m, d])
    host = [A, B, A]
    preds = [torch.tensor(rng.standard_normal((len(c), d)).astype(np.float32), device="cuda") for c in host]
    # the prepared stores, byte for byte
    for c in (A, B):
        da, ds = _pack_only(torch.tensor(c, device="cuda"))
        sa, ss = _pack_only(_sparse(c))
        assert np.array_equal(ds, ss) and (ds == 0).all() and (da["hdr"][0::8] == 1).all(), (ds, ss)
        for k in ARRAYS:
            assert np.array_equal(da[k], sa[k]), k
    dense = _chain([torch.tensor(c, device="cuda") for c in host], preds)
    again = _chain([torch.tensor(c, device="cuda") for c in host], preds)
    sparse = _chain([_sparse(c) for c in host], preds)
    for i in range(3):
        assert (dense[i]["status"] == 0).all()
        for k in OUTS + ("status", "iters"):
            assert np.array_equal(dense[i][k], sparse[i][k]), (i, k)
            assert np.array_equal(dense[i][k], again[i][k]), (i, k, "two launches")
        ref = cone_op_dense(torch.tensor(host[i], device="cuda"), preds[i], MODE_INNER, -1.0, 0.2, outputs=OUTS, waves=2)
        rl, rg = ref["loss"].cpu().numpy(), ref["grad"].cpu().numpy()
        assert np.all(np.abs(dense[i]["loss"] - rl) <= TOL), i
        assert np.all(np.abs(dense[i]["grad"] - rg) <= 4 * TOL * max(1.0, float(np.abs(rg).max()))), i
    _fresh(m, d)
