"""GPU tier: the model minimisation of one Newton iteration ALONE on the MI355X, against the extended-precision
restatement.

The cases, the reference, the bound and the checks are those of tests/test_model_emul.py (tests/model_cases.py);
lite_model_step and dense_model_step run as kernels of their own from tests/prims/_prims.so (the product's sources, flags,
contexts and LDS sizes; tests/prims/model_entries.h).  Only here do the forms that differ between the emulation and the
hardware show what they compute: v_rcp_f64 plus one Newton step in gj_partial (the lite form's eps = 2^-47), the DPP
reductions of the tableau loop, and -- dense form -- the MFMA trailing update of dense_factor, held to the same bound as
the build with CAVE_DENSE_NO_MFMA; how far apart the two are is recorded, not asserted.  Every launch is repeated and
must give the same bits.

The worst error / bound per entry goes into profiles/model_step_margins.json (tier "mi355x"; the environment variable
CAVE_MODEL_MARGINS names another file)."""

import os
import sys

import numpy as np
import pytest

import model_cases as MC

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "prims"))


@pytest.fixture(scope="module")
def prims():
    import prims_lib

    p = prims_lib.Prims()
    yield p
    MC.dump_margins("mi355x", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "model_step_margins.json"))


def _twice(prims, form, kind, p, nF, reg, cases, tag, ord_=None, **kw):
    a, u = MC.check_group(prims.model_run, form, kind, p, nF, reg, cases, MC.EPS[form], tag, ord_=ord_, **kw)
    b = MC.launch(prims.model_run, form, kind, p, nF, reg, cases, ord_, **kw)
    for k in ("tc", "moved", "sact", "ss"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (kind, p, nF, k, "two launches differ")
    return a, u


def _apart(a, b):
    s = max(float(np.abs(a).max(initial=0.0)), float(np.abs(b).max(initial=0.0)))
    return float(np.abs(a - b).max(initial=0.0)) / s if s > 0 else 0.0


@pytest.mark.parametrize("p,nF", MC.LITE_SHAPES)
def test_lite_model_step(prims, p, nF):
    reg, cases = MC.random_group("lite", p, nF)
    _, u = _twice(prims, "lite", "lite_model", p, nF, reg, cases, "lite_model")
    assert u <= 1


_MFMA_TC: dict = {}   # tc of the MFMA build per (kind, p, nF, order), kept for the plain build's test to measure against


def _order(p, nF, order):
    """(group of the draw, ord): the identity order on the first draw, the seeded interleaving on the second"""
    return (0, None) if order == "identity" else (1, MC.seeded_ord(p, nF, 5 + p))


@pytest.mark.parametrize("order", ("identity", "seeded"))
@pytest.mark.parametrize("p,nF", MC.DENSE_SHAPES)
@pytest.mark.parametrize("kind", MC.DENSE_KINDS)
def test_dense_model_step(prims, kind, p, nF, order):
    """the product's build (MFMA trailing update): two launches, same bits"""
    gi, ord_ = _order(p, nF, order)
    reg, cases = MC.random_group("dense", p, nF, gi)
    a, u = _twice(prims, "dense", kind, p, nF, reg, cases, kind, ord_=ord_)
    assert u <= 1
    _MFMA_TC[(kind, p, nF, order)] = a["tc"]


@pytest.mark.parametrize("order", ("identity", "seeded"))
@pytest.mark.parametrize("p,nF", MC.DENSE_SHAPES)
@pytest.mark.parametrize("kind", MC.DENSE_KINDS)
def test_dense_model_step_plain_update(prims, kind, p, nF, order):
    """the build with CAVE_DENSE_NO_MFMA: the same bound, two launches, same bits; how far its tc is from the MFMA
    build's (the test above; launched here if that did not run) is recorded, not asserted"""
    gi, ord_ = _order(p, nF, order)
    reg, cases = MC.random_group("dense", p, nF, gi)
    b, u = _twice(prims, "dense", kind, p, nF, reg, cases, kind + "_nomfma", ord_=ord_, nomfma=True)
    assert u <= 1
    a = _MFMA_TC.get((kind, p, nF, order))
    if a is None:
        a = MC.launch(prims.model_run, "dense", kind, p, nF, reg, cases, ord_)["tc"]
    MC.record(kind + ":mfma_vs_plain_tc_rel", _apart(a, b["tc"]))
    print(f"{kind} p={p} nF={nF} {order}: MFMA and plain form apart by {_apart(a, b['tc']):.3g} (tc)")


@pytest.mark.parametrize("reg", (1e-12, 0.0))
@pytest.mark.parametrize("kind,nomfma", [("lite_model", False)] + [(k, n) for k in MC.DENSE_KINDS for n in (False, True)])
def test_constructed_cases(prims, kind, nomfma, reg):
    form = "lite" if kind == "lite_model" else "dense"
    p, nF = MC.CONSTRUCTED_SHAPE[form]
    cases = MC.constructed_group(form, reg)
    kw = {"nomfma": True} if nomfma else {}
    _twice(prims, form, kind, p, nF, reg, cases, kind + ("_nomfma" if nomfma else "") + ":constructed",
           ord_=None if form == "lite" else MC.seeded_ord(p, nF, 3), **kw)
