"""GPU tier: every operator of the Newton loop ALONE on the MI355X, against the extended-precision restatement.

The cases, the restatement and the bounds are those of tests/test_ops_emul.py (tests/ops_cases.py, tests/ops_ref.py);
the operators run as kernels of their own from tests/prims/_prims.so (tests/prims/ops_abi.hip: the product's sources,
flags, context types and LDS layouts).  Only here do the forms that differ between the emulation and the hardware show
what they compute: the lite_* functions (DPP scans, __builtin_amdgcn_rsqf), band_weight's rsqrt, the 64-bit LDS atomics
of the fixed-point forms, the global_* loads of the streamed forms.  The fixed-point forms are launched twice and must
give the same bits.  The worst error / bound per entry of a run goes into profiles/ops_margins.json (tier "mi355x"; the
environment variable CAVE_OPS_MARGINS names another file)."""

import os
import sys

import numpy as np
import pytest

import ops_cases as OC

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "prims"))


@pytest.fixture(scope="module")
def run():
    import prims_lib

    yield prims_lib.Prims().op_run
    OC.dump_margins("mi355x", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "ops_margins.json"))


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", OC.SMALL_CTX)
def test_gather_mt(run, ctx, pm1):
    OC.check_gather(run, "gather", ctx, pm1, "gather_mt")


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", OC.LARGE_CTX)
def test_gather_mt_streamed(run, ctx, pm1):
    OC.check_gather(run, "gather_st", ctx, pm1, "gather_mt_streamed")


def test_gather_mt_streamed_diet(run):
    OC.check_gather(run, "gather_diet", "l4", True, "gather_mt_streamed_diet")


@pytest.mark.parametrize("ctx,rb", [(c, 0) for c in ("w1", "b2", "b4", "solo")] + [(c, 1) for c in OC.LARGE_CTX])
def test_refresh_clipped_dphi_update_theta(run, ctx, rb):
    OC.check_refresh(run, ctx, rb)
    OC.check_dphi(run, ctx, rb)
    OC.check_update_theta(run, ctx, rb)


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", OC.SMALL_CTX)
def test_gradient(run, ctx, pm1):
    OC.check_gradient(run, "grad", ctx, pm1, "gradient")


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", OC.LARGE_CTX)
def test_gradient_streamed(run, ctx, pm1):
    OC.check_gradient(run, "grad_st", ctx, pm1, "gradient_streamed")


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", ["l2", "l4"])
def test_dense_gradient(run, ctx, pm1):
    OC.check_dense_gradient(run, ctx, pm1, seeds=(0, 0))  # two launches: the same bits


def test_band_weight(run):
    """16 x 2^-52 where z >= 0 (8 u (w + |q| / 2) for both signs): a condition on the rsqrt form, not a measurement"""
    OC.check_band_weight(run, cap=8.0)


def test_band_weight_extremes(run):
    """as tests/test_ops_emul.py: with rsqrt, 1 / sqrt(inf) = 0 gives the same 1/2, and 0 x inf the same NaN"""
    got = OC.band_weight_extremes(run)
    assert got[:4] == [0.5, 0.5, 0.5, 0.5] and np.isnan(got[4]) and np.isnan(got[5]), got


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", OC.LARGE_CTX)
def test_band_hessian(run, ctx, pm1):
    OC.check_band_hessian(run, ctx, pm1, seeds=(0, 0), wcap=8)


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", ["l2", "l4"])
def test_dense_hessian(run, ctx, pm1):
    OC.check_dense_hessian(run, ctx, pm1, seeds=(0, 0), wcap=8)


@pytest.mark.parametrize("ctx", ["w1", "b4", "solo"])
def test_epilogue(run, ctx):
    OC.check_epilogue(run, ctx)


def test_lite_gather_and_gradient(run):
    OC.check_lite_gather_gradient(run)


def test_lite_hessian_sequence(run):
    OC.check_lite_hessian(run)


def test_lite_hessian_ipm(run):
    OC.check_lite_hessian_ipm(run)
