"""CPU tier: every operator of the Newton loop ALONE, against an extended-precision restatement.

The linear solvers have tests/test_linsys_emul.py; this is the other half of a Newton iteration -- the code that builds
what the solvers are given and consumes what they return: the gathers y - M^T theta, the gradient g = -M Pi(r) in its
row-wise, long-row, streamed, column-wise fixed-point and prefix-sum forms, the Hessian M W M^T as a band, folded dense
and lite lower triangle, the weight functions, the line search (refresh_clipped, dphi, exact_step, update_theta) and the
epilogue.  A projected semismooth Newton method converges with a wrong Hessian, a wrong weight or a sloppy line search --
it only takes more iterations -- so nothing end-to-end sees such an error.  Each operator runs through the entries of
tests/prims/op_entries.h under the SIMT emulation on reduced cones that are supplied directly as SolveView arrays (rows
exactly on kLongRow / kTeamRow / the chunk sizes, every column count around the unrolled prefixes), and its output is
held to the bound derived in tests/ops_ref.py.  The fixed-point forms also run under a shuffled lane schedule and must
give the same bits.  The same cases run on the hardware in tests/test_gpu_ops.py, where the forms that differ there
(band_weight's rsqrt, v_rsq_f32 in lite_hessian, the DPP scan of lite_gradient, the 64-bit LDS atomics) are checked.
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest

import ops_cases as OC
import ops_ref as R
from emul_lib import Simt


@pytest.fixture(scope="module")
def simt():
    return Simt()


@pytest.fixture(scope="module")
def run(simt):
    yield simt.op_run
    OC.dump_margins("cpu_emulation")


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


def test_exact_step(simt):
    OC.check_exact_step(simt)


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
    OC.check_dense_gradient(run, ctx, pm1, seeds=(0, 77))


def test_band_weight(run):
    OC.check_band_weight(run, cap=4.0)


def test_band_weight_extremes(run):
    """z^2 overflows from |t / mu| = 1.4e154 on: the root is inf, the quotient 0 and the weight 1/2 where the limit is
    0 or 1; 1 / mu = inf with t = 0 gives 0 x inf = NaN.  Whether solve_cone_impl can get there: it builds a Hessian
    only while pgn / g0n > 1e-15 (the convergence test above it), so mu >= 0.03 max|y| min(1e-15, 0.7^it) and
    |t / mu| <= 33 |r_k| / max|y| / min(1e-15, 0.7^it).  That passes 1.4e154 only once 0.7^it < 1e-152, i.e. from
    iteration 985 on, and 1 / mu overflows only from iteration 1990 on (0.7^it denormal) -- out of reach of the default
    cap of 100 iterations and of every caller in this repository, reachable by a caller that raises max_iter past 985
    on a cone that does not converge (noted next to band_weight in cone_band.h).  Pinned here so that a change of
    either side shows up."""
    got = OC.band_weight_extremes(run)
    assert got[:4] == [0.5, 0.5, 0.5, 0.5] and np.isnan(got[4]) and np.isnan(got[5]), got


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", OC.LARGE_CTX)
def test_band_hessian(run, ctx, pm1):
    OC.check_band_hessian(run, ctx, pm1, seeds=(0, 78))


@pytest.mark.parametrize("pm1", [True, False])
@pytest.mark.parametrize("ctx", ["l2", "l4"])
def test_dense_hessian(run, ctx, pm1):
    OC.check_dense_hessian(run, ctx, pm1, seeds=(0, 79))


@pytest.mark.parametrize("ctx", ["w1", "b4", "solo"])
def test_epilogue(run, ctx):
    OC.check_epilogue(run, ctx)


def test_epilogue_reference_gradient_is_the_derivative():
    """the restatement's analytic d loss / d pred against a central difference of its own loss, target held constant"""
    e = [x for x in OC.epilogue_cases() if x["d"] == 63 and x["mode"] == R.MODE_INNER and x["what"] == "plain"][0]
    ref, _ = R.epilogue(e["mode"], e["sign"], e["ratio"], 0, e["y"], e["res"], e["f"], e["avg"])
    y = R._num(e["y"].astype(np.float64))
    for k in (0, 17, 62):
        h = R._num([1e-7])[0]
        yp, ym = y.copy(), y.copy()
        yp[k] += h
        ym[k] -= h
        num = -(ref["_cos"](yp) - ref["_cos"](ym)) / (2 * h) * e["sign"]
        assert abs(float(num - ref["grad"][k])) <= 1e-9 * max(1.0, abs(float(ref["grad"][k])))


def test_lite_gather_and_gradient(run):
    OC.check_lite_gather_gradient(run)


def test_lite_hessian_sequence(run):
    OC.check_lite_hessian(run)


def test_lite_hessian_ipm(run):
    OC.check_lite_hessian_ipm(run)
