"""CPU tier: the model minimisation of one Newton iteration ALONE, against an extended-precision restatement.

lite_model_step (cone_core.h) and dense_model_step (cone_dense.h) sit between the operators and the exact line search,
and the Newton loop forgives them everything: any descent direction converges, so a step that stops on the wrong face,
fixes the wrong row, forgets theta_I in the tableau's constant column or mixes ord[q] with q only costs iterations.
Here both run on their own through the entries of tests/prims/model_entries.h under the SIMT emulation -- every product
context (SoloCtx<32, 4>; WaveCtx, BlockCtx<2, true>, BlockCtx<4, true>), both lane schedules, the build with the 24-bit
reciprocal -- on seeded systems at the smallest shapes where each mechanism is live, and tests/model_cases.py asserts
the same path as tests/model_ref.py (long double), the bitwise contracts update_theta and the convergence test consume,
stationarity on the kernel's own face and descent.  The same cases run on the hardware in tests/test_gpu_model.py.
The sanitizer build runs as a program of its own (tests/emul/model_asan_main.cpp): cases in through a file, results
back through a file.  TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest

import linsys_ref as L
import model_cases as MC
import model_ref as MR
from emul_lib import Simt


@pytest.fixture(scope="module")
def run():
    simt = Simt()
    yield simt.model_run
    MC.dump_margins("emul")


@pytest.fixture(scope="module")
def run_rcp24():
    """the emulation whose v_rcp_f64 stand-in carries 24 bits (see tests/test_linsys_emul.py): the lite form is held to
    eps = 2^-45 there, the dense form (two Newton steps everywhere) keeps 2^-52"""
    yield Simt(defines=("SIMT_APPROX_RCP",), tag="_rcp24").model_run
    MC.dump_margins("emul_rcp24", prefix="rcp24:")


def test_reference_leaves_few_cases_undecided():
    """the cap, from the reference alone: at most 2 % of the random cases, at most one per group, have a comparison on
    their path closer to flipping than 4 B -- so the same-path assertion covers the suite and cannot drift"""
    tot = n = 0
    for form in ("lite", "dense"):
        t, k, worst = MC.undecided_in_reference(form, MC.EPS[form])
        print(f"{form}: {t} of {k} random cases undecided, worst group {worst}")
        assert worst <= 1, (form, worst)
        tot, n = tot + t, n + k
    assert tot <= 0.02 * n, (tot, n)


def test_reference_on_mpmath_agrees():
    """the fallback of linsys_ref (mpmath numbers where long double is too narrow) runs the same code to the same path"""
    mpmath = pytest.importorskip("mpmath")  # noqa: F841
    for form, p, nF in (("lite", 9, 4), ("dense", 12, 7)):
        H, theta, g = MC.draw_case(77, "gauss", p, nF, 1e-12)
        fn = MR.lite if form == "lite" else MR.dense
        a = fn(H, theta, g, nF, 1e-12)
        L.FORCE_MPMATH = True
        try:
            b = fn(H, theta, g, nF, 1e-12)
        finally:
            L.FORCE_MPMATH = False
        assert np.array_equal(a["held"], b["held"]) and a["moved"] == b["moved"] and a["rounds"] == b["rounds"]
        assert np.abs(a["tc"] - b["tc"]).max() <= 4 * np.finfo(np.float64).eps * np.abs(a["tc"]).max()


def test_reference_ends_stationary_on_its_face():
    """the restatement against first principles: at reg_rel = 0 its end point is feasible and the model's gradient
    vanishes on the free rows and on the bound rows it does not hold, in long double, and it is no worse than theta.
    (The loop only ever adds rows to the held set, so a held row may end with a negative gradient: the procedure's end
    point, not the constrained minimum, is what the kernels are compared with.)"""
    for form, p, nF in (("lite", 14, 8), ("dense", 20, 11)):
        fn = MR.lite if form == "lite" else MR.dense
        for seed in range(6):
            H, theta, g = MC.draw_case(1000 + seed, MC.FAMILIES[seed % 3], p, nF, 0.0)
            r = fn(H, theta, g, nF, 0.0)
            grad = np.array(g, np.longdouble) + np.array(H, np.longdouble) @ (np.array(r["tc"], np.longdouble) - np.array(theta, np.longdouble))
            tol = 1e-12 * r["kappa"] * max(np.abs(g).max(), 1.0)
            assert np.abs(grad[:nF]).max(initial=0.0) <= tol
            gI, held = grad[nF:], r["held"]
            assert np.abs(gI[~held]).max(initial=0.0) <= tol and (r["tc"][nF:] >= 0).all() and (r["tc"][nF:][held] == 0).all(), (form, seed)
            assert MR.model_value(r, r["tc"])[0] <= 0.0, (form, seed)


@pytest.mark.parametrize("p,nF", MC.LITE_SHAPES)
def test_lite_model_step(run, p, nF):
    reg, cases = MC.random_group("lite", p, nF)
    a, u0 = MC.check_group(run, "lite", "lite_model", p, nF, reg, cases, MC.EPS["lite"], "lite_model")
    b, u1 = MC.check_group(run, "lite", "lite_model", p, nF, reg, cases, MC.EPS["lite"], "lite_model", seed=21)
    assert u0 <= 1 and u1 <= 1
    assert np.array_equal(a["tc"].view(np.uint64), b["tc"].view(np.uint64))   # the schedule of the lanes changes nothing


@pytest.mark.parametrize("p,nF", MC.DENSE_SHAPES)
@pytest.mark.parametrize("kind", MC.DENSE_KINDS)
def test_dense_model_step(run, kind, p, nF):
    """identity order, and a seeded order that interleaves free and bound rows (a second draw); each under the
    round-robin and the shuffled lane schedule, which must give the same bits"""
    for gi, ord_ in ((0, None), (1, MC.seeded_ord(p, nF, 5 + p))):
        reg, cases = MC.random_group("dense", p, nF, gi)
        a, u0 = MC.check_group(run, "dense", kind, p, nF, reg, cases, MC.EPS["dense"], kind, ord_=ord_)
        b, u1 = MC.check_group(run, "dense", kind, p, nF, reg, cases, MC.EPS["dense"], kind, ord_=ord_, seed=22)
        assert u0 <= 1 and u1 <= 1
        assert np.array_equal(a["tc"].view(np.uint64), b["tc"].view(np.uint64))


@pytest.mark.parametrize("reg", (1e-12, 0.0))
@pytest.mark.parametrize("kind", ("lite_model",) + MC.DENSE_KINDS)
def test_constructed_cases(run, kind, reg):
    form = "lite" if kind == "lite_model" else "dense"
    p, nF = MC.CONSTRUCTED_SHAPE[form]
    cases = MC.constructed_group(form, reg)
    for ord_, seed in ((None, 0), (MC.seeded_ord(p, nF, 3), 23)):
        if form == "lite" and ord_ is not None:
            ord_ = None   # (the lite form has no order of its own: the second pass is the shuffled schedule alone)
        MC.check_group(run, form, kind, p, nF, reg, cases, MC.EPS[form], kind + ":constructed", ord_=ord_, seed=seed)


def test_with_a_24_bit_reciprocal(run_rcp24):
    for p, nF in MC.LITE_SHAPES:
        reg, cases = MC.random_group("lite", p, nF)
        _, u = MC.check_group(run_rcp24, "lite", "lite_model", p, nF, reg, cases, MC.EPS_RCP24["lite"], "rcp24:lite_model")
        assert u <= 1
    for p, nF in MC.DENSE_SHAPES:
        reg, cases = MC.random_group("dense", p, nF, 1)
        _, u = MC.check_group(run_rcp24, "dense", "dense_model_w2", p, nF, reg, cases, MC.EPS_RCP24["dense"], "rcp24:dense_model_w2",
                              ord_=MC.seeded_ord(p, nF, 5 + p))
        assert u <= 1
    for form, kind in (("lite", "lite_model"), ("dense", "dense_model_w2")):
        p, nF = MC.CONSTRUCTED_SHAPE[form]
        for reg in (1e-12, 0.0):
            MC.check_group(run_rcp24, form, kind, p, nF, reg, MC.constructed_group(form, reg), MC.EPS_RCP24[form], "rcp24:" + kind + ":constructed")


def test_model_steps_are_asan_ubsan_clean(tmp_path):
    """every constructed case and the limit shapes through the entries compiled with -fsanitize=address,undefined into a
    program of its own (the workgroup's LDS is an exact-size heap block there: an overrun of any array is a finding);
    the results are held to the same checks"""
    from emul_model_asan import AsanRunner

    runner = AsanRunner(str(tmp_path))
    for kind in ("lite_model",) + MC.DENSE_KINDS:
        form = "lite" if kind == "lite_model" else "dense"
        p, nF = MC.CONSTRUCTED_SHAPE[form]
        for reg in (1e-12, 0.0):
            MC.check_group(runner.run, form, kind, p, nF, reg, MC.constructed_group(form, reg), MC.EPS[form], "asan:" + kind,
                           ord_=None if form == "lite" else MC.seeded_ord(p, nF, 3), seed=24)
        for p, nF in MC.LIMIT_SHAPES[form]:
            reg, cases = MC.random_group(form, p, nF)
            MC.check_group(runner.run, form, kind, p, nF, reg, cases[:3], MC.EPS[form], "asan:" + kind)
    for k in [k for k in MC.MARGINS if k.startswith("asan:")]:   # (the same code as the plain build: not a tier of its own)
        del MC.MARGINS[k]
