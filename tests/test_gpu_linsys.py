"""GPU tier: every linear solver of the Newton loop ALONE on the MI355X, against the extended-precision reference.

The cases, the reference and the bound are those of tests/test_linsys_emul.py (tests/linsys_cases.py); the solvers run
as kernels of their own from tests/prims/_prims.so (the product's sources, flags, workgroup shapes and LDS layouts).
Only here do the forms that differ between the emulation and the hardware show what they compute:

  * the reciprocals -- v_rcp_f64 plus one Newton step in gj_solve_regs / gj_partial_regs (bound with eps = 2^-47), plus
    two in the other forms (2^-52); the emulation divides exactly;
  * the rank-4 trailing update of dense_factor on the f64 matrix cores (v_mfma_f64_16x16x4_f64: lane -> tile mapping,
    clamps for rows and columns past p), which hipcc alone compiles.  The same entry built with CAVE_DENSE_NO_MFMA (the
    two-columns-per-lane form the emulation runs) is held to the same bound, and how far apart the two forms are is
    recorded, not asserted.

The worst error / bound per entry of a run goes into profiles/linsys_margins.json (tier "mi355x"; the environment
variable CAVE_LINSYS_MARGINS names another file)."""

import os
import sys

import numpy as np
import pytest

import linsys_cases as LC

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "prims"))


@pytest.fixture(scope="module")
def prims():
    import prims_lib

    return prims_lib.Prims()


@pytest.fixture(scope="module")
def run(prims):
    yield prims.run
    LC.dump_margins("mi355x", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "linsys_margins.json"))


@pytest.mark.parametrize("kind,p", [(k, p) for k in LC.REG_KINDS for p in LC.reg_sizes(k)])
def test_register_solver(run, kind, p):
    LC.check_solves(run, kind, p, LC.reg_of(p, LC.REG_KINDS.index(kind)))


@pytest.mark.parametrize("kind", LC.REG_KINDS)
def test_register_solver_drops_zero_pivots(run, kind):
    if kind == "spd_solo":
        LC.check_solves(run, kind, 8, 0.0, zero_rows=LC.ZERO_ROWS_8)
    else:
        LC.check_solves(run, kind, 24, 0.0, zero_rows=LC.ZERO_ROWS_24)


@pytest.mark.parametrize("p", [p for p in LC.SIZES_REG if p <= 32])
def test_gj_partial(run, p):
    for k, nF in enumerate(LC.partial_nF(p)):
        LC.check_gj_partial(run, p, nF, LC.reg_of(p, k))


@pytest.mark.parametrize("nF", (24, 19))
def test_gj_partial_drops_zero_pivots(run, nF):
    LC.check_gj_partial(run, 24, nF, 0.0, zero_rows=LC.ZERO_ROWS_24[:1] + ((18,),) + LC.ZERO_ROWS_24[2:])


@pytest.mark.parametrize("nI", (8, 5, 1))
@pytest.mark.parametrize("seq", LC.EXCHANGES)
def test_tableau_exchange(run, seq, nI):
    LC.check_tableau(run, tuple(j for j in seq if j < nI) or (0,), nI)


def test_tableau_exchange_refuses_a_zero_pivot(run):
    LC.check_tableau(run, (0, 2, 5), 8, zero_row=2)


def _apart(a, b):
    """largest difference between two outputs, relative to the larger one's largest entry"""
    m = np.isfinite(a) & np.isfinite(b)
    s = max(float(np.abs(a[m]).max(initial=0.0)), float(np.abs(b[m]).max(initial=0.0)))
    return float(np.abs(a[m] - b[m]).max(initial=0.0)) / s if s > 0 else 0.0


@pytest.mark.parametrize("p", LC.SIZES_DENSE)
@pytest.mark.parametrize("kind", ("dense_w2", "dense_w4"))
def test_dense_ldl_mfma_and_plain_form(prims, run, kind, p):
    """dense_factor + dense_backsub with the MFMA trailing update and with the plain one: both within the bound"""
    for k, nF in enumerate(LC.dense_nF(p)):
        a = LC.check_dense(run, kind, p, nF, LC.reg_of(p, k))
        b = LC.check_dense(lambda *x, **kw: prims.run(*x, nomfma=True, **kw), kind, p, nF, LC.reg_of(p, k), tag=kind + "_nomfma")
        LC.record(kind + ":mfma_vs_plain_factor_rel", _apart(a["M"], b["M"]))
        LC.record(kind + ":mfma_vs_plain_x_rel", _apart(a["x"], b["x"]))
        print(f"{kind} p={p} nF={nF}: MFMA and plain form apart by {_apart(a['M'], b['M']):.3g} (factor), {_apart(a['x'], b['x']):.3g} (x)")


@pytest.mark.parametrize("nF", (24, 19))
@pytest.mark.parametrize("kind", ("dense_w2", "dense_w4"))
def test_dense_ldl_drops_zero_pivots(prims, run, kind, nF):
    zr = LC.ZERO_ROWS_24[:1] + ((18,),) + LC.ZERO_ROWS_24[2:]
    LC.check_dense(run, kind, 24, nF, 0.0, zero_rows=zr)
    LC.check_dense(lambda *x, **kw: prims.run(*x, nomfma=True, **kw), kind, 24, nF, 0.0, zero_rows=zr, tag=kind + "_nomfma")


@pytest.mark.parametrize("bw", [b for b in LC.BANDWIDTHS if b >= 4])
@pytest.mark.parametrize("kind", LC.BAND_WAVE_KINDS)
def test_band_wave(run, kind, bw):
    for k, p in enumerate(LC.band_sizes(bw)):
        LC.check_solves(run, kind, p, LC.reg_of(p, k), bw=bw)


@pytest.mark.parametrize("bw", LC.BANDWIDTHS)
@pytest.mark.parametrize("kind", LC.BAND_TEAM_KINDS)
def test_band_team(run, kind, bw):
    for k, p in enumerate(LC.band_sizes(bw)):
        LC.check_solves(run, kind, p, LC.reg_of(p, k), bw=bw)


@pytest.mark.parametrize("kind", LC.BAND_WAVE_KINDS + LC.BAND_TEAM_KINDS)
def test_band_drops_zero_pivots(run, kind):
    LC.check_solves(run, kind, 40, 0.0, bw=5, zero_rows=LC.ZERO_ROWS_40)
