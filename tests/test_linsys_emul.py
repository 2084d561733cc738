"""CPU tier: every linear solver of the Newton loop ALONE, against an extended-precision reference.

The end-to-end tests cannot see a solver that is slightly wrong: the semismooth Newton iteration has an exact line
search and corrects itself, so a damped rank-1 term or a 1e-3 error in a multiplier only costs iterations (measured:
five such mutations left all 108 emulation tests green).  Here each solver -- the register Gauss-Jordan forms of
wave_prims.h behind every context's solve_spd / solve_spd_tri, gj_partial, tableau_exchange, dense_factor +
dense_backsub (cone_dense.h), solve_spd_band_wave and solve_spd_band (cone_band.h) -- runs on its own through the
entries of tests/prims/prim_entries.h under the SIMT emulation, on seeded H = M W M^T systems at every dispatch
threshold, and its output is compared with tests/linsys_ref.py (long double) under

    || x - x_ref ||_inf <= p * eps * kappa_2 * || x_ref ||_inf,    eps = 2^-47 (one Newton step on the reciprocal) or 2^-52

(matrix outputs entry-wise, relative to the block's largest entry, kappa_2 of the regularised free block).  The same
cases run on the hardware in tests/test_gpu_linsys.py; the emulation's reciprocal is exact, so the 2^-47 forms are
only checked for real there.  TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest

import linsys_cases as LC
import linsys_ref as L
from emul_lib import Simt


@pytest.fixture(scope="module")
def run():
    simt = Simt()
    yield simt.prim_run
    LC.dump_margins("cpu_emulation")


@pytest.fixture(scope="module")
def run_rcp24():
    """the emulation built with SIMT_APPROX_RCP: its v_rcp_f64 stand-in is a single-precision reciprocal (24 bits, a
    little less than the instruction gives), so the Newton steps behind every reciprocal have to earn the accuracy the
    bound assumes already in the CPU tier.  The stand-in rounds its argument and its quotient to single precision:
    relative error d <= 2^-23, which one Newton step squares to 2^-46 -- above the 2^-47 the hardware forms are held to
    on the GPU -- so the one-step forms are held to eps = 2^-45 here (d^2 plus the rounding of the step itself); two
    steps leave 2^-92 and those forms keep 2^-52"""
    return Simt(defines=("SIMT_APPROX_RCP",), tag="_rcp24").prim_run


def test_reference_is_extended_precision_and_its_fallback_agrees():
    """long double carries 64 mantissa bits here; where it does not, the reference runs on mpmath numbers -- the same
    code, checked against each other on one system"""
    H = L.draw_spd(5, "scaled", 24, 1e-12)
    rhs = np.random.default_rng(5).standard_normal(24)
    act = L.act_patterns(np.random.default_rng(6), 24)["random20"]
    a = L.solve(H, rhs, act, 1e-12)
    assert L._wide_enough() == (np.finfo(np.longdouble).eps <= 2.0 ** -63)
    L.FORCE_MPMATH = True
    try:
        assert not L._wide_enough()
        b = L.solve(H, rhs, act, 1e-12)
        pb = L.partial(H, rhs, 17, 1e-12, x_bound=np.ones(7))
    finally:
        L.FORCE_MPMATH = False
    pa = L.partial(H, rhs, 17, 1e-12, x_bound=np.ones(7))
    assert np.abs(a["x"] - b["x"]).max() <= 4 * np.finfo(np.float64).eps * np.abs(a["x"]).max()
    for k in ("X", "S", "xg", "rI", "U", "dinv", "zF", "xF"):
        assert np.abs(pa[k] - pb[k]).max() <= 4 * np.finfo(np.float64).eps * np.abs(pa[k]).max(), k
    # and it is a solve: residual of the masked system in long double
    K = np.array(H, np.longdouble)
    free = act == 0
    K[np.diag_indices(24)] += np.longdouble(1e-12) * H.diagonal()[free].max()
    K[~free, :] = 0
    K[~free, ~free] = 1
    assert float(np.abs(K @ np.array(a["x"], np.longdouble) - rhs).max()) <= 1e-13 * a["kappa"] ** 0 * 24 * np.abs(K).max() * np.abs(a["x"]).max()


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


@pytest.mark.parametrize("p", LC.SIZES_DENSE)
@pytest.mark.parametrize("kind", ("dense_w2", "dense_w4"))
def test_dense_ldl(run, kind, p):
    for k, nF in enumerate(LC.dense_nF(p)):
        LC.check_dense(run, kind, p, nF, LC.reg_of(p, k))


@pytest.mark.parametrize("nF", (24, 19))
@pytest.mark.parametrize("kind", ("dense_w2", "dense_w4"))
def test_dense_ldl_drops_zero_pivots(run, kind, nF):
    LC.check_dense(run, kind, 24, nF, 0.0, zero_rows=LC.ZERO_ROWS_24[:1] + ((18,),) + LC.ZERO_ROWS_24[2:])


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


def test_shuffled_lane_order(run):
    """one seeded shuffled schedule of the lanes between two rendezvous: a hand-over through LDS the source does not
    order computes wrong numbers here"""
    for kind, p in (("gj", 33), ("gjs_tri", 57), ("spd_l4", 64), ("spd_b4", 29), ("tri_l4", 41), ("spd_solo", 8)):
        LC.check_solves(run, kind, p, 1e-12, seed=11)
    LC.check_gj_partial(run, 25, 20, 1e-12, seed=12)
    LC.check_tableau(run, LC.EXCHANGES[4], 8, seed=13)
    for kind, p, nF in (("dense_w2", 66, 61), ("dense_w4", 127, 100), ("dense_w4", 33, 33)):
        LC.check_dense(run, kind, p, nF, 1e-12, seed=14)
    for kind, bw, p in (("bandw1", 13, 97), ("bandw2", 33, 129), ("bandw2", 4, 65), ("band_hot_l4", 12, 65),
                        ("band_hot_l2", 3, 65), ("band_cold_l4", 2, 65), ("band_hot_w1", 34, 65)):
        LC.check_solves(run, kind, p, 1e-12, bw=bw, seed=15)


def test_with_a_24_bit_reciprocal(run_rcp24):
    """every entry once more with the approximate reciprocal (see run_rcp24); recorded under its own names"""
    run, e1 = run_rcp24, 2.0 ** -45
    for kind in LC.REG_KINDS:
        for p in (1, 8, 17, 33, 64):
            if p <= LC.KIND_PMAX.get(kind, 64):
                LC.check_solves(run, kind, p, LC.reg_of(p, LC.REG_KINDS.index(kind)), tag="rcp24:" + kind, eps_one=e1)
    for p, nF in ((1, 1), (9, 4), (25, 20), (32, 29)):
        LC.check_gj_partial(run, p, nF, LC.reg_of(p, nF), tag="rcp24:partial", eps_one=e1)
    for seq in LC.EXCHANGES:
        LC.check_tableau(run, seq, 8, tag="rcp24:tableau")
    for kind, p, nF in (("dense_w2", 1, 1), ("dense_w2", 17, 14), ("dense_w4", 66, 61), ("dense_w4", 128, 97), ("dense_w2", 33, 33)):
        LC.check_dense(run, kind, p, nF, LC.reg_of(p, nF), tag="rcp24:" + kind)
    for kind, bw, p in (("bandw1", 4, 6), ("bandw1", 13, 97), ("bandw2", 34, 129), ("band_hot_w1", 1, 65), ("band_hot_l2", 3, 65),
                        ("band_hot_l4", 12, 97), ("band_cold_l4", 33, 65)):
        LC.check_solves(run, kind, p, LC.reg_of(p, bw), bw=bw, tag="rcp24:" + kind)
