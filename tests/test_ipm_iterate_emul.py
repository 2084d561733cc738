"""CPU tier: the interior-point iterate of CAVE_MODE_INNER_IPM against its own definition.

tests/ipm_ref.py restates DESIGN section 3c and the comment above solve_cone_ipm_impl in extended precision;
tests/ipm_cases.py holds the inputs and the bound.  Every implementation of the mode that a CPU can run is held to that
restatement here, at 1, 2, 3 and 6 steps -- the step counts the mode is used at; by 12 steps the iterate has nearly
converged and a wrong constant hides again:

  serial build          Emul.cone_dense, Emul.cone_dense_large (small cones forced onto the band / dense forms too)
  SIMT emulation        Simt.cone_dense at 1 / 2 / 4 waves under two lane schedules (BlockCtx: fixed-point Hessian)
                        Simt.cone_packed_large at 2 waves on the band and dense forms
                        SimtStepIpm.step_solve_ipm (lite_solve_ipm) through step_pack and lite_from_packed
  the solver alone      tests/prims/ipm_entries.h: res, theta, z in double after k steps (assertion (b))

(a) float outputs within 2^-24 |ref| + E_k;  (b) the double state within E_k;  (c) at 24 steps, where tau sits on its
floor, within TOL sc;  (d) y 2^e gives proj 2^e, rnorm 2^e and the same loss and target, e = -20 and +10;  (e) the cap
on ill-conditioned cases, asserted from the reference alone.  Nothing is compared with another kernel.
TEST INFRASTRUCTURE: nothing in cave_amd loads these builds."""

import numpy as np
import pytest

import ipm_cases as IC
import ipm_ref as I
import limit_cones as LC
from emul_lib import Emul, store_bandwidth
from emul_step_ipm_lib import SimtStepIpm
from golden_cases import TOL
from oracle import cave_oracle as O

SEEDS = (0, 17)   # round robin, one shuffled lane schedule
OUT = ("proj", "rnorm", "target", "loss", "grad", "status", "iters")


@pytest.fixture(scope="module", autouse=True)
def _margins_file():
    yield
    IC.write_record("emulation")


@pytest.fixture(scope="module")
def simt():
    return SimtStepIpm()


@pytest.fixture(scope="module")
def emul():
    return Emul()


def budget(name, ctrs):
    """non-zero budget and LDS figure of the general kernels: the product's defaults, except on the limit cones"""
    return (LC.dense_nnz(ctrs) + 64, 160 * 1024) if name.startswith("limit/") else (0, 0)


def same_bits(a, b, what):
    for k in OUT:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def check_scaling(out, name, what, k=3, weights="f32"):
    """(d): rows 5 i + 3 (y 2^-20) and 5 i + 4 (y 2^10) against row 5 i (y) -> does it hold bit for bit.
    The procedure is scale free; the epilogue is not where its clamp of |proj|_2 at 1e-8 acts (the reference's
    clamp(norm, 1e-8): `setup` projects onto nearly nothing, and times 2^-20 that falls below the clamp), so target and
    loss are compared where the REFERENCE's |proj|_2 of both rows is above 2e-8."""
    f = IC.family(name)
    bitwise = True
    for b0 in np.flatnonzero(f["kind"] == 0):
        for off, e in ((3, -20), (4, 10)):
            a, g = b0 + off, b0
            assert f["kind"][a] == off and np.array_equal(f["y"][a], f["y"][g] * np.float32(2.0 ** e))
            pn = min(float(np.sqrt((I.L._f64(IC.reference(name, int(r), weights)[1][k]["proj"]) ** 2).sum())) for r in (a, g))
            for q, pw in (("proj", e), ("rnorm", e)) + ((("loss", 0), ("target", 0)) if pn > 2e-8 else ()):
                want = np.atleast_1d(out[q][g]).astype(np.float64) * 2.0 ** pw
                got = np.atleast_1d(out[q][a]).astype(np.float64)
                ulp = np.spacing(np.abs(np.atleast_1d(out[q][g])).astype(np.float32)).astype(np.float64) * 2.0 ** pw
                assert (np.abs(got - want) <= ulp).all(), (what, name, int(g), e, q, float(np.abs(got - want).max()))
                bitwise = bitwise and bool((got == want).all())
    IC.RECORD[f"{what}|{name.split('/')[0]}|scaling_bitwise"] = min(IC.RECORD.get(f"{what}|{name.split('/')[0]}|scaling_bitwise", 1.0),
                                                                   float(bitwise))
    return bitwise


# ------------------------------------------------------------------------------------------ the reference, alone
def test_cap_on_ill_conditioned_cases_from_the_reference_alone():
    """(e): E_k <= TOL sc / 4 on every fixture, limit cone and constructed cone; at most 2 % of the random draws
    (the synthetic and banded cones of the large path) may exceed it.  No kernel is called."""
    n_rand = bad_rand = 0
    for name in IC.SMALL:
        for b in range(len(IC.family(name)["y"])):
            for fixed in (False, True):
                assert not IC.capped(name, b, "f32", fixed), (name, b, fixed)
            assert not IC.capped(name, b, "f32", False, True), (name, b, "reciprocals of the device")
            assert not IC.capped(name, b, "f64"), (name, b)   # the same cone forced onto the large path
    for name in IC.LARGE:
        for b in range(len(IC.family(name)["y"])):
            n_rand += 1
            bad_rand += IC.capped(name, b, "f64")
    assert bad_rand <= 0.02 * n_rand, (bad_rand, n_rand)
    worst = max(max(IC.E(n, b, k, "f32", True)[q] for q in IC.COMPARED) / IC.scale_of(n, b)
                for n in IC.SMALL for b in range(len(IC.family(n)["y"])) for k in IC.K_STEPS)
    print(f"largest E_k / sc over the small families: {worst:.2e} (cap {TOL / 4:.1e})")
    IC.RECORD["reference|largest E_k / sc"] = worst


def test_the_inputs_take_the_branches_they_are_meant_for():
    """from the reference's own state: the step lengths of the constructed cones, the 0.995 branch on tsp20, the
    0.2 tau branch on sp5, no step without reduced rows, usign = 3, a duplicated row, one bound row"""
    f = IC.family("built")
    at = {n: 5 * i for i, n in enumerate(f["names"])}
    for n, want in IC.ALPHA_WANT.items():
        c, ref = IC.reference("built", at[n])
        assert want(float(ref[1]["alpha_p"]), float(ref[1]["alpha_d"])), (n, ref[1]["alpha_p"], ref[1]["alpha_d"])
    c, ref = IC.reference("built", at["unit_only"])
    assert c["p"] == 0 and ref[3] is ref[0] and float(ref[0]["tau"]) == pytest.approx(0.1 * np.abs(f["y"][at["unit_only"]]).max() ** 2)
    assert (IC.reference("built", at["both_signs"])[0]["usign"] == 3).sum() == 2
    c = IC.reference("built", at["dup_row"])[0]
    assert np.array_equal(c["M"][0], c["M"][1]) and (c["vkind"] == 0).all()
    c = IC.reference("built", at["one_bound"])[0]
    assert c["p"] == 1 and c["vkind"][0] == 0 and (c["usign"] == 0).all()
    c = IC.reference("built", at["pair_and_ineq"])[0]
    assert list(c["vkind"]) == [1, 1, 0, 0, 0]
    assert set(IC.reference("built", at["one_sign"])[0]["usign"]) == {0, 1}
    for b in range(0, 20, 5):
        c, ref = IC.reference("tsp20", b)
        assert 2 <= (c["vkind"] == 0).sum() <= 5 and float(ref[1]["alpha_p"]) < 1
        c, ref = IC.reference("sp5", b)
        assert (c["vkind"] == 1).all() and float(ref[1]["tau"]) == pytest.approx(0.2 * float(ref[0]["tau"]), rel=1e-15)
        assert not IC.reference("generic", b)[0]["pm1"] and not IC.reference("setup", b)[0]["pm1"]
    # tau reaches its floor by 24 steps on the inputs of (c)
    for name, rows in IC.FLOOR_ROWS.items():
        for b in rows:
            ref = IC.reference(name, b, "f32", IC.K_FLOOR)[1]
            ymax = float(np.abs(IC.family(name)["y"][b]).max())
            assert float(ref[-1]["tau"]) == pytest.approx(1e-14 * ymax * ymax, rel=1e-12), (name, b)


MUTATIONS = {
    "0.99 for 0.995": dict(consts={"frac": 0.99}), "0.25 for 0.2": dict(consts={"sigma": 0.25}),
    "tau0 = 0.2 ymax^2": dict(consts={"tau0": 0.2}), "floor 1e-10": dict(consts={"floor": 1e-10}),
    "- z dropped from dz": dict(mutate=("no_minus_z",)), "alpha_d on theta": dict(mutate=("alpha_d_on_theta",)),
    "final smoothing at the old tau": dict(mutate=("old_tau",)), "z / theta not on the diagonal": dict(mutate=("no_diag_barrier",)),
    "tau / theta not on the right-hand side": dict(mutate=("no_rhs_barrier",)), "nineq counts every row": dict(mutate=("nineq_all",)),
    "u = 1 and u = 2 swapped": dict(mutate=("swap_u",)),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_the_bound_sees_every_departure_from_the_procedure(what):
    """The reference with one constant or term changed, against the reference: on at least one input of the suite it
    lies more than a thousand bounds away (float outputs at k <= 6; the floor at k = 24 by more than TOL sc).  So a
    kernel with that error cannot pass (a) / (c).  Measured on the reference alone."""
    worst = 0.0
    if what == "floor 1e-10":
        for name, rows in IC.FLOOR_ROWS.items():
            f = IC.family(name)
            for b in rows:
                c, ref = IC.reference(name, b, "f32", IC.K_FLOOR)
                mut = I.iterate(c, f["y"][b], IC.K_FLOOR, "f32", **MUTATIONS[what])
                worst = max(worst, float(np.abs(I.L._f64(mut[-1]["proj"] - ref[-1]["proj"])).max()) / (TOL * IC.scale_of(name, b)))
        assert worst > 1.0, worst
        return
    for name in ("tsp20", "sp5", "generic", "built"):
        f = IC.family(name)
        for b in np.flatnonzero(f["kind"] == 0):
            c, ref = IC.reference(name, int(b))
            mut = I.iterate(c, f["y"][b], 3, "f32", **MUTATIONS[what])
            for k in (1, 2, 3):
                _, bnd = I.output_bounds(c, f["y"][b], ref[k], IC.E(name, int(b), k, "f32", True), IC.SIGN)
                worst = max(worst, float((np.abs(I.L._f64(mut[k]["proj"] - ref[k]["proj"])) / bnd["proj"]).max()))
    assert worst > 1e3, (what, worst)


def test_the_weights_switch_is_visible_in_the_double_state():
    """rho' kept in float32 or in double: the two references differ by more than 4 E_k on tsp20 at every k <= 3, so the
    comparison of the double state is known to see 1e-8 and a form checked with the wrong switch fails."""
    for b in range(0, 20, 5):
        for k in (1, 2, 3):
            a, w = IC.reference("tsp20", b, "f32")[1][k], IC.reference("tsp20", b, "f64")[1][k]
            for q in ("rho", "theta_b"):
                qq = "proj" if q == "rho" else q
                e = max(IC.E("tsp20", b, k, "f32", True)[qq], IC.E("tsp20", b, k, "f64", True)[qq])
                assert I._dev(a[q], w[q]) > 4 * e, (b, k, q, I._dev(a[q], w[q]), e)


def test_the_oracle_epilogue_agrees_with_the_restated_one():
    """target, loss and gradient of the reference's projection through oracle/cave_oracle.py (float32 / float64 numpy)
    agree with the extended-precision epilogue of ops_ref.py, which the comparisons use, to float32 rounding"""
    for name in ("tsp20", "generic"):
        f = IC.family(name)
        for b in (0, 1, 5):
            c, ref = IC.reference(name, b)
            vals, scale = I.outputs(c, f["y"][b], ref[3], IC.SIGN)
            p32 = I.L._f64(vals["proj"]).astype(np.float32)[None]
            t = p32 / np.maximum(O._rownorm(p32), np.float32(1e-8))
            pred = f["pred"][b][None]
            assert np.abs(t[0] - I.L._f64(vals["target"])).max() <= 4 * I.U32
            assert abs(float(O.cone_loss(pred, t, IC.SIGN)[0]) - float(vals["loss"])) <= 8 * I.U32
            assert np.abs(O.cone_loss_grad(pred, t, IC.SIGN)[0] - I.L._f64(vals["grad"])).max() <= 8 * I.U32 * scale["grad"]


def test_the_reference_runs_on_mpmath_where_long_double_is_narrow():
    """the fallback of linsys_ref, forced once: same states to 1e-17"""
    f = IC.family("built")
    b = 5 * f["names"].index("pair_and_ineq")
    c, ref = IC.reference("built", b)
    I.L.FORCE_MPMATH = True
    try:
        alt = I.iterate(c, f["y"][b], 2)
    finally:
        I.L.FORCE_MPMATH = False
    for k in (1, 2):
        assert alt[k]["proj"].dtype == object
        assert np.abs(I.L._f64(alt[k]["proj"]) - I.L._f64(ref[k]["proj"])).max() <= 1e-15


# ------------------------------------------------------------------------------------------------- (a), (d): floats
@pytest.mark.parametrize("name", IC.SMALL)
def test_serial_build(emul, name):
    f = IC.family(name)
    cap, lds = budget(name, f["ctrs"])
    outs = {}
    for k in IC.K_STEPS:
        o = emul.cone_dense(f["ctrs"], f["pred"], IC.MODE_IPM, sign=IC.SIGN, max_iter=k, nnz_cap=cap, lds_bytes=lds)
        IC.compare(o, name, k, "f32", False, "serial/cone_dense", IC.RECORD)
        check_scaling(o, name, "serial/cone_dense", k)
        outs[k] = o
    same_bits(emul.cone_dense(f["ctrs"], f["pred"], IC.MODE_IPM, sign=IC.SIGN, max_iter=0, nnz_cap=cap, lds_bytes=lds), outs[3],
              (name, "max_iter = 0 means 3"))


@pytest.mark.parametrize("name", IC.SMALL + IC.LARGE)
def test_serial_build_large_path(emul, name):
    """the band / dense forms keep rho' in doubles: weights = 'f64'"""
    f = IC.family(name)
    outs = {}
    for k in IC.K_STEPS:
        o = emul.cone_dense_large(f["ctrs"], f["pred"], IC.MODE_IPM, sign=IC.SIGN, max_iter=k)
        IC.compare(o, name, k, "f64", False, "serial/cone_dense_large", IC.RECORD)
        if name in IC.SMALL:
            check_scaling(o, name, "serial/cone_dense_large", k, "f64")
        outs[k] = o
    same_bits(emul.cone_dense_large(f["ctrs"], f["pred"], IC.MODE_IPM, sign=IC.SIGN, max_iter=0), outs[3], (name, "max_iter = 0"))


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("name", IC.SMALL)
def test_general_kernels_under_emulation(simt, name, waves):
    """WaveCtx (floating-point sums in lane order) and BlockCtx<2/4> (64-bit fixed-point Hessian: F_k joins the bound);
    the lane schedule changes nothing"""
    f = IC.family(name)
    cap, lds = budget(name, f["ctrs"])
    for k in IC.K_STEPS:
        prev = None
        for seed in SEEDS:
            o = simt.cone_dense(f["ctrs"], f["pred"], IC.MODE_IPM, sign=IC.SIGN, max_iter=k, waves=waves, seed=seed) if not cap else \
                simt.general_ipm(f["ctrs"], f["pred"], k, waves, sign=IC.SIGN, nnz_cap=cap, lds_bytes=lds)
            IC.compare(o, name, k, "f32", waves > 1, f"simt/cone_dense/w{waves}", IC.RECORD)
            check_scaling(o, name, f"simt/cone_dense/w{waves}", k)
            if prev is not None and waves > 1:   # fixed point: the order in which the lanes arrive changes no bit
                same_bits(o, prev, (name, k, waves, "schedule"))
            prev = o
            if cap:
                break   # (general_ipm takes no schedule)


@pytest.mark.parametrize("name", IC.LARGE + ("tsp20", "generic"))
def test_large_path_under_emulation(emul, simt, name):
    """cave_hip_cone_packed_large's code at two waves: band_hessian + the band elimination (sp12, band4), dense_hessian +
    dense_factor (tsp30, and the small cones, which the dense shape takes)"""
    f = IC.family(name)
    rows = np.arange(len(f["y"])) if name in IC.LARGE else np.arange(0, 10)
    st, arrs, mr, _ = emul.pack_large(f["ctrs"][rows])
    bw = store_bandwidth(arrs, len(rows), f["ctrs"].shape[2])
    for k in IC.K_STEPS:
        for seed in SEEDS:
            o = simt.cone_packed_large(st, arrs, mr, bw, np.arange(len(rows)), f["pred"][rows], IC.MODE_IPM, sign=IC.SIGN,
                                       max_iter=k, waves=2, seed=seed)
            full = {q: np.zeros((len(f["y"]),) + o[q].shape[1:], o[q].dtype) for q in o}
            for q in o:
                full[q][rows] = o[q]
            IC.compare(full, name, k, "f64", False, "simt/cone_packed_large/w2", IC.RECORD, rows=rows)


# (the limit cones reach the lite store through lite_from_packed only, as in tests/test_step_ipm_emul.py)
LITE_ROUTES = [(n, "step_pack") for n in IC.PM1_ONLY if not n.startswith("limit/")] + [(n, "lite_from_packed") for n in IC.PM1_ONLY]


@pytest.mark.parametrize("name,route", LITE_ROUTES)
def test_lite_solve_under_emulation(emul, simt, name, route):
    """lite_solve_ipm on SoloCtx<32, 4> behind the product's own lite_build, through both ways a lite slot is written"""
    f = IC.family(name)
    B, m, d = f["ctrs"].shape
    if route == "step_pack":
        st, arrs, status = simt.step_pack(f["ctrs"])
        kw = dict(m_max=m)
    else:
        ps, pa, mr, mn = emul.pack(f["ctrs"], nnz_cap=LC.dense_nnz(f["ctrs"]) + 64, lds_bytes=160 * 1024)
        st, arrs, status = simt.lite_from_packed(ps)
        kw = dict(lds_bytes=LC.solve_lds_bytes(d))
    assert (status == 0).all() and (arrs["hdr"][0::8] == 1).all(), (status, arrs["hdr"][0::8])
    outs = {}
    for k in IC.K_STEPS:
        for seed in SEEDS:
            o = simt.step_solve_ipm(st, f["pred"], sign=IC.SIGN, max_iter=k, seed=seed, **kw)
            IC.compare(o, name, k, "f32", False, f"simt/step_solve_ipm/{route}", IC.RECORD)
            check_scaling(o, name, f"simt/step_solve_ipm/{route}", k)
            if seed:
                same_bits(o, outs[k], (name, k, "schedule"))
            outs[k] = o
    same_bits(simt.step_solve_ipm(st, f["pred"], sign=IC.SIGN, max_iter=0, **kw), outs[3], (name, "max_iter = 0 means 3"))


# ---------------------------------------------------------------------------------------------- (b): the double state
STATE_FAMILIES = {"ipm_iter": IC.SMALL, "ipm_lite": IC.PM1_ONLY}


def run_state(simt, name, op, ctx, tier, seeds=SEEDS, rcp=False):
    lite = op == "ipm_lite"
    rows = IC.state_rows(name, lite)
    for k in IC.STATE_STEPS:
        cases, pm1 = IC.state_cases(name, k, rows)
        prev = None
        for seed in seeds:
            outs = simt.op_run(op, ctx, pm1, cases, seed=seed)
            IC.compare_state(outs, name, k, rows, ctx == "b4", f"{tier}/{op}/{ctx}", IC.RECORD, lite=lite, rcp=rcp)
            if prev is not None and ctx != "w1":   # fixed-point sums / one wave in lane order: the schedule changes no bit
                for a, b in zip(outs, prev):
                    assert np.array_equal(a["out"], b["out"]), (name, k, op, ctx, "schedule")
            prev = outs


@pytest.mark.parametrize("op,ctx,name", [(op, ctx, n) for op, ctx in IC.STATE_KINDS for n in STATE_FAMILIES[op]])
def test_double_state_of_the_solver_alone(simt, op, ctx, name):
    """(b): rho, theta and z of the bound rows and M^T theta in double after 1, 2, 3 steps, within E_k -- no float32
    term, so the rounding of rho' to float (1.7e-8) is in reach: test_the_weights_switch_is_visible... shows that the
    other setting of the switch lies more than 4 E_k away"""
    run_state(simt, name, op, ctx, "simt")


@pytest.fixture(scope="module")
def simt_rcp24():
    """the emulation with reciprocals and square roots accurate to 2^-24 before their Newton steps, as v_rcp_f64 /
    v_rsq_f64 are on the device (the emulation otherwise divides exactly)"""
    from emul_lib import Simt

    return Simt(defines=("SIMT_APPROX_RCP",), tag="_rcp24_ops", ops=True)


@pytest.mark.parametrize("op,ctx", IC.STATE_KINDS)
def test_double_state_with_approximate_reciprocals(simt_rcp24, op, ctx):
    """(b) once more in the SIMT_APPROX_RCP build, on the fixtures and the constructed cones; its margin is recorded
    under its own tier"""
    for name in ("tsp20", "sp5", "built") + (() if op == "ipm_lite" else ("generic",)):
        run_state(simt_rcp24, name, op, ctx, "rcp24", seeds=(0,), rcp=ctx != "b4")   # one wave: a register Gauss-Jordan


def test_interior_point_entries_are_asan_ubsan_clean(tmp_path):
    """the constructed cones and the limit shapes through the three entries compiled with -fsanitize=address,undefined
    into a program of its own (tests/emul/ipm_asan_main.cpp; the workgroup's LDS, the case blob and the outputs are
    exact-size heap blocks there: an overrun of any array is a finding), one shuffled lane schedule; the results are
    held to the same bound.  Nothing is loaded into Python under a sanitizer."""
    from emul_ipm_asan import AsanRunner

    runner = AsanRunner(str(tmp_path))
    for op, ctx in IC.STATE_KINDS:
        lite = op == "ipm_lite"
        for name in ("built",) + tuple(n for n in IC.SMALL if n.startswith("limit/")):
            rows = IC.state_rows(name, lite)
            cases, pm1 = IC.state_cases(name, 3, rows)
            outs = runner.op_run(op, ctx, pm1, cases, seed=24)
            IC.compare_state(outs, name, 3, rows, ctx == "b4", f"asan/{op}/{ctx}", None, lite=lite)


# ------------------------------------------------------------------------------------------------- (c): on the floor
def floor_runs(emul, simt, name, ctrs, pred, k):
    """entry -> (run, weights), grouped by the build that carries it"""
    serial = {"serial/cone_dense": (lambda: emul.cone_dense(ctrs, pred, IC.MODE_IPM, sign=IC.SIGN, max_iter=k), "f32"),
              "serial/cone_dense_large": (lambda: emul.cone_dense_large(ctrs, pred, IC.MODE_IPM, sign=IC.SIGN, max_iter=k), "f64")}
    if simt is None:
        return serial
    runs = {"simt/cone_dense/w1": (lambda: simt.cone_dense(ctrs, pred, IC.MODE_IPM, sign=IC.SIGN, max_iter=k, waves=1), "f32"),
            "simt/cone_dense/w4": (lambda: simt.cone_dense(ctrs, pred, IC.MODE_IPM, sign=IC.SIGN, max_iter=k, waves=4), "f32")}
    if name in IC.PM1_ONLY:
        st, arrs, status = simt.step_pack(ctrs)
        assert (status == 0).all()
        # (the store struct points into `arrs`: the closure keeps them alive)
        runs["simt/step_solve_ipm"] = (lambda keep=arrs: simt.step_solve_ipm(st, pred, sign=IC.SIGN, max_iter=k, m_max=ctrs.shape[1]), "f32")
    return runs


def check_floor(runs, name, rows, k):
    for what, (run, weights) in runs.items():
        o = run()
        assert (o["status"] == 0).all() and (o["iters"] == k).all(), what
        for j, b in enumerate(rows):
            ref = IC.reference(name, int(b), weights, k)[1][k]
            err = float(np.abs(o["proj"][j] - I.L._f64(ref["proj"])).max()) / (TOL * IC.scale_of(name, int(b)))
            key = f"{what}|{name}|k={k} (error / TOL sc)"
            IC.RECORD[key] = max(IC.RECORD.get(key, 0.0), err)
            assert err <= 1.0, (what, name, int(b), err)


@pytest.mark.parametrize("build", ["serial", "simt"])
@pytest.mark.parametrize("name", list(IC.FLOOR_ROWS))
def test_floor_of_tau_at_24_steps(emul, request, name, build):
    """(c): at 24 steps tau sits on max(1e-14 ymax^2, 1e-300) (asserted from the reference above).  A floor of 1e-10
    moves the iterate by sqrt(tau) ~ 1e-5 ymax where a coordinate with a unit row has no residual -- the predictions
    inside the cone: 12 TOL sc on tsp20, 6 on sp5; on the Gaussian ones it moves it by tau / |s| only, which no float
    sees --; the linear systems are ill conditioned by then, so the bound is golden_cases.TOL and not E_k."""
    f = IC.family(name)
    rows = np.array(IC.FLOOR_ROWS[name])
    simt = request.getfixturevalue("simt") if build == "simt" else None
    check_floor(floor_runs(emul, simt, name, f["ctrs"][rows], f["pred"][rows], IC.K_FLOOR), name, rows, IC.K_FLOOR)
