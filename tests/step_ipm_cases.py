"""Inputs and the yardstick of the interior-point fused step's tests (TEST INFRASTRUCTURE; numpy only).

Both tiers -- tests/test_step_ipm_emul.py (SIMT emulation) and tests/test_gpu_step_ipm.py (MI355X) -- run the new one-wave
kernel on the inputs below and compare it with the EXISTING general kernel in the same mode on the same inputs.

What "agree" means.  The two kernels run the same iterates with sums taken in different orders, so the bounds are the
fixture tolerances of tests/golden_cases.py, per instance:
    proj / target / grad   2e-6 * max(1, |y|_inf)        rnorm   2e-6 * max(1, rnorm)        loss   2e-6
`normalised` divides a difference by that scale, so every figure below is "<= TOL".  The general kernel's own spread
between one wave and four waves per instance (floating-point sums in lane order against 64-bit fixed-point sums) is
measured the same way; where it exceeds a quarter of the bound for some input and output, that input's bound for that
output is four times the spread.  The yardstick is never the kernel under test.
"""

import json
import os

import numpy as np

import limit_cones as LC
from golden_cases import TOL

FIELDS = ("proj", "target", "grad", "rnorm", "loss")
SIGN = -1.0
# tests/limit_cones.py: d = 256 / 255 / 193, 32 rows, 8 bound rows, 1536 and 1027 non-zeros, every column full
LIMIT_NAMES = ("d256_16f8b_1536", "d256_27f5b_1536", "d255_25f6b_1056", "d193_19f8b_1027", "d64_8f8b_512", "d256_32f0b_1536")
LIMIT_SEED = 11


def limit_case(name):
    return {c.name: c for c in LC.IN_CASES}[name]


def limit_batch(name):
    """B = 6: Gaussian, Gaussian, inside the cone, ZERO, Gaussian * 1e-6, Gaussian * 1e3 (limit_cones.predictions)"""
    return LC.batch(limit_case(name), LIMIT_SEED, B=6)


def fixture_inputs(golden):
    """structured.npz: tsp20 (all 16) and sp5[:8] -> {name: (ctrs, costs)}"""
    s = golden["structured"]
    return {"tsp20": (s["tsp20_ctrs"], s["tsp20_costs"]), "sp5": (s["sp5_ctrs"][:8], s["sp5_costs"][:8])}


def edge_batch():
    """d = 40, m = 48, B = 4: [the empty cone, unit rows only (p = 0), a small cone with a ZERO prediction, the same cone
    with a Gaussian one] -> (ctrs, pred, reduced rows expected [0, 0, 13, 13])"""
    rng = np.random.default_rng(5)
    d, m = 40, 48
    ctrs = np.zeros((4, m, d), np.float32)
    for k in range(0, d, 2):   # instance 1: +-e_k on every other coordinate, nothing else
        ctrs[1, k // 2, k] = 1.0 if k % 4 == 0 else -1.0
    blk, _ = LC.cone(LC.Case("d40_small", d, 10, 3, 130), 3, 0)
    assert blk.shape[0] <= m
    ctrs[2, :blk.shape[0]] = blk
    ctrs[3, :blk.shape[0]] = blk
    pred = rng.standard_normal((4, d)).astype(np.float32)
    pred[2] = 0.0
    return ctrs, pred, np.array([0, 0, 13, 13])


def property_golden(golden):
    """What tests/test_ipm_mode.py check_ipm_properties reads, for a kernel that takes +-1 cones only: its `generic` and
    `setup` inputs (Gaussian rows) are replaced by further instances of the structured fixtures -- sp5[8:16] and
    tsp20[4:8] --, `sp5` and `tsp20` stay the instances that function picks itself."""
    s = golden["structured"]
    return {"generic": {"generic_ctrs": s["sp5_ctrs"][8:16], "generic_costs": s["sp5_costs"][8:16],
                        "setup_ctrs": s["tsp20_ctrs"][4:8], "setup_costs": s["tsp20_costs"][4:8]},
            "structured": s}


def normalised(a, b, y):
    """max over the batch of |a - b| / scale per output, the scales of the module docstring (y = sign * pred)"""
    sc = np.maximum(1.0, np.abs(y).max(axis=1))
    out = {}
    for k in ("proj", "target", "grad"):
        out[k] = float((np.abs(a[k].astype(np.float64) - b[k]).max(axis=1) / sc).max())
    rn = np.maximum(1.0, np.abs(b["rnorm"]).astype(np.float64))
    out["rnorm"] = float((np.abs(a["rnorm"].astype(np.float64) - b["rnorm"]) / rn).max())
    out["loss"] = float(np.abs(a["loss"].astype(np.float64) - b["loss"]).max())
    return out


def bounds(spread):
    """the bound per output for one input, from the general kernel's own spread on it"""
    return {k: (TOL if spread[k] <= TOL / 4 else 4 * spread[k]) for k in FIELDS}


def compare(new, ref, gen1, gen4, y, what, record=None):
    """`new` against `ref`, the existing general kernel on the same inputs (GPU tier: at one wave, i.e. `gen1` itself;
    CPU tier: its serial build); `gen1` / `gen4`: the general kernel at one wave and at four, whose difference is the
    spread.  Prints the figures, records them under `what`, then asserts."""
    diff, spread = normalised(new, ref, y), normalised(gen1, gen4, y)
    bnd = bounds(spread)
    print(f"{what}: worst {max(diff.values()):.3e} spread {max(spread.values()):.3e} " +
          " ".join(f"{k}={diff[k]:.2e}/{spread[k]:.2e}" for k in FIELDS))
    if record is not None:
        record[what] = {"worst": max(diff.values()), "spread": max(spread.values()),
                        "diff": diff, "general_1_vs_4_waves": spread, "bound": bnd}
    for k in FIELDS:
        assert np.isfinite(new[k]).all(), (what, k)
        assert diff[k] <= bnd[k], (what, k, diff[k], spread[k], bnd[k])


def write_record(record):
    """the recorded figures as JSON where CAVE_IPM_MARGINS_OUT says (tools/diag/ipm_margins.py sets it); else nothing"""
    path = os.environ.get("CAVE_IPM_MARGINS_OUT")
    if path and record:
        with open(path, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
