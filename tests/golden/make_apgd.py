#!/usr/bin/env python
"""Generate tests/golden/apgd.npz by running the REFERENCE'S OWN `project_apgd` (src/qpsolver.py:11-110, unmodified,
imported by path) eagerly on the CPU (TORCHDYNAMO_DISABLE=1 makes its @torch.compile a no-op).

Run from the repo root:   python tests/golden/make_apgd.py
Needs /root/reference (read-only); the fixture it writes is committed, and tests only read that.  Inputs are regenerated
from seeds (tests/apgd_cases.py fixture_inputs) and not stored.

Per input and per max_iters in {1, 2, 3, 20, 200, 400}, tol_grad=None:
    <name>_<k>_ref32_proj / _ref32_rn   the reference as shipped, in fp32 (rn: its SQUARED residual)
    <name>_<k>_ref64_proj / _ref64_rn   the same program with the inputs cast to double
    <name>_<k>_ld_proj / _ld_rnorm (un-squared) / _ld_loss / _ld_pgrad / _ld_gscale
                                        the long-double restatement (tests/apgd_ref.py), rounded to double
    <name>_<k>_S                        the spread of its three double twins (asserted <= 1e-12)
One converged record (`conv_*`: sp_batch(5, 5, 8, seed=0), tol_grad=1e-4, default cap): chunk count, the check quantity
the reference read after each chunk (fp32 and fp64 run), the final proj / squared rnorm, and the restatement at the
iteration count it stopped at.  Asserted: both runs stop after the same number of chunks, and every fp64 check quantity is
at least 10 % away from tol_grad.
"""

from __future__ import annotations

import importlib.util
import os
import sys

os.environ["TORCHDYNAMO_DISABLE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import apgd_cases as AC  # noqa: E402
import apgd_ref as R  # noqa: E402

S_MAX = 1e-12


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_qpsolver", os.path.join(REF, "src", "qpsolver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def store_restatement(out, tag, ref, S):
    assert S <= S_MAX, (tag, S)
    out[f"{tag}_ld_proj"] = ref.proj.astype(np.float64)
    out[f"{tag}_ld_rnorm"] = ref.rnorm.astype(np.float64)
    out[f"{tag}_ld_loss"] = ref.loss.astype(np.float64)
    out[f"{tag}_ld_pgrad"] = ref.pgrad.astype(np.float64)
    out[f"{tag}_ld_gscale"] = ref.gscale
    out[f"{tag}_S"] = np.float64(S)


def main():
    ref_mod = load_reference()
    out = {}
    for name, (A, y, sign) in AC.fixture_inputs().items():
        signed = sign * y
        for k in AC.SNAP:
            for dt, tag in ((torch.float32, "ref32"), (torch.float64, "ref64")):
                proj, rn = ref_mod.project_apgd(torch.tensor(A, dtype=dt), torch.tensor(signed, dtype=dt), tol_grad=None, max_iters=k)
                out[f"{name}_{k}_{tag}_proj"], out[f"{name}_{k}_{tag}_rn"] = proj.numpy(), rn.numpy()
        ld = R.run(A, y, sign, max(AC.SNAP), 8, snaps=AC.SNAP)
        tw = R.twins(A, y, sign, max(AC.SNAP), 8, snaps=AC.SNAP)
        for k in AC.SNAP:
            S = R.spread(ld.snaps[k], [t.snaps[k] for t in tw])
            store_restatement(out, f"{name}_{k}", ld.snaps[k], S)
            dev = np.abs(out[f"{name}_{k}_ref64_proj"] - out[f"{name}_{k}_ld_proj"]).max() / max(np.abs(out[f"{name}_{k}_ld_proj"]).max(), 1e-300)
            print(f"{name:6s} k={k:3d}  S {S:.2e}  ref64 vs restatement {dev:.2e}  "
                  f"ref32 vs ref64 {np.abs(out[f'{name}_{k}_ref32_proj'] - out[f'{name}_{k}_ref64_proj']).max():.2e}", flush=True)
    assert not out["setup_400_ref64_proj"].any() and not out["setup_400_ld_proj"].any()  # the zero projection

    # ---- the converged record: the values the reference's own loop reads (its only .item() call, src/qpsolver.py:57)
    A, y, sign = AC.converged_input()
    item = torch.Tensor.item
    for dt, tag in ((torch.float32, "ref32"), (torch.float64, "ref64")):
        seen = []
        torch.Tensor.item = lambda self, _item=item, _seen=seen: (_seen.append(float(_item(self))), _item(self))[1]
        try:
            proj, rn = ref_mod.project_apgd(torch.tensor(A, dtype=dt), torch.tensor(sign * y, dtype=dt))
        finally:
            torch.Tensor.item = item
        out[f"conv_{tag}_pgrad"], out[f"conv_{tag}_proj"], out[f"conv_{tag}_rn"] = np.asarray(seen), proj.numpy(), rn.numpy()
        print("converged record", tag, seen)
    assert len(out["conv_ref32_pgrad"]) == len(out["conv_ref64_pgrad"])
    assert (np.abs(out["conv_ref64_pgrad"] - 1e-4) >= 1e-5).all(), out["conv_ref64_pgrad"]
    chunks = len(out["conv_ref64_pgrad"])
    out["conv_chunks"] = np.int64(chunks)
    snaps = tuple(200 * (j + 1) for j in range(chunks))
    ld = R.run(A, y, sign, 200 * chunks, 8, snaps=snaps)
    tw = R.twins(A, y, sign, 200 * chunks, 8, snaps=snaps)
    for k in snaps:
        store_restatement(out, f"conv_{k}", ld.snaps[k], R.spread(ld.snaps[k], [t.snaps[k] for t in tw]))
    path = os.path.join(HERE, "apgd.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
