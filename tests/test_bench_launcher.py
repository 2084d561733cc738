"""CPU tier: `python bench.py --gpus N` (RANK unset) launches its own ranks, relays rank 0's single JSON
line and propagates failure.  --dry-run swaps the GPU work for a gloo rendezvous + all-reduce."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def test_self_launch_relays_one_json_line():
    p = _run("--gpus", "2", "--steps", "5", "--warmup", "1", "--dry-run")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 5 and res["dry_run"] is True
    assert res["instances_seen"] == 2 * 1024  # both ranks took part in the all-reduce


def test_self_launch_propagates_rank_failure():
    import torch

    if torch.cuda.is_available():
        import pytest

        pytest.skip("needs a box without a GPU: the ranks must fail")
    p = _run("--gpus", "2", "--steps", "1", "--warmup", "0", "--no-extras", "--cpu-sample", "0")
    assert p.returncode != 0
    assert "metric" not in p.stdout


def test_dump_outputs_keeps_a_fixed_sample_under_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy per output; over the size limit, the same seeded rows of every output."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    loss = np.arange(1000, dtype=np.float64)
    grad = np.arange(1000 * 50, dtype=np.float32).reshape(1000, 50)
    bench.dump_outputs(str(tmp_path / "all"), {"loss": loss, "grad": grad})
    assert sorted(os.listdir(tmp_path / "all")) == ["grad.npy", "loss.npy"]
    assert np.load(tmp_path / "all" / "loss.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "all" / "grad.npy"), grad)

    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 << 10)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"loss": loss, "grad": grad})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grad.npy", "loss.npy", "sample_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 10
    rows = np.load(tmp_path / "a" / "sample_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 1000 and np.array_equal(rows, np.load(tmp_path / "b" / "sample_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "grad.npy"), grad[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "loss.npy"), loss[rows].astype(np.float32))
