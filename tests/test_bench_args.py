"""CPU: bench.py's argument checks and the sampling of --dump-outputs (no GPU: nothing here imports torch)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_steps_must_be_positive():
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *bad], capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 2 and "--steps must be >= 1" in p.stderr, (bad, p.stderr)


def test_dump_writes_every_group_below_the_limit(tmp_path):
    keys = np.arange(1000, dtype=np.int64) * 7
    sums = np.linspace(-1.0, 1.0, 1000)
    bench.dump_outputs(str(tmp_path), {"group_keys": keys, "sum": sums})
    assert sorted(os.listdir(tmp_path)) == ["group_keys.npy", "sum.npy"]
    k, s = np.load(tmp_path / "group_keys.npy"), np.load(tmp_path / "sum.npy")
    assert k.dtype == np.float64 and np.array_equal(k, keys.astype(np.float64))
    assert np.array_equal(s.view(np.uint64), sums.view(np.uint64))


def test_dump_samples_the_same_groups_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8000)
    G = 10_000
    arrays = {"group_keys": np.arange(G, dtype=np.int64) + 5, "count": np.arange(G, dtype=np.int64) * 3}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    total = sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a"))
    assert total <= 8000 and len(idx) == 8000 // 24 and np.all(np.diff(idx) > 0) and idx[-1] < G
    for f in ("group_keys.npy", "count.npy", "sample_index.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    assert np.array_equal(np.load(tmp_path / "a" / "group_keys.npy"), idx + 5)
    assert np.array_equal(np.load(tmp_path / "a" / "count.npy"), idx * 3)
