"""bench.py's rank-count contract, checked without a GPU: the JSON line's n_gpus must be the number of
ranks that ran, so inconsistent requests fail before any rank starts."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True,
                          text=True, timeout=120, cwd=ROOT)


def test_gpus_beyond_visible_devices_fails_before_spawning():
    import torch
    n = max(torch.cuda.device_count() + 1, 2)
    r = _run(["--gpus", str(n), "--no-cpu-baseline"], LONER_DIST_BACKEND="nccl")
    assert r.returncode != 0
    assert "GPU(s) visible" in r.stderr


def test_gpus_must_match_launcher_world_size():
    r = _run(["--gpus", "3", "--no-cpu-baseline"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0
    assert "--gpus 3 but WORLD_SIZE=2" in r.stderr


def test_dump_outputs_budget_and_sample(tmp_path, monkeypatch):
    """--dump-outputs: float32 files (float64 stays), within the byte budget over all arrays; an array that fits is
    written whole, a larger one as the same sorted sample on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1000 * 1000)
    arrays = {"small": torch.arange(10, dtype=torch.float16), "big": torch.arange(300000, dtype=torch.float32),
              "wide": torch.arange(400000, dtype=torch.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], np.arange(10))
    assert got["big"].dtype == np.float32 and got["wide"].dtype == np.float64
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 1000 * 1000
    for n in ("big", "wide"):  # samples: values are their own indices here, so sorted and distinct
        assert 0 < got[n].size < arrays[n].numel() and np.all(np.diff(got[n]) > 0)
        assert np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy")))


def test_single_gpu_configs_refuse_multiple_ranks():
    r = _run(["--config", "C3", "--no-cpu-baseline"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0
    assert "single-GPU bench" in r.stderr
