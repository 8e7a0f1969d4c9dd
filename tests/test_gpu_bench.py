"""bench.py at N = 1 as the driver runs it: a plain run prints the headline line alone, `--dump-outputs` writes what the last timed
step returned, and the same arguments give the same outputs from run to run, with or without `--full`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_BYTES_MAX = 64 * 1024 * 1024


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SONAR_BENCH_FORCE_DIST")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--prewarm", "0", *args],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _load(path):
    names = sorted(f for f in os.listdir(path) if f.endswith(".npy"))
    return {f: np.load(os.path.join(path, f), allow_pickle=False) for f in names}


def test_plain_run_dumps_the_same_outputs_every_time(tmp_path):
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    out = _bench("--dump-outputs", str(a))
    assert out["metric"] == "noise-latents/sec (SDXL 4x128x128)" and out["unit"] == "latents/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["steps"] == 4 and out["warmup"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert "extra" not in out and "cpu_baseline" not in out and "kernels" not in out["roofline"]  # --full only
    got = _load(a)
    assert set(got) == {"noise_sample.npy", "noise_sample_index.npy", "noise_latent_stats.npy"}
    assert sum(os.path.getsize(a / f) for f in got) <= DUMP_BYTES_MAX
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    sample, index, stats = got["noise_sample.npy"], got["noise_sample_index.npy"], got["noise_latent_stats.npy"]
    assert sample.shape == (64, 4, 128, 128) and index.shape == (64,) and stats.shape == (512, 2)
    assert np.all(np.isfinite(sample)) and np.all(np.diff(index) > 0) and 0 <= index[0] and index[-1] < 512
    # the sampled latents are the batch's: their own statistics are the ones written for them (normalised noise: unit std overall)
    flat = sample.reshape(64, -1).astype(np.float64)
    np.testing.assert_allclose(flat.mean(1), stats[index.astype(np.int64), 0], atol=1e-6)
    np.testing.assert_allclose(flat.std(1, ddof=1), stats[index.astype(np.int64), 1], rtol=1e-6)
    assert abs(np.sqrt((stats[:, 1] ** 2).mean()) - 1.0) < 1e-2
    # the same arguments: the same outputs, bit for bit; --full measures more after the timed steps but computes the same ones
    _bench("--dump-outputs", str(b))
    full = _bench("--dump-outputs", str(c), "--full", "--no-extra", "--no-cpu-baseline")
    assert "extra" not in full and "cpu_baseline" not in full
    for other in (b, c):
        again = _load(other)
        assert set(again) == set(got)
        for name, v in got.items():
            assert np.array_equal(v, again[name]), f"{other.name}/{name} differs from the first run"
