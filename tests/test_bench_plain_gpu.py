"""A plain `python bench.py --gpus 1 --steps K --warmup W` is the headline alone: set-up, W warm-up rounds, K timed rounds and
the one JSON line (metric, value, unit, higher_is_better, dtype, ms_per_step); the nested sections, rooflines, peaks and CPU
baseline belong to `--full`.  `--dump-outputs DIR` writes what the last timed round computed as float32 .npy files, and two
runs with the same arguments start from the same inputs, so they write the same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_dumps_its_outputs(tmp_path):
    dumps = [tmp_path / "a", tmp_path / "b"]
    lines = [_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)]) for d in dumps]
    d = lines[0]
    assert d["metric"] == "ppo_update_samples_per_sec" and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["config"]["workload"].startswith("C2:")
    assert d["ms_per_step"] > 0 and abs(d["value"] - 128 / (d["ms_per_step"] * 1e-3)) < 1e-2 * d["value"]
    for k in ("c3", "c2_latent_cache", "c3_latent_cache", "c2_direct_conv", "c2_stem_bf16x3", "measured_peaks", "cpu_baseline",
              "roofline", "update_roofline", "t_encode_ms"):
        assert k not in d, k
    shapes = {"losses": (8, 3), "params_sample": (1 << 22,), "features": (1, 129, 8, 530), "returns": (1, 2, 129, 1),
              "advantages": (1, 2, 128, 1)}
    out = [{n: np.load(str(dd / (n + ".npy"))) for n in shapes} for dd in dumps]
    assert sorted(p.name for p in dumps[0].iterdir()) == sorted(n + ".npy" for n in shapes)
    assert sum(a.nbytes for a in out[0].values()) <= 64 << 20
    for n, shape in shapes.items():
        a, b = out[0][n], out[1][n]
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all(), (n, a.dtype, a.shape)
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=n)
    np.testing.assert_allclose(out[0]["losses"][-1], d["last_losses"], rtol=1e-5, atol=1e-6)
