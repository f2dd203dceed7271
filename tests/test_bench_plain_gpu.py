"""`python bench.py --gpus 1 --steps K --warmup W` (the plain run) times the K headline steps and reports nothing that needs runs
of its own; `--dump-outputs DIR` writes what the last timed step returned, computed from seeded inputs and weights, so that two
runs (or two builds) can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    a = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == 3 and a["warmup"] == 1 and a["unit"] == "utterances/s" and a["higher_is_better"] is True
    assert a["dtype"] == "bf16" and a["ms_per_step"] > 0
    assert abs(a["value"] - 64 * 1e3 / a["ms_per_step"]) <= 1e-2 * a["value"]  # 64 utterances per step
    for key in ("sustained", "roofline", "roofline_fbank", "cfg3", "cfg5", "train_dp", "cpu_baseline"):
        assert key not in a, key  # (--full)
    b = _bench(["--steps", "2", "--warmup", "2", "--dump-outputs", str(tmp_path / "b")])
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["encoder_out.npy"]
    x, y = np.load(tmp_path / "a" / "encoder_out.npy"), np.load(tmp_path / "b" / "encoder_out.npy")
    assert x.dtype == np.float32 and x.shape == (64, 249, 256) and np.isfinite(x).all() and np.abs(x).max() > 0
    assert np.abs(x - y).max() <= 1e-3 * np.abs(x).max()
