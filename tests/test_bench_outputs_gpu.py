"""GPU: what a plain `python bench.py` run prints and what `--dump-outputs DIR` writes.

A plain run times the headline steps only (the roofline, "also" and CPU-baseline legs are `--full`'s).  The dumped
outputs of the last timed step are float32 / float64 arrays within 64 MB and repeat exactly from run to run, however
many steps the time-based pre-roll happened to take: it trains on a copy of the state.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", *args], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs_repeat_whatever_the_preroll(tmp_path):
    common = ["--steps", "3", "--warmup", "1", "--batch", "512"]
    a = _bench(*common, "--preroll-ms", "0", "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*common, "--preroll-ms", "30", "--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert line["unit"] == "trials/s" and line["value"] > 0 and line["higher_is_better"] is True
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
        assert not {"also", "cpu_baseline", "roofline_hbm"} & set(line)
    assert a["preroll_steps"] == 0 and b["preroll_steps"] > 0
    assert a["final_loss"] == b["final_loss"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"features.npy", "logits.npy", "loss.npy", "params.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    feats = np.load(tmp_path / "a" / "features.npy")
    assert feats.shape == (512, 9, 64, 17) and np.isfinite(feats).all()
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")[0]) - a["final_loss"]) < 1e-5
