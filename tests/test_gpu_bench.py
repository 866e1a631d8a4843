"""bench.py on the GPU, at config 1 (one 128^3 volume, 1280x720: a few seconds): a plain run measures the
headline figure only, --full adds the CPU baseline, and --dump-outputs writes the last timed frame's image,
identical from run to run with the same arguments."""
from __future__ import annotations

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--config", "1", "--steps", "3", "--warmup", "1"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """A plain run and a --full run of the same arguments, side by side: (record, image) of each."""
    tmp = tmp_path_factory.mktemp("bench")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    procs = {}
    for tag, extra in (("plain", []), ("full", ["--full", "--cpu-budget", "0.5"])):
        cmd = [sys.executable, str(ROOT / "bench.py"), *ARGS, "--dump-outputs", str(tmp / tag), *extra]
        procs[tag] = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    out = {}
    for tag, p in procs.items():
        stdout, stderr = p.communicate(timeout=240)
        assert p.returncode == 0, (stdout + stderr)[-4000:]
        lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, stdout
        assert sorted(f.name for f in (tmp / tag).iterdir()) == ["image.npy"]
        out[tag] = (json.loads(lines[0]), np.load(tmp / tag / "image.npy"))
    return out


def test_result_line(runs):
    for rec, _ in runs.values():
        assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
        assert rec["unit"] == "frames/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["metric"].startswith("frames/sec @1280x720")
        assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] - 1000.0) < 1e-6 * 1000.0


def test_cpu_baseline_only_with_full(runs):
    assert runs["plain"][0]["cpu_baseline"] is None
    cpu = runs["full"][0]["cpu_baseline"]
    assert cpu is not None and cpu["value"] > 0 and cpu["unit"] == "frames/s"


def test_dumped_image(runs):
    a, b = runs["plain"][1], runs["full"][1]
    assert a.dtype == np.float32 and a.shape == (720, 1280, 4)
    assert a.min() >= 0.0 and a.max() <= 255.0 and np.array_equal(a, np.round(a))
    assert np.count_nonzero(a[..., 3]) > 1000   # the volume covers part of the screen
    assert np.array_equal(a, b)   # same arguments, same inputs: the same frame, bit for bit
