"""bench.py on the GPU, small frames: a plain run reports the headline figure only and times exactly --steps steps; --dump-outputs writes
the last step's results as float32 / float64 .npy files that two runs with the same arguments reproduce; --full adds the extra legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--gpus", "1", "--batch", "4", "--height", "240", "--width", "320"]
EXTRA = ("roofline", "cpu_baseline", "end_to_end", "conv")


def _run(args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, BENCH] + SMALL + args, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [line for line in p.stdout.splitlines() if line.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_and_dump_outputs(tmp_path):
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _run(["--steps", "3", "--warmup", "1", "--dump-outputs", d1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line
    assert all(line[k] is None for k in EXTRA), {k: line[k] for k in EXTRA}
    out = _load(d1)
    assert set(out) == {"counts", "rows", "xy_scale", "orientation", "white", "descriptors", "pairs", "fit"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= 64 << 20
    n = len(out["rows"])
    assert out["counts"].shape == (4,) and n == min(int(out["counts"].sum()), 65536) and n > 0
    assert out["xy_scale"].shape == (n, 3) and out["descriptors"].shape == (n, 64)
    assert out["orientation"].shape == out["white"].shape == out["pairs"].shape == out["fit"].shape == (n,)
    assert (out["pairs"] >= -1).all() and (out["pairs"] >= 0).any()
    # the same arguments: the same frames, the same results
    _run(["--steps", "2", "--warmup", "0", "--dump-outputs", d2])
    again = _load(d2)
    for k, a in out.items():
        assert np.array_equal(a, again[k]), k


def test_full_run_adds_the_extra_legs():
    line = _run(["--steps", "2", "--warmup", "1", "--full", "--cpu-frames", "2"])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert all(line[k] is not None for k in EXTRA), {k: line[k] for k in EXTRA}
