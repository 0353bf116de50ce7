"""bench.py's plain run and its two options: a plain `--steps N --warmup W` run prints the headline line only (no parity, other contraction path,
extras or cpu_baseline), `--dump-outputs DIR` writes what the last timed step computed, identically seeded from run to run, and `--full` still
measures the blocks the plain run leaves out.  `--size 4096` keeps each run to seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_BLOCKS = ("parity", "split_contraction", "extras", "cpu_baseline")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size", "4096", *extra], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_the_last_timed_step(dev, tmp_path):
    recs, dumps = [], []
    for tag in ("a", "b"):
        recs.append(_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / tag)))
        dumps.append(_load(tmp_path / tag))
    rec, out = recs[0], dumps[0]
    assert rec["steps"] == 2 and rec["warmup"] == 1 and len(rec["config"]["cg_iterations_all"]) == 2 and rec["ms_per_step"] > 0
    assert rec["metric"] == "exactgp_mll_kv_tflops" and rec["unit"] == "TFLOP/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert not any(k in rec for k in FULL_BLOCKS), sorted(rec)
    assert set(out) == {"mll", "inv_quad", "logdet", "y_solve", "probe_solves_sample", "probe_solves_sample_rows", "cg_iterations"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert out["y_solve"].shape == (1, 4096) and out["probe_solves_sample"].shape == (64, 4096)
    assert np.all(np.isfinite(out["y_solve"])) and np.all(np.isfinite(out["probe_solves_sample"]))
    # the last step's values, as the result line reports them
    assert float(out["mll"][0]) == rec["mll"] and int(out["cg_iterations"][0]) == rec["config"]["cg_iterations_all"][-1]
    n = 4096
    mll = -0.5 * (float(out["inv_quad"].sum()) + float(out["logdet"][0]) + n * np.log(2 * np.pi)) / n
    assert abs(mll - rec["mll"]) < 1e-5 * max(1.0, abs(rec["mll"]))
    # same arguments, same inputs: a second run computes the same step
    other = dumps[1]
    assert set(other) == set(out) and all(other[k].shape == out[k].shape for k in out)
    assert np.array_equal(other["probe_solves_sample_rows"], out["probe_solves_sample_rows"])
    assert abs(other["cg_iterations"][0] - out["cg_iterations"][0]) <= 1
    assert abs(recs[1]["mll"] - rec["mll"]) < 1e-4 * max(1.0, abs(rec["mll"]))


def test_full_run_keeps_the_other_blocks(dev):
    rec = _bench("--steps", "1", "--warmup", "0", "--full", "--skip-extras", "--other-steps", "1")
    assert "parity" in rec and rec["parity"]["kv_rel_err"] < rec["parity"]["tolerance"]
    assert "split_contraction" in rec and rec["split_contraction"]["steps_timed"] == 1
    assert "cpu_baseline" in rec and rec["cpu_baseline"]["value"] > 0
    assert "extras" not in rec       # (--skip-extras still applies under --full)
