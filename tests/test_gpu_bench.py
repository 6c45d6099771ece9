"""bench.py's output contract on the GPU (the driver parses this line): one JSON line with the metric, the whole-job
value and the timing fields; with --full also the roofline and cpu_baseline objects -- through ch_step_n (the default)
and with one launch per step (--steps-per-launch 1).  A plain run reports the headline alone, and --dump-outputs writes
the last timed step's outputs, the same from run to run.  Short runs: 20 timed steps after a 50-step burn-in."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
             "vs_baseline", "dtype", "data", "config")
KEYS = HEAD_KEYS + ("roofline", "cpu_baseline")


def _run(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_head(d, envs=4096):
    assert d["metric"].startswith("env-steps/sec") and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["scaling"] == "weak"
    assert d["dtype"] == "f64" and d["vs_baseline"] is None
    # value = envs x steps / wall of the timed region
    assert abs(d["value"] - envs * 20 / (d["ms_per_step"] * 20 / 1e3)) < 1e-6 * d["value"]
    assert d["config"]["envs_per_gpu"] == envs and d["config"]["num_drones"] == 4 and d["config"]["num_cattle"] == 16


@pytest.mark.gpu
@pytest.mark.parametrize("spl", [-1, 1])
def test_bench_line_contract(spl):
    d = _run(["--full", "--steps", "20", "--warmup", "5", "--burn-in", "50", "--no-cpu-baseline", "--no-extras",
              "--steps-per-launch", str(spl)])
    for k in KEYS:
        assert k in d, k
    _check_head(d)
    assert d["cpu_baseline"] is None
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["algorithmic_bytes_per_launch"] == r["bytes_per_env_step"] * 4096
    assert ("k_step2_multi" in r["kernel"]) == (spl != 1)
    assert d["rollout_metrics"]["nan_rewards"] == 0


@pytest.mark.gpu
def test_bench_plain_line_and_dump(tmp_path):
    """Without --full: the headline fields and none of the legs that take runs of their own; --dump-outputs writes the
    last timed step's outputs as float32 / float64 .npy files, bit-identical between two runs with the same arguments
    (the default ch_step_n path at the default size; 4096 envs' outputs are 18 MB, below the 64 MB sampling limit)."""
    dumps = []
    for tag in ("a", "b"):
        out = tmp_path / tag
        d = _run(["--steps", "20", "--warmup", "5", "--burn-in", "50", "--dump-outputs", str(out)])
        for k in HEAD_KEYS:
            assert k in d, k
        _check_head(d)
        assert "k_step2_multi" in d["launch"]
        for k in ("roofline", "roofline_survey", "cpu_baseline", "host_surfaces", "terminal_obs_leg", "single_launch_leg",
                  "rollout_metrics", "rollout_end_us", "valu", "flock_roofline"):
            assert k not in d, k
        dumps.append({f: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == sorted(b) == sorted(k + ".npy" for k in (
        "obs", "reward", "terminated", "truncated", "agent_active", "reset_happened", "actions", "episode_stats"))
    assert a["obs.npy"].shape == (4096, 12, 86) and a["actions.npy"].shape == (4096, 4, 4)
    assert a["reward.npy"].shape == (4096, 1) and a["episode_stats.npy"].dtype == np.float64
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f, x in a.items():
        assert x.dtype in (np.float32, np.float64), f
        assert np.array_equal(x, b[f], equal_nan=True), f
    # the outputs of a step that ran: observations and drawn actions are populated, actions within the VEL box
    assert np.abs(a["obs.npy"]).max() > 0 and np.abs(a["actions.npy"]).max() > 0
    assert np.abs(a["actions.npy"]).max() <= 1.0
