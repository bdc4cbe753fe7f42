"""bench.py end to end on the GPU: a plain run is the headline figure alone (set up, warm up, time the steps, dump, print the
line), and --full adds the rest of the report to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARNERS = 64

# the fields of the line only --full writes
FULL_ONLY = ("env_steps_per_sec", "rollout", "single_learner_updates_per_sec", "single_learner", "roofline",
             "baseline_configs_one_learner", "roofline_dqn", "dropin_classes", "dqn_single_learner_loop", "cpu_baseline")


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--learners", str(LEARNERS)] + list(args), capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone(tmp_path):
    from freerl_amd import _native as N
    line = _bench("--dump-outputs", str(tmp_path))
    assert line["metric"] == "learner_updates_per_sec" and line["unit"] == "updates/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (4, 2, 1)
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value = learners x steps / wall-clock, ms_per_step = wall-clock / steps: the same K steps
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / LEARNERS - 1.0) < 1e-9
    assert line["config"]["learners_per_gpu"] == LEARNERS
    assert not [k for k in FULL_ONLY if k in line], line.keys()
    got = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert got == ["actor_online", "actor_target", "critic_online", "critic_target", "stats"]
    stats = np.load(tmp_path / "stats.npy")
    assert stats.shape == (LEARNERS, 1, N.FRL_STAT_COUNT) and np.all(np.isfinite(stats))


def test_full_headline_only_adds_the_engine_figures():
    """What the profiling tools run (tools/ab_bench.sh, dev_check.sh, population_sweep.sh): --full --headline-only carries the
    per-kernel times, the roofline and the rollout loop of the headline engine, and nothing of the other engines."""
    line = _bench("--full", "--headline-only")
    assert line["value"] > 0 and line["ms_per_step"] > 0
    r = line["roofline"]
    assert r["avg_launch_ms"] > 0 and 0 < r["frac"] < 1 and r["kernels"]["grad_critic"]["launches"] >= 4
    assert line["env_steps_per_sec"] > 0 and line["rollout"]["updates_per_sec_in_loop"] > 0
    for k in ("single_learner_updates_per_sec", "single_learner", "baseline_configs_one_learner", "roofline_dqn",
              "dropin_classes", "dqn_single_learner_loop", "cpu_baseline"):
        assert line[k] is None, k
