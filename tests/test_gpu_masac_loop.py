"""GPU: `freerl_amd.train masac` against a golden run of the reference's own `__main__` loop of MAAC_file/MASAC.py
(tests/golden/make_masac_loop_golden.py) on the in-repo SpreadEnv: same flags, same seed -> the env actions and rewards step by step,
and the final checkpoint, by the rules and tolerances tests/test_gpu_loops.py applies to its MADDPG_simple case (actions 2e-3 absolute,
rewards 1e-3, checkpoint digests 5e-3 / 5e-4).  The script keeps the return of every 100th episode only, so in these 6 episodes its
returns array is empty ([3, 0]): its shape and file name are held, the per-episode sums are covered by the step-by-step rewards."""
import os

import numpy as np
import pytest
import torch

from tests.golden import synth
from tests.golden.make_loop_golden import Recorder
from tests.golden.make_masac_loop_golden import FLAGS, NAME, seeded_spread_env

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_training_loop_follows_the_reference(tmp_path):
    from freerl_amd import envs as E
    from freerl_amd import train
    fx = np.load(os.path.join(GOLD, NAME + ".npz"))
    assert str(fx["flags"]) == FLAGS
    argv = FLAGS.replace("--device cpu", "--device cuda").split() + ["--results_root", str(tmp_path / "results")]
    log = dict(actions=[], rewards=[])
    with seeded_spread_env():      # (the script never seeds its env: the recording and this run start the stand-in's generator alike)
        env = Recorder(E.SpreadEnv(int(argv[argv.index("--N") + 1]), 25), log)
    out = train.run("masac", argv, env=env, log=lambda *a: None)
    assert out["policy"]._e.algo == 15 and out["steps"] == 150
    acts, rews = np.stack(log["actions"]), np.stack(log["rewards"])
    assert acts.shape == fx["actions"].shape, (acts.shape, fx["actions"].shape)     # same number of env steps
    worst = float(np.max(np.abs(acts - fx["actions"])))
    print("env actions: max abs diff from the reference loop %g over %d steps" % (worst, len(acts)))
    assert worst < 2e-3, "env actions diverge from the reference loop: max abs diff %g" % worst
    np.testing.assert_allclose(rews, fx["rewards"], rtol=1e-3, atol=2e-3)
    assert out["returns"].shape == fx["returns"].shape == (3, 0)        # (nothing to compare element by element: see above)
    files = sorted(os.listdir(out["model_dir"]))
    assert str(fx["npy_name"]) in files and str(fx["ckpt_name"]) == "MASAC.pth" and "MASAC.pth" in files, files
    assert os.path.basename(out["model_dir"]) == "MASAC_1"
    sd = torch.load(os.path.join(out["model_dir"], "MASAC.pth"))
    for a, d in sd.items():
        synth.check_digest("ckpt/" + a, {k: v.numpy() for k, v in d.items()}, fx, 5e-3, 5e-4, NAME)


def test_defaults_are_the_scripts():
    from freerl_amd import train
    a = train.build_parser("masac").parse_args([])
    assert (a.env_name, a.N, a.seed, a.max_episodes, a.save_freq, a.start_steps, a.random_steps, a.learn_steps_interval, a.batch_size, a.buffer_size) == \
        ("simple_spread_v3", None, 100, 40000, 150, 500, 0, 1, 256, int(1e6))
    assert (a.actor_lr, a.critic_lr, a.gamma, a.tau, a.policy_name, a.trick, a.device) == (1e-4, 1e-4, 0.95, 0.01, "MASAC", None, "cpu")
