"""GPU: `freerl_amd.train maddpg_att` against a golden run of the reference's own `__main__` loop of MADDPG_simple_with_tricks.py with
its default trick {'ATT': True} (tests/golden/make_att_loop_golden.py) on the in-repo SpreadEnv: same flags, same seed -> the env
actions and rewards step by step, the per-episode returns and the final checkpoint, by the rules and tolerances tests/test_gpu_loops.py
applies to its MADDPG_simple case (actions 2e-3 absolute, rewards and returns 1e-3, checkpoint digests 5e-3 / 5e-4)."""
import os

import numpy as np
import pytest
import torch

from tests.golden import synth
from tests.golden.make_att_loop_golden import FLAGS, NAME
from tests.golden.make_loop_golden import Recorder

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_training_loop_follows_the_reference(tmp_path):
    from freerl_amd import envs as E
    from freerl_amd import train
    fx = np.load(os.path.join(GOLD, NAME + ".npz"))
    assert str(fx["flags"]) == FLAGS
    argv = FLAGS.replace("--device cpu", "--device cuda").split() + ["--results_root", str(tmp_path / "results")]
    log = dict(actions=[], rewards=[])
    env = Recorder(E.SpreadEnv(int(argv[argv.index("--N") + 1]), 25), log)
    out = train.run("maddpg_att", argv, env=env, log=lambda *a: None)
    assert out["args"].trick == {"ATT": True} and out["policy"]._e.algo == 14
    acts, rews = np.stack(log["actions"]), np.stack(log["rewards"])
    assert acts.shape == fx["actions"].shape, (acts.shape, fx["actions"].shape)     # same number of env steps
    worst = float(np.max(np.abs(acts - fx["actions"])))
    assert worst < 2e-3, "env actions diverge from the reference loop: max abs diff %g" % worst
    np.testing.assert_allclose(rews, fx["rewards"], rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(out["returns"], fx["returns"], rtol=1e-3, atol=1e-3)
    files = sorted(os.listdir(out["model_dir"]))
    assert str(fx["npy_name"]) in files and str(fx["ckpt_name"]) in files, files
    assert os.path.basename(out["model_dir"]) == "MADDPG_simple_ATT_1"              # the script's make_dir: the trick's name in the folder's
    np.testing.assert_allclose(np.load(os.path.join(out["model_dir"], str(fx["npy_name"]))), fx["returns"], rtol=1e-3, atol=1e-3)
    sd = torch.load(os.path.join(out["model_dir"], str(fx["ckpt_name"])))
    for a, d in sd.items():
        synth.check_digest("ckpt/" + a, {k: v.numpy() for k, v in d.items()}, fx, 5e-3, 5e-4, NAME)


def test_defaults_are_the_scripts():
    from freerl_amd import train
    a = train.build_parser("maddpg_att").parse_args([])
    assert (a.env_name, a.N, a.seed, a.max_episodes, a.batch_size, a.actor_lr, a.critic_lr, a.gamma, a.tau, a.gauss_init_scale, a.start_steps) == \
        ("simple_spread_v3", 5, 0, 600, 256, 1e-3, 1e-3, 0.95, 0.01, 1, 500)
    assert a.trick == {"ATT": True} and not hasattr(a, "save_freq") and a.policy_name == "MADDPG_simple"
