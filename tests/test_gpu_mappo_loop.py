"""GPU: `python -m freerl_amd.train mappo` / `ippo` on SpreadEnv against the reference scripts' own loops
(tests/golden/loop_mappo_spread.npz, loop_ippo_spread.npz; recorded by tests/golden/make_mappo_golden.py), compared the way
tests/test_gpu_loops.py compares loop_maddpg_spread: the same number of env steps, env actions within 2e-3, rewards and returns at its
tolerances, the scripts' file names, the saved actors' digests.  Three learn() calls fall inside the run (150 steps, horizon 50)."""
import os

import numpy as np
import pytest
import torch

from tests.golden import synth
from tests.golden.make_loop_golden import Recorder

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("algo", ["mappo", "ippo"])
def test_training_loop_follows_the_reference(algo, tmp_path):
    from freerl_amd import envs as E
    from freerl_amd import train
    name = "loop_%s_spread" % algo
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    argv = str(fx["flags"]).replace("--device cpu", "--device cuda").split() + ["--results_root", str(tmp_path / "results")]
    log = dict(actions=[], rewards=[])
    env = Recorder(E.SpreadEnv(int(argv[argv.index("--N") + 1]), 25), log)
    out = train.run(algo, argv, env=env, log=lambda *a: None)
    acts, rews = np.stack(log["actions"]), np.stack(log["rewards"])
    assert acts.shape == fx["actions"].shape, (acts.shape, fx["actions"].shape)     # same number of env steps
    assert out["steps"] == 150 and out["args"].policy_name == algo.upper() and all(v == (k not in ("reward_norm", "lr_decay")) for k, v in out["args"].trick.items())
    worst = float(np.max(np.abs(acts - fx["actions"])))
    print("%s: max |env action - reference| %.3g" % (name, worst))
    assert worst < 2e-3, "env actions diverge from the reference loop: max abs diff %g" % worst
    np.testing.assert_allclose(rews, fx["rewards"], rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(out["returns"], fx["returns"], rtol=1e-3, atol=1e-3)
    files = sorted(os.listdir(out["model_dir"]))
    assert str(fx["npy_name"]) in files and str(fx["ckpt_name"]) in files and "obs_norm.pkl" in files, files
    assert os.path.basename(out["model_dir"]) == algo.upper() + "_1"
    np.testing.assert_allclose(np.load(os.path.join(out["model_dir"], str(fx["npy_name"]))), fx["returns"], rtol=1e-3, atol=1e-3)
    sd = torch.load(os.path.join(out["model_dir"], str(fx["ckpt_name"])))
    for a, d in sd.items():
        synth.check_digest("ckpt/" + a, {k: v.numpy() for k, v in d.items()}, fx, 5e-3, 5e-4, name)


def test_mappo_lr_decay_names_the_reference_line():
    from freerl_amd.MAPPO import MAPPO
    p = MAPPO({"a": [4, 2], "b": [4, 2]}, True, 1e-3, 1e-3, 8, "cuda", hidden=32)
    with pytest.raises(NotImplementedError, match=r"MAPPO\.py:488"):
        p.lr_decay(1, 10)
    assert hasattr(p.agents["a"], "ac_optimizer") and not hasattr(p.agents["a"], "actor_optimizer")
