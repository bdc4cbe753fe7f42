"""GPU: freerl_amd.PPO2.PPO (GAIL_file/PPO2.py's class surface on kernels_gail_ppo.hip) and GAIL.train, against the reference's records in
tests/golden/gail_ppo.npz: the seeded default init and state_dict keys, PPO_learn from torch's own randperm stream, and one GAIL.train on
the in-repo PendulumShort-v1 followed step by step.  Tolerances are tests/test_gpu_gail_ppo.py's (tests/test_gpu_ppo_edges.py's)."""
import os

import numpy as np
import pytest
import torch

from tests import gail_ppo_oracle as go
from tests.golden import synth

pytestmark = pytest.mark.gpu

ACTOR_TOL = dict(rtol=2e-4, atol=5e-6)
CRITIC_TOL = dict(rtol=2e-4)
PARAM_TOL = dict(rtol=2e-3, atol=2e-5)
ADV_TOL = dict(rtol=1e-4, atol=1e-5)
KEYS_P = ["log_std"] + [n + s for n in go.NAMES for s in (".weight", ".bias")]
KEYS_V = [n + s for n in go.NAMES for s in (".weight", ".bias")]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gail_ppo.npz"))


def _sd(net):
    return {k: v.numpy() for k, v in net.state_dict().items()}


def test_state_dict_keys_init_and_round_trip(fx, tmp_path):
    from freerl_amd.PPO2 import PPO
    c = dict(go.BY_NAME["leaky-3-1"], name="class")
    ppo = PPO(go.config(c))
    assert list(ppo.P.state_dict().keys()) == KEYS_P and list(ppo.V.state_dict().keys()) == KEYS_V
    assert ppo.P.state_dict()["log_std"].shape == (1, 1) and (ppo.P.state_dict()["log_std"] == 0).all()
    # torch's generator in the reference's construction order, P then V: bit for bit the reference's init
    synth.check_digest("class/init_actor", _sd(ppo.P), fx, 0, 0, "init")
    synth.check_digest("class/init_critic", _sd(ppo.V), fx, 0, 0, "init")
    assert [g["lr"] for g in ppo.optim.param_groups] == [go.HYPER["p_lr"], go.HYPER["v_lr"]] and ppo.optim.param_groups[0]["betas"] == (0.9, 0.999)
    # checkpoint round trip with the reference's keys
    ppo.config["log_dir"] = str(tmp_path)
    ppo.save_model(name="x", iteration=3)
    ck = torch.load(str(tmp_path / "model_x.pth"), weights_only=False)
    assert {"iteration", "P_state_dict", "V_state_dict", "optim_state_dict", "cpu_rng_state", "numpy_rng_state"} <= set(ck)
    other = PPO(dict(go.config(c), seed=99))
    assert not torch.equal(other.P.state_dict()["backbone.0.weight"], ppo.P.state_dict()["backbone.0.weight"])
    assert other.load_model(str(tmp_path / "model_x.pth")) == 3
    for a, b in ((other.P, ppo.P), (other.V, ppo.V)):
        for k, v in a.state_dict().items():
            assert torch.equal(v, b.state_dict()[k]), k
    probe = torch.as_tensor(go.inputs(go.BY_NAME["leaky-3-1"])["probe"])
    assert torch.equal(other.pi(probe, return_mean=True), ppo.pi(probe, return_mean=True)) and torch.equal(other.value(probe), ppo.value(probe))
    assert ppo.value(probe).shape == (len(probe), 1) and ppo.pi(probe[0], return_mean=True).shape == (1,)
    d = ppo.pi(probe, return_dist=True)
    assert torch.allclose(d.mean, ppo.pi(probe, return_mean=True)) and torch.allclose(d.stddev, torch.ones_like(d.mean))


def test_ppo_learn_from_torchs_own_randperm_stream(fx):
    from freerl_amd.PPO2 import PPO
    base = go.BY_NAME["leaky-3-1"]
    c = dict(base, name="class")
    tab = go.inputs(base)["table"]
    ppo = PPO(go.config(c))
    batch = dict(states=torch.as_tensor(tab["states"]), actions=torch.as_tensor(tab["actions"]), rewards=torch.as_tensor(tab["rewards"]),
                 masks_2=torch.as_tensor(1.0 - tab["done"]))
    torch.manual_seed(c["seed"] + 1)
    state = torch.get_rng_state()
    traces, returns = [], []
    for call in range(c["calls"]):
        ppo.PPO_learn(batch, torch.tensor(np.float32(c["last_value"])))
        traces.append(ppo.last_learn["trace"][0])
        returns.append(ppo.last_learn["returns"][0])
    # the draws the class consumed are the reference's recorded ones
    torch.set_rng_state(state)
    drawn = np.stack([torch.randperm(c["T"]).numpy() for _ in range(c["calls"] * c["K"])]).reshape(c["calls"], c["K"], c["T"])
    np.testing.assert_array_equal(drawn, fx["class/perms"])
    trace = np.concatenate(traces)
    np.testing.assert_allclose(np.stack(returns), fx["class/returns"], **ADV_TOL)
    np.testing.assert_allclose(trace[:, 0], fx["class/actor_losses"], **ACTOR_TOL)
    np.testing.assert_allclose(trace[:, 1], fx["class/critic_losses"], **CRITIC_TOL)
    synth.check_digest("class/actor", _sd(ppo.P), fx, PARAM_TOL["rtol"], PARAM_TOL["atol"], "class")
    synth.check_digest("class/critic", _sd(ppo.V), fx, PARAM_TOL["rtol"], PARAM_TOL["atol"], "class")
    assert ppo.optim.state_dict()["step"] == int(fx["class/step"])
    probe = go.inputs(base)["probe"]
    np.testing.assert_allclose(ppo.pi(torch.as_tensor(probe), return_mean=True).numpy(), fx["class/probe_pi"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(ppo.value(torch.as_tensor(probe)).numpy().reshape(-1), fx["class/probe_value"], rtol=1e-3, atol=1e-4)


def test_gail_train_follows_the_references_own_run(fx, tmp_path):
    from freerl_amd import envs
    from freerl_amd.GAIL import GAIL, ExpertDataset, create_expert_loader
    from freerl_amd.PPO2 import PPO, gymEnvWrapper
    t = go.TRAIN
    cfg = go.train_config(str(tmp_path / "logs"))
    states, actions = go.train_expert()
    path = str(tmp_path / "expert.npz")
    np.savez(path, states=states, actions=actions)
    gail = GAIL(cfg, ppo=PPO(cfg), max_rows=t["horizon"])
    synth.check_digest("train/init_actor", _sd(gail.ppo.P), fx, 0, 0, "init")
    synth.check_digest("train/init_critic", _sd(gail.ppo.V), fx, 0, 0, "init")
    synth.check_digest("train/init_d", _sd(gail.D_model), fx, 0, 0, "init")
    wrapper = gymEnvWrapper(envs.PendulumShortEnv(), cfg)
    loader = create_expert_loader(ExpertDataset(path), cfg)
    seen = {}
    real_learn, real_pi = gail.ppo.PPO_learn, gail.ppo.pi

    def learn(batch, last_value):
        seen["batch"] = {k: v.numpy().copy() for k, v in batch.items()}
        seen["last_value"] = float(last_value)
        real_learn(batch, last_value)
    acts = []

    def pi(s, **k):
        a = real_pi(s, **k)
        if not k:
            acts.append(a.numpy().reshape(-1).copy())
        return a
    gail.ppo.PPO_learn, gail.ppo.pi = learn, pi
    gail.train(wrapper, loader, t["episodes"])
    T = t["horizon"]
    acts = np.stack(acts)
    assert len(acts) == t["episodes"] * 40
    # the first horizon: the reference's torch.normal stream, its init, its env — actions and states exact
    np.testing.assert_allclose(acts[:T], fx["train/normal_sample"][:T], rtol=0, atol=1e-6)
    np.testing.assert_allclose(seen["batch"]["actions"], fx["train/actions"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(seen["batch"]["states"], fx["train/states"], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(seen["batch"]["masks_2"], fx["train/masks_2"])
    assert seen["batch"]["masks_2"][39] == 0 and seen["batch"]["masks_2"].sum() == T - 1          # the episode end inside the horizon
    np.testing.assert_array_equal(loader.last_indices, fx["train/expert_idx"])
    # trian_D, compute_reward, last_value and PPO_learn at the tolerances of the two engines' own tests
    np.testing.assert_allclose(gail.d_history[0], fx["train/d_tuple"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(seen["batch"]["rewards"], fx["train/gail_rewards"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(seen["last_value"], float(fx["train/last_value"]), **ADV_TOL)
    out = gail.ppo.last_learn
    np.testing.assert_allclose(out["returns"][0], fx["train/returns"][0], **ADV_TOL)
    np.testing.assert_allclose(out["trace"][0][:, 0], fx["train/actor_losses"], **ACTOR_TOL)
    np.testing.assert_allclose(out["trace"][0][:, 1], fx["train/critic_losses"], **CRITIC_TOL)
    # ... and behind it: the steps of the second episode under the updated policy, the three nets
    np.testing.assert_allclose(acts[T:], fx["train/normal_sample"][T:], rtol=1e-3, atol=1e-4)
    assert os.path.exists(os.path.join(gail.ppo.config["log_dir"], "model_final.pth")) and gail.ppo.episode_num == t["episodes"]


def test_train_without_a_policy_raises_as_before_and_discrete_is_refused():
    from freerl_amd.GAIL import GAIL
    from freerl_amd.PPO2 import PPO
    cfg = go.train_config()
    with pytest.raises(NotImplementedError, match="PPO2"):
        GAIL(cfg).train(None, None, 1)
    with pytest.raises(NotImplementedError, match=r"GAIL\(config, ppo=PPO\(config\)\)"):
        GAIL(cfg).train(None, None, 1)
    with pytest.raises(NotImplementedError, match="PPO2"):            # ... and with something that is no policy of this kind
        GAIL(cfg, ppo="not called").train(None, None, 1)
    dcfg = dict(cfg, discrete=True, a_dim=2)
    with pytest.raises(ValueError, match="discrete"):
        GAIL(dcfg, ppo=PPO(dcfg)).train(None, None, 1)


def test_train_entries_run_their_loops(tmp_path):
    """`python -m freerl_amd.train gail_ppo` writes the eval_data.npz that `gail --expert` learns from."""
    import glob
    from freerl_amd import train
    small = ["--env_name", "PendulumShort-v1", "--horizon", "64", "--mini_batch_size", "16", "--K_epochs", "2", "--policy_mlp_dim", "32",
             "--results_root", str(tmp_path), "--seed", "3"]
    out = train.run("gail_ppo", small + ["--max_episodes", "4", "--eval_interval", "2"], log=lambda *a: None)
    assert len(out["returns"]) == 4 and out["steps"] == 160 and np.isfinite(out["returns"]).all()
    found = glob.glob(os.path.join(out["model_dir"], "eval_data.npz"))
    # (the two updates fall behind episodes 1 and 3: no evaluation saved a model_best.pth, train_post evaluates the final model)
    assert found and os.path.exists(os.path.join(out["model_dir"], "model_final.pth"))
    data = np.load(found[0])
    assert data["states"].shape == (400, 3) and data["actions"].shape == (400, 1) and data["index"].tolist() == [40] * 10
    out = train.run("gail", small + ["--max_episodes", "3", "--d_mlp_dim", "32", "--expert", found[0]], log=lambda *a: None)
    assert len(out["returns"]) == 3 and len(out["policy"].d_history) == 1 and np.isfinite(out["policy"].d_history[0]).all()
    assert np.isfinite(out["policy"].ppo.last_learn["trace"]).all()
    with pytest.raises(ValueError, match="--expert"):
        train.run("gail", small, log=lambda *a: None)
