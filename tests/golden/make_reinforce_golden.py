#!/usr/bin/env python3
"""Golden OUTPUT vectors of REINFORCE (REINFORCE_file/REINFORCE.py), by running the imported reference (PyTorch CPU) on the
seeded cases of tests/reinforce_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_reinforce_golden

Driven as make_sacd_golden.py drives discrete SAC: PCG64 parameters through `load_state_dict`, losses captured by wrapping
`update_policy`.  The action sequence is injected: the log-prob of each given action is taken through the reference's own
net and `Categorical(probs)` and appended to `log_probs` as `select_action` would, then `add(reward, done)`.

Writes reinforce.npz (seven cases x 12 calls), long_reinforce.npz (a 150-call loss curve) and loop_reinforce_cartpole.npz:
the script's own `__main__` loop on the in-repo CartPole, run and recorded by make_loop_golden.py's run_reference /
Recorder, replayed by tests/test_gpu_reinforce.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import reinforce_oracle as ro  # noqa: E402
from tests.golden import synth  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_loop_golden import run_reference  # noqa: E402
from tests.golden.make_golden import CPU, adam_state, load, t2n, wrap_losses  # noqa: E402


def run_case(c, inp):
    mod = import_reference("REINFORCE_file", "REINFORCE")
    pol = mod.REINFORCE([c["obs_dim"], c["n_act"]], False, c["lr"], CPU)
    if c["hidden"] != 128:               # Policy_MLP takes the width as a constructor argument (:39)
        pol.agent.policy_net = mod.Policy_MLP(c["obs_dim"], c["n_act"], c["hidden"])
        pol.agent.policy_net_optimizer = torch.optim.Adam(pol.agent.policy_net.parameters(), lr=c["lr"])
    load(pol.agent.policy_net, inp["params"])
    rec = wrap_losses(pol.agent, ["update_policy"])
    logps = []
    for call in inp["calls"]:
        for t in range(len(call["rew"])):
            obs = torch.as_tensor(call["obs"][t], dtype=torch.float32).reshape(1, -1)
            dist = torch.distributions.Categorical(pol.agent.policy_net(obs))
            pol.log_probs.append(dist.log_prob(torch.tensor([int(call["act"][t])])))
            pol.add(float(call["rew"][t]), bool(call["done"][t]))
        logps.append(np.array([lp.item() for lp in pol.log_probs], np.float32))
        pol.learn(c["gamma"])
        assert pol.rewards == [] and pol.log_probs == []
    return pol, np.array(rec["update_policy"], np.float32), logps


def gen_cases():
    out = {}
    for name in ro.CASES:
        c = ro.case(name)
        pol, losses, logps = run_case(c, ro.inputs(c))
        out[name + "/loss"] = losses
        out[name + "/logp"] = np.concatenate(logps)                   # the recorded log-probs, call after call
        synth.pack_digest(name + "/policy", t2n(pol.agent.policy_net.state_dict()), out)
        m, v, step = adam_state(pol.agent.policy_net_optimizer, pol.agent.policy_net)
        synth.pack_digest(name + "/policy_m", m, out)
        synth.pack_digest(name + "/policy_v", v, out)
        out[name + "/step"] = np.int64(step)
    np.savez_compressed(os.path.join(HERE, "reinforce.npz"), **out)


def gen_long():
    c = ro.case("long")
    _, losses, _ = run_case(c, ro.inputs(c))
    np.savez_compressed(os.path.join(HERE, "long_reinforce.npz"), loss=losses)


# the script's defaults (seed 100, one learn() per episode, lr 1e-3) for 12 episodes
LOOP_FLAGS = "--env_name CartPole-v1 --seed 100 --max_episodes 12 --save_freq 5 --device cpu"


def gen_loop():
    log, returns, sd, npy_name, ckpt_name = run_reference("REINFORCE_file", "REINFORCE", LOOP_FLAGS)
    out = {"flags": np.array(LOOP_FLAGS), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
           "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
    synth.pack_digest("ckpt", {k: v.numpy() for k, v in sd.items()}, out, full_limit=0)
    np.savez_compressed(os.path.join(HERE, "loop_reinforce_cartpole.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen_cases()
    gen_long()
    gen_loop()
    print("wrote reinforce.npz, long_reinforce.npz, loop_reinforce_cartpole.npz")
