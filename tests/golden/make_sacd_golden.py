#!/usr/bin/env python3
"""Golden OUTPUT vectors of discrete SAC (SAC_file/SAC_add_discrete.py), by running the imported reference (PyTorch CPU)
on the seeded cases of tests/sacd_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_sacd_golden

Driven as make_golden.py drives the other algorithms: PCG64 parameters through `load_state_dict`, the
`np.random.choice` indices injected, losses captured by wrapping `update_*`.  The reference's `learn()` branches on a
module-global `is_continue` that only its `__main__` block defines: the importer sets it (False).

Writes sac_discrete.npz (four cases x 25 calls), long_sac_discrete.npz (a 200-call loss curve) and
loop_sacd_cartpole.npz: the script's own `__main__` loop on the in-repo CartPole, run and recorded by make_loop_golden.py's
run_reference / Recorder (as the loop_* fixtures of the other scripts are), replayed by tests/test_gpu_sac_discrete.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import sacd_oracle as so  # noqa: E402
from tests.golden import synth  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_loop_golden import run_reference  # noqa: E402
from tests.golden.make_golden import CPU, adam_state, feeder, fill, inject, load, t2n, wrap_losses  # noqa: E402


def run_case(c, inp, n_learn):
    mod = import_reference("SAC_file", "SAC_add_discrete")
    mod.is_continue = False                          # the module global learn() reads (see the docstring)
    trick = {"Batch_ObsNorm": bool(c["bn"])}
    pol = mod.SAC([c["obs_dim"], c["n_act"]], False, c["actor_lr"], c["critic_lr"], len(inp["table"]["rew"]), CPU,
                  trick=trick)
    if c["hidden"] != 128:           # the reference's nets take the widths as constructor arguments (:138, :153)
        H, ag = c["hidden"], pol.agent
        ag.actor = mod.Actor_discrete_hands_on(c["obs_dim"], c["n_act"], H, H)
        ag.critic = mod.Critic_discrete_hands_on([c["obs_dim"], c["n_act"]], H, H)
        ag.actor_optimizer = torch.optim.Adam(ag.actor.parameters(), lr=c["actor_lr"])
        ag.critic_optimizer = torch.optim.Adam(ag.critic.parameters(), lr=c["critic_lr"])
        ag.actor_target = mod.Actor_discrete_hands_on(c["obs_dim"], c["n_act"], H, H)
        ag.critic_target = mod.Critic_discrete_hands_on([c["obs_dim"], c["n_act"]], H, H)
    for net, key in (("actor", "actor"), ("critic", "critic")):
        load(getattr(pol.agent, net), inp[key])
        load(getattr(pol.agent, net + "_target"), inp[key])
    fill(pol, inp["table"])
    rec = wrap_losses(pol.agent, ["update_critic", "update_actor"])
    rec_a = wrap_losses(pol.alphas, ["update_alpha"])
    alphas = []
    with inject(np.random, "choice", feeder(inp["idx"][:n_learn])):
        for _ in range(n_learn):
            pol.learn(c["batch"], c["gamma"], c["tau"])
            alphas.append(np.float32(pol.alphas.alpha.item()))
    return pol, rec, rec_a, np.array(alphas, np.float32)


def gen_cases():
    out = {}
    for name in so.CASES:
        c = so.case(name)
        pol, rec, rec_a, alphas = run_case(c, so.inputs(c), c["n_learn"])
        out[name + "/loss_critic"] = np.array(rec["update_critic"], np.float32)
        out[name + "/loss_actor"] = np.array(rec["update_actor"], np.float32)
        out[name + "/loss_alpha"] = np.array(rec_a["update_alpha"], np.float32)
        out[name + "/alpha"] = alphas
        out[name + "/target_entropy"] = np.float32(pol.alphas.target_entropy.item())
        # digests (synth.pack_digest: sums and a strided sample) keep the fixture small; the GPU test compares every element
        # against the oracle, which test_sacd_oracle.py holds to these digests
        for net in ("actor", "critic", "actor_target", "critic_target"):
            synth.pack_digest(name + "/" + net, t2n(getattr(pol.agent, net).state_dict()), out)
        for net in ("actor", "critic"):
            m, _, step = adam_state(getattr(pol.agent, net + "_optimizer"), getattr(pol.agent, net))
            synth.pack_digest(name + "/" + net + "_m", m, out)
            out["%s/%s_step" % (name, net)] = np.int64(step)
    np.savez_compressed(os.path.join(HERE, "sac_discrete.npz"), **out)


def gen_long():
    c = so.case("long")
    _, rec, rec_a, alphas = run_case(c, so.inputs(c), c["n_learn"])
    np.savez_compressed(os.path.join(HERE, "long_sac_discrete.npz"), loss_critic=np.array(rec["update_critic"], np.float32),
                        loss_actor=np.array(rec["update_actor"], np.float32),
                        loss_alpha=np.array(rec_a["update_alpha"], np.float32), alpha=alphas)


# a short run: 14 episodes, 64 random steps then Categorical draws, learn() from step 65 on (the closed loop amplifies fp32
# differences; the comparison is step by step).  Batch_ObsNorm on, as the script's default trick.
LOOP_FLAGS = ("--env_name CartPole-v1 --seed 0 --max_episodes 14 --save_freq 100 --random_steps 64 --start_steps 64 "
              "--batch_size 32 --buffer_size 2000 --device cpu")


def gen_loop():
    log, returns, sd, npy_name, ckpt_name = run_reference("SAC_file", "SAC_add_discrete", LOOP_FLAGS)
    out = {"flags": np.array(LOOP_FLAGS), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
           "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
    synth.pack_digest("ckpt", {k: v.numpy() for k, v in sd.items()}, out, full_limit=0)
    np.savez_compressed(os.path.join(HERE, "loop_sacd_cartpole.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen_cases()
    gen_long()
    gen_loop()
    print("wrote sac_discrete.npz, long_sac_discrete.npz, loop_sacd_cartpole.npz")
