#!/usr/bin/env python3
"""Golden OUTPUT vectors of envelope multi-objective DDPG (ENVELOPE_MORL_file/ENVELOPE_DDPG.py), by running the imported
reference (PyTorch CPU) on the seeded cases of tests/envelope_ddpg_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_envelope_ddpg_golden

The script imports `mo_gymnasium`, which only its training loop uses: an empty module stands in for it.  A case's nets are
`Actor(O, A, R, H, H)` and `Critic([O, A], R, H, H)` swapped in for the constructor's default width, with PCG64 parameters through
`load_state_dict`; the table goes in through `add()` (which also fills `priority_mem`), and every `learn()` draws its rows
(`np.random.choice` over the priorities) and preference vectors (`np.random.randn`) from NumPy's seeded global stream.  The
fixture records what each call drew, both losses, both pre-clip gradient norms (what `clip_grad_norm_` returns), and digests of
the four nets and Adam's moments.

There is no argmax in this algorithm, so no seed is rejected for a margin.  The class case's seed must draw the same rows when
every priority is scaled by an independent factor in [1 - 1e-4, 1 + 1e-4], as the envelope-DQN generator requires.
"""
import os
import sys
import types
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import envelope_ddpg_oracle as eo  # noqa: E402
from tests.golden import synth  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import CPU, adam_state, inject, load, t2n, wrap_losses  # noqa: E402

N_SEEDS = 48          # seeds tried for the class case


def reference():
    sys.modules.setdefault("mo_gymnasium", types.ModuleType("mo_gymnasium"))
    return import_reference("ENVELOPE_MORL_file", "ENVELOPE_DDPG")


def build(mod, c, inp, capacity):
    O, A, R, H = c["obs_dim"], c["act_dim"], c["rdim"], c["hidden"]
    pol = mod.ENVELOPE_DDPG([O, A, R], True, c["actor_lr"], c["critic_lr"], capacity, CPU, c["beta"], c.get("max_episodes", 1000))
    ag = pol.agent
    ag.actor = mod.Actor(O, A, R, H, H)
    ag.critic = mod.Critic([O, A], R, H, H)
    load(ag.actor, inp["actor"])
    load(ag.critic, inp["critic"])
    ag.actor_target, ag.critic_target = deepcopy(ag.actor), deepcopy(ag.critic)
    ag.actor_optimizer = torch.optim.Adam(ag.actor.parameters(), lr=c["actor_lr"])
    ag.critic_optimizer = torch.optim.Adam(ag.critic.parameters(), lr=c["critic_lr"])
    return pol


class Recorder:
    """What a learn() call drew — the rows (through buffer.sample) and the preference vectors (through np.random.randn) — and the
    pre-clip gradient norms clip_grad_norm_ returned: the critic's first, then the actor's."""

    def __init__(self, pol):
        self.pol, self.idx, self.weights, self.norms = pol, [], [], []
        self._sample, self._randn, self._clip = pol.buffer.sample, np.random.randn, torch.nn.utils.clip_grad_norm_

    def sample(self, indices):
        self.idx.append(np.asarray(indices, np.int64).copy())
        return self._sample(indices)

    def randn(self, *shape):
        raw = self._randn(*shape)
        self.weights.append((np.abs(raw) / np.linalg.norm(raw, ord=1, axis=1, keepdims=True)).astype(np.float32))
        return raw

    def clip(self, params, max_norm, *a, **k):
        total = self._clip(params, max_norm, *a, **k)
        self.norms.append(float(total))
        return total

    def learn(self, c):
        with inject(self.pol.buffer, "sample", self.sample), inject(np.random, "randn", self.randn), \
                inject(torch.nn.utils, "clip_grad_norm_", self.clip):
            self.pol.learn(c["batch"], c["gamma"], c["tau"], c["weight_num"], 1)


def pack_state(name, pol, out):
    ag = pol.agent
    for key, net in (("actor", ag.actor), ("critic", ag.critic), ("actor_target", ag.actor_target), ("critic_target", ag.critic_target)):
        synth.pack_digest(name + "/" + key, t2n(net.state_dict()), out)
    for key, opt, net in (("actor", ag.actor_optimizer, ag.actor), ("critic", ag.critic_optimizer, ag.critic)):
        m, v, step = adam_state(opt, net)
        synth.pack_digest(name + "/" + key + "_m", m, out)
        synth.pack_digest(name + "/" + key + "_v", v, out)
        out[name + "/" + key + "_step"] = np.int64(step)


def run_case(mod, c, seed):
    inp = eo.inputs(c, seed=seed)
    t = inp["table"]
    pol = build(mod, c, inp, len(t["done"]))
    np.random.seed(seed)
    torch.manual_seed(seed)
    for i in range(len(t["done"])):
        pol.add(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"])
    pol.beta = c["beta"]                 # the cases pin beta: the table's done rows have moved the homotopy
    losses = wrap_losses(pol.agent, ["update_critic", "update_actor"])
    rec = Recorder(pol)
    for _ in range(c["n_learn"]):
        rec.learn(c)
    return pol, rec, losses, {}


def run_class(mod, c, seed):
    """The class case (envelope_ddpg_oracle.CLASS): select_action + add per step, learn() on the schedule; -> None when a
    perturbed priority list draws other rows."""
    inp = eo.inputs(c, seed=seed)
    t = inp["table"]
    pol = build(mod, c, inp, c["capacity"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    losses = wrap_losses(pol.agent, ["update_critic", "update_actor"])
    rec = Recorder(pol)
    prefs, actions, prios, betas = [], [], [], []
    randn = torch.randn

    def torch_randn(*a, **k):
        p = randn(*a, **k)
        prefs.append((torch.abs(p) / torch.norm(p, p=1)).numpy().copy())
        return p
    learn_at = set(eo.class_schedule(c))
    pert = np.random.default_rng(seed + 7)
    with inject(torch, "randn", torch_randn):
        for i in range(c["n_steps"]):
            actions.append(np.asarray(pol.select_action(t["obs"][i]), np.float32).copy())
            pol.add(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"])
            prios.append(float(pol.priority_mem[-1]))
            betas.append(float(pol.beta))
            if i in learn_at:
                state = np.random.get_state()
                rec.learn(c)
                after = np.random.get_state()
                pm = np.array(pol.priority_mem, dtype=np.float64)
                for _ in range(32):
                    q = pm * pert.uniform(1 - 1e-4, 1 + 1e-4, pm.size)
                    np.random.set_state(state)
                    if not np.array_equal(np.random.choice(range(pm.size), c["batch"], replace=False, p=q / q.sum()), rec.idx[-1]):
                        return None
                np.random.set_state(after)
    extra = dict(pref=np.array(prefs, np.float32), action=np.array(actions, np.float32), priority=np.array(prios, np.float64),
                 beta=np.array(betas, np.float64), final_priority=np.array(pol.priority_mem, np.float64))
    return pol, rec, losses, extra


def gen():
    mod = reference()
    out = {}
    for name in list(eo.CASES) + ["class"]:
        c = eo.case(name)
        for k in range(N_SEEDS if name == "class" else 1):
            seed = c["seed"] + k
            got = run_class(mod, c, seed) if name == "class" else run_case(mod, c, seed)
            if got is not None:
                break
        else:
            raise SystemExit("%s: no seed in %d draws the same rows under perturbed priorities" % (name, N_SEEDS))
        pol, rec, losses, extra = got
        closs, aloss = np.array(losses["update_critic"], np.float32), np.array(losses["update_actor"], np.float32)
        norms = np.array(rec.norms, np.float64).reshape(c["n_learn"], 2)
        assert len(closs) == len(aloss) == c["n_learn"]
        out[name + "/seed"] = np.int64(seed)
        out[name + "/critic_loss"], out[name + "/actor_loss"] = closs, aloss
        out[name + "/critic_norm"], out[name + "/actor_norm"] = norms[:, 0], norms[:, 1]
        out[name + "/idx"] = np.stack(rec.idx)
        out[name + "/weights"] = np.stack(rec.weights)
        pack_state(name, pol, out)
        for k2, v in extra.items():
            out[name + "/" + k2] = v
        print("%-16s seed %d  critic loss %.6g .. %.6g  actor loss %.6g .. %.6g  norms %s / %s" %
              (name, seed, closs[0], closs[-1], aloss[0], aloss[-1], np.round(norms[:, 0], 3), np.round(norms[:, 1], 3)))
    np.savez_compressed(os.path.join(HERE, "envelope_ddpg.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen()
    print("wrote envelope_ddpg.npz")
