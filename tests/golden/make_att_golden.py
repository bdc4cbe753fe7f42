#!/usr/bin/env python3
"""Golden OUTPUT vectors of ATT-MADDPG (MADDPG_file/MADDPG_simple_with_tricks.py with trick['ATT'], ATT.py:181-229), by running the
imported reference (PyTorch CPU) on the seeded cases of tests/att_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_att_golden

A case's nets are `Actor(O, A, H, H)` and `ATT_critic(dim_info, hidden_dim=H)` with PCG64 parameters through `load_state_dict`;
`ATT_critic.id_num` (a class-level counter: the critic's identity) is reset before every build.  The ring of 300 rows goes in through
`add()`, every `learn()` takes its rows from `np.random.choice` (fed the oracle's PCG64 draws, recorded again in the fixture).  Per
call the fixture holds both losses and both pre-clip gradient norms (what `clip_grad_norm_` returns) per agent, and after the last
call digests of the online and target nets and of Adam's moments; for the first call also Q of the sampled rows from `critic` and
`critic_target`.  Outputs only, no program text.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import att_oracle as ao  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import CPU, adam_state, feeder, inject, load, t2n, wrap_losses  # noqa: E402

TRICK = {"ATT": True}


def ids_of(c):
    return ["agent_%d" % j for j in range(len(c["dims"]))]


def build(mod, c, inp, capacity):
    """the reference's MADDPG with the case's width and parameters"""
    ids = ids_of(c)
    dim_info = {a: list(c["dims"][j]) for j, a in enumerate(ids)}
    mod.ATT_critic.id_num = 0
    pol = mod.MADDPG(copy.deepcopy(dim_info), True, c["actor_lr"], c["critic_lr"], capacity, CPU, TRICK)
    H = c["hidden"]
    for j, a in enumerate(ids):
        ag = pol.agents[a]
        if inp is not None:
            ag.actor = mod.Actor(dim_info[a][0], dim_info[a][1], H, H)
            mod.ATT_critic.id_num = j
            ag.critic = mod.ATT_critic(dim_info, hidden_dim=H)
            load(ag.actor, inp["actor"][j])
            load(ag.critic, inp["critic"][j])
            ag.actor_optimizer = torch.optim.Adam(ag.actor.parameters(), lr=c["actor_lr"])
            ag.critic_optimizer = torch.optim.Adam(ag.critic.parameters(), lr=c["critic_lr"])
            ag.actor_target, ag.critic_target = copy.deepcopy(ag.actor), copy.deepcopy(ag.critic)
    return pol, ids


def add_row(pol, ids, t, i):
    pol.add({a: t[j]["obs"][i] for j, a in enumerate(ids)}, {a: t[j]["act"][i] for j, a in enumerate(ids)},
            {a: float(t[j]["rew"][i]) for j, a in enumerate(ids)}, {a: t[j]["next_obs"][i] for j, a in enumerate(ids)},
            {a: bool(t[j]["done"][i]) for j, a in enumerate(ids)})


class Norms:
    def __init__(self):
        self.v, self._clip = [], torch.nn.utils.clip_grad_norm_

    def clip(self, params, max_norm, *a, **k):
        total = self._clip(params, max_norm, *a, **k)
        self.v.append(float(total))
        return total


def first_q(pol, ids, t, idx0):
    q, qt = [], []
    T = lambda x: torch.as_tensor(np.asarray(x, np.float32))
    for i, a in enumerate(ids):
        rows = idx0[i]
        obs, act = [T(t[j]["obs"][rows]) for j in range(len(ids))], [T(t[j]["act"][rows]) for j in range(len(ids))]
        with torch.no_grad():
            q.append(pol.agents[a].critic(obs, act).numpy()[:, 0].copy())
            qt.append(pol.agents[a].critic_target(obs, act).numpy()[:, 0].copy())
    return np.stack(q), np.stack(qt)


def pack_net(prefix, tensors, names, out):
    out[prefix + "/stats"], out[prefix + "/sample"] = ao.compact_digest(tensors, names)


def pack_state(name, pol, ids, out):
    for j, a in enumerate(ids):
        ag = pol.agents[a]
        for key in ("actor", "critic", "actor_target", "critic_target"):
            pack_net("%s/%d/%s" % (name, j, key), t2n(getattr(ag, key).state_dict()), ao.ACTOR_NAMES if "actor" in key else ao.CRITIC_NAMES, out)
        for key, opt, net in (("actor", ag.actor_optimizer, ag.actor), ("critic", ag.critic_optimizer, ag.critic)):
            m, v, step = adam_state(opt, net)
            names = ao.ACTOR_NAMES if key == "actor" else ao.CRITIC_NAMES
            pack_net("%s/%d/%s_m" % (name, j, key), m, names, out)
            pack_net("%s/%d/%s_v" % (name, j, key), v, names, out)
            out["%s/%d/%s_step" % (name, j, key)] = np.int64(step)


def actor_clip_search(mod, n_seeds=48):
    """does some actor step of the `pair` case pass the clip at 0.5 under one of the first n_seeds seeds?  -> (seed or None, largest norm)"""
    best = 0.0
    for k in range(n_seeds):
        c = ao.case("pair")
        inp = ao.inputs(c, seed=c["seed"] + k)
        pol, ids = build(mod, c, inp, c["n_table"])
        for i in range(c["n_table"]):
            add_row(pol, ids, inp["table"], i)
        norms = Norms()
        with inject(np.random, "choice", feeder([ix for per_call in inp["idx"] for ix in per_call])), inject(torch.nn.utils, "clip_grad_norm_", norms.clip):
            for _ in range(c["n_learn"]):
                pol.learn(c["batch"], c["gamma"], c["tau"])
        an = np.array(norms.v).reshape(-1, 2)[:, 1]
        best = max(best, float(an.max()))
        if an.max() > 0.5:
            return c["seed"] + k, best
    return None, best


def run_case(mod, name, out):
    c = ao.case(name)
    inp = ao.inputs(c)
    t = inp["table"]
    pol, ids = build(mod, c, inp, c["n_table"])
    n = len(ids)
    for i in range(c["n_table"]):
        add_row(pol, ids, t, i)
    assert all(0 < x["done"].mean() < 1 for x in t), "done of both values"
    q0, qt0 = first_q(pol, ids, t, inp["idx"][0])
    # no softmax weight of the first call may underflow: the float64 oracle's scores on the same rows
    o64 = ao.make(c, inp, np.float64)
    for i in range(n):
        rows = inp["idx"][0][i]
        _, k = o64.q(o64.critic[i], i, [x[rows] for x in o64.obs], [x[rows] for x in o64.act])
        spread = float((k["s"].max(axis=1) - k["s"].min(axis=1)).max())
        assert spread < 60.0, "%s agent %d: score spread %.3g underflows a softmax weight" % (name, i, spread)
    losses = [wrap_losses(pol.agents[a], ["update_critic", "update_actor"]) for a in ids]
    norms = Norms()
    flat_idx = [ix for per_call in inp["idx"] for ix in per_call]
    with inject(np.random, "choice", feeder(flat_idx)), inject(torch.nn.utils, "clip_grad_norm_", norms.clip):
        for _ in range(c["n_learn"]):
            pol.learn(c["batch"], c["gamma"], c["tau"])
    nv = np.array(norms.v, np.float64).reshape(c["n_learn"], n, 2)
    out[name + "/idx"] = np.stack(inp["idx"])
    out[name + "/critic_loss"] = np.array([l["update_critic"] for l in losses], np.float32).T       # [calls, n]
    out[name + "/actor_loss"] = np.array([l["update_actor"] for l in losses], np.float32).T
    out[name + "/critic_norm"], out[name + "/actor_norm"] = nv[:, :, 0], nv[:, :, 1]
    out[name + "/first_q"], out[name + "/first_q_target"] = q0, qt0
    pack_state(name, pol, ids, out)
    print("%-8s critic loss %s\n         actor loss %s\n         critic norms %s\n         actor norms %s" %
          (name, np.round(out[name + "/critic_loss"][0], 4), np.round(out[name + "/actor_loss"][0], 4), np.round(nv[:, :, 0], 3).tolist(),
           np.round(nv[:, :, 1], 4).tolist()))
    return nv


def run_class(mod, out):
    """class/: the torch RNG order at construction (initial parameter digests of a 3-agent policy under torch.manual_seed), then
    select_action / add / learn for a few steps with NumPy's seeded global stream drawing the rows"""
    c = ao.case("class")
    inp = ao.inputs(c)
    t = inp["table"]
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])
    pol, ids = build(mod, c, None, c["capacity"])
    for j, a in enumerate(ids):
        for key in ("actor", "critic"):
            pack_net("class/init/%d/%s" % (j, key), t2n(getattr(pol.agents[a], key).state_dict()), ao.ACTOR_NAMES if key == "actor" else ao.CRITIC_NAMES, out)
    losses = [wrap_losses(pol.agents[a], ["update_critic", "update_actor"]) for a in ids]
    learn_at = set(ao.class_schedule(c))
    actions, drawn = [], []
    choice = np.random.choice

    def rec_choice(*a, **k):
        r = choice(*a, **k)
        drawn.append(np.asarray(r, np.int64).copy())
        return r
    with inject(np.random, "choice", rec_choice):
        for i in range(c["n_steps"]):
            act = pol.select_action({a: t[j]["obs"][i] for j, a in enumerate(ids)})
            actions.append(np.concatenate([np.asarray(act[a], np.float32) for a in ids]))
            add_row(pol, ids, t, i)
            if i in learn_at:
                pol.learn(c["batch"], c["gamma"], c["tau"])
    out["class/action"] = np.array(actions, np.float32)
    out["class/idx"] = np.array(drawn, np.int64).reshape(c["n_learn"], len(ids), c["batch"])
    out["class/critic_loss"] = np.array([l["update_critic"] for l in losses], np.float32).T
    out["class/actor_loss"] = np.array([l["update_actor"] for l in losses], np.float32).T
    pack_state("class", pol, ids, out)
    print("class    critic loss %s .. %s" % (np.round(out["class/critic_loss"][0], 4), np.round(out["class/critic_loss"][-1], 4)))


def gen():
    mod = import_reference("MADDPG_file", "MADDPG_simple_with_tricks")
    out = {}
    above = below = a_above = a_below = False
    for name in ao.CASES:
        nv = run_case(mod, name, out)
        above, below = above or bool((nv[:, :, 0] > 0.5).any()), below or bool((nv[:, :, 0] < 0.5).any())
        a_above, a_below = a_above or bool((nv[:, :, 1] > 0.5).any()), a_below or bool((nv[:, :, 1] < 0.5).any())
    assert above and below, "the critic's pre-clip norm must sit on both sides of 0.5 somewhere"
    print("critic norms on both sides of the clip: yes; actor norms above / below 0.5: %s / %s" % (a_above, a_below))
    seed, best = actor_clip_search(mod)
    print("actor step above the clip among the first 48 seeds of `pair`: %s (largest actor norm %.4g)" % (seed, best))
    run_class(mod, out)
    np.savez_compressed(os.path.join(HERE, "att_maddpg.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen()
    print("wrote att_maddpg.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "att_maddpg.npz")))
