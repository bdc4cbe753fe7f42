#!/usr/bin/env python3
"""Golden OUTPUT vectors of MAAC (MAAC_file/MAAC_discrete.py with Attention.py), by running the imported reference class (PyTorch CPU) on
the hidden-128 cases of tests/maac_oracle.py (the reference fixes its widths at 128).  Run by hand where the reference tree exists:

    python -m tests.golden.make_maac_golden

A case is `MAAC(dim_info, False, actor_lr, critic_lr, 300, cpu)` as the class builds itself — every online critic holding the ONE
`Attention` block of the default argument — with PCG64 parameters through `load_state_dict` (the shared block loaded through agent 0's
critic), the targets deep-copied afterwards as `Agent.__init__` does.  The ring of 300 rows goes in through `add()` with one-hot actions;
every `sample()` takes its rows from `np.random.choice`, and every `Categorical.sample()` its draw from `torch.multinomial`, replaced by
its own single-sample rule argmax(probs / q) with q the oracle's Exp(1) stream (`multinomial_rule` first ASSERTS, against the real
torch.multinomial and torch's generator, that this is the rule).  Per call the fixture holds both losses and both pre-clip gradient norms
(what `clip_grad_norm_` returns) per agent; after the 1st and the 3rd call digests of every online and target net and of Adam's first
moments, the critic optimisers' step counts and which tensors have Adam state.  Outputs only, no program text.

The generator ASSERTS what the cases are for (`conditions`): critic pre-clip norms on both sides of 0.5 across a case's agents, both done
values per agent, every action index stored and drawn per agent, draw 1 != draw 2 on >= 25 % of each agent's rows, attention weights that
differ by >= 0.05 on >= 10 % of the rows where there are two others (from the float64 oracle, which tests/test_maac_golden.py holds to
this recording), the 8 frozen tensors per agent bit-unchanged and without Adam state, every critic optimiser at step k for the shared
block after k calls, and each oracle switch moving a compared quantity by >= 10 x its tolerance in at least one case.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import maac_oracle as mo  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import CPU, feeder, inject, load, t2n, wrap_losses  # noqa: E402

GOLDEN_CASES = ("pair", "hetero", "spread3", "spread5")
ACTOR_KEYS = [n + s for n in mo.ACTOR_NAMES for s in (".weight", ".bias")]


def multinomial_rule():
    """torch.multinomial(p, 1, True) == argmax(p / q), q = empty_like(p).exponential_(1) from the same generator state"""
    g = np.random.default_rng(77)
    for B, A in ((5, 4), (64, 5), (17, 2), (50, 17)):
        p = torch.as_tensor(g.random((B, A)).astype(np.float32) + 0.01)
        p = p / p.sum(-1, keepdim=True)
        torch.manual_seed(1234 + B)
        st = torch.get_rng_state()
        q = torch.empty_like(p).exponential_(1)
        torch.set_rng_state(st)
        k = torch.multinomial(p, 1, True)
        assert torch.equal(k, torch.argmax(p / q, dim=-1, keepdim=True)), "torch.multinomial's single-sample rule is not argmax(p / Exp(1))"


def ids_of(c):
    return ["agent_%d" % j for j in range(len(c["dims"]))]


def build(mod, c, inp):
    ids = ids_of(c)
    dim_info = {a: list(c["dims"][j]) for j, a in enumerate(ids)}
    sys.modules["Attention"].Attention_Critic.id_num = 0       # (the class-level counter: a second MAAC in one process raises IndexError otherwise)
    pol = mod.MAAC(copy.deepcopy(dim_info), False, c["actor_lr"], c["critic_lr"], c["n_table"], CPU)
    assert pol.attention and pol.one_hot and not pol.adaptive_alpha
    block = pol.agents[ids[0]].critic.attention
    assert all(pol.agents[a].critic.attention is block for a in ids), "every online critic holds the same Attention module"
    for j, a in enumerate(ids):
        ag = pol.agents[a]
        load(ag.actor, inp["actor"][j])
        load(ag.critic, mo.critic_params(inp, j))
        assert list(ag.critic.state_dict().keys()) == mo.CRITIC_KEYS and list(ag.actor.state_dict().keys()) == ACTOR_KEYS
    for a in ids:
        ag = pol.agents[a]
        ag.actor_target, ag.critic_target = copy.deepcopy(ag.actor), copy.deepcopy(ag.critic)
        assert ag.critic_target.attention is not block
        assert abs(float(pol.alphas[a].alpha) - c["alpha"]) < 1e-7 and not pol.alphas[a].log_alpha.requires_grad
    return pol, ids


class Norms:
    def __init__(self):
        self.v, self._clip = [], torch.nn.utils.clip_grad_norm_

    def clip(self, params, max_norm, *a, **k):
        total = self._clip(params, max_norm, *a, **k)
        self.v.append(float(total))
        return total


class Draws:
    """stands in for torch.multinomial: its single-sample rule on the next injected Exp(1) block; keeps every index drawn"""

    def __init__(self, blocks):
        self.it, self.k = iter(blocks), []

    def __call__(self, probs, num_samples, replacement=False, **kw):
        assert num_samples == 1
        q = torch.as_tensor(next(self.it))
        assert tuple(q.shape) == tuple(probs.shape), (tuple(q.shape), tuple(probs.shape))
        k = torch.argmax(probs / q.to(probs.dtype), dim=-1, keepdim=True)
        self.k.append(k.reshape(-1).numpy().copy())
        return k


def adam_by_key(opt, module):
    names = {id(p): n for n, p in module.named_parameters()}
    m, steps = {}, {}
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state.get(p, None)
            if st:
                m[names[id(p)]] = st["exp_avg"].numpy().copy()
                steps[names[id(p)]] = int(st["step"])
    return m, steps


def pack_state(pre, pol, ids, out, call):
    for j, a in enumerate(ids):
        ag = pol.agents[a]
        for key in ("actor", "critic", "actor_target", "critic_target"):
            out["%s/%d/%s/stats" % (pre, j, key)], out["%s/%d/%s/sample" % (pre, j, key)] = \
                mo.digest_keys(t2n(getattr(ag, key).state_dict()), ACTOR_KEYS if "actor" in key else mo.CRITIC_KEYS)
        m, steps = adam_by_key(ag.actor_optimizer, ag.actor)
        assert sorted(m) == sorted(ACTOR_KEYS) and set(steps.values()) == {call}
        out["%s/%d/actor_m/stats" % (pre, j)], out["%s/%d/actor_m/sample" % (pre, j)] = mo.digest_keys(m, ACTOR_KEYS)
        m, steps = adam_by_key(ag.critic_optimizer, ag.critic)
        # 12 tensors with Adam state, the shared block among them at this agent's own step count; the 8 frozen ones have none
        assert sorted(m) == sorted(mo.TRAINED_KEYS), sorted(m)
        assert set(steps.values()) == {call}, steps
        out["%s/%d/critic_m/stats" % (pre, j)], out["%s/%d/critic_m/sample" % (pre, j)] = mo.digest_keys(m, mo.TRAINED_KEYS)
        out["%s/%d/critic_step" % (pre, j)] = np.int64(steps["attention.query.weight"])


def run_case(mod, name, out):
    c = mo.case(name)
    inp = mo.inputs(c)
    t = inp["table"]
    pol, ids = build(mod, c, inp)
    n, B = len(ids), c["batch"]
    for i in range(c["n_table"]):
        pol.add({a: t[j]["obs"][i] for j, a in enumerate(ids)}, {a: t[j]["act"][i] for j, a in enumerate(ids)},
                {a: float(t[j]["rew"][i]) for j, a in enumerate(ids)}, {a: t[j]["next_obs"][i] for j, a in enumerate(ids)},
                {a: bool(t[j]["done"][i]) for j, a in enumerate(ids)})
    for j, x in enumerate(t):
        assert 0 < x["done"].mean() < 1, "%s agent %d: done of both values" % (name, j)
        assert (x["act"].sum(axis=0) > 0).all(), "%s agent %d: every action index stored" % (name, j)
    frozen0 = [{k: v.copy() for k, v in t2n(pol.agents[a].critic.state_dict()).items() if k in mo.FROZEN_KEYS} for a in ids]
    losses = [wrap_losses(pol.agents[a], ["update_critic", "update_actor"]) for a in ids]
    norms = Norms()
    flat_idx = [ix for per_call in inp["idx"] for ix in per_call]
    # the reference's draw order per updating agent: n target actors, n online actors (new_action), the updating actor again
    draws = Draws([e for per_call in inp["eps"] for per_agent in per_call for e in per_agent])
    with inject(np.random, "choice", feeder(flat_idx)), inject(torch.nn.utils, "clip_grad_norm_", norms.clip), inject(torch, "multinomial", draws):
        for k in range(c["n_learn"]):
            pol.learn(B, c["gamma"], c["tau"])
            if k + 1 in mo.RECORD_AFTER:
                pack_state("%s/after%d" % (name, k + 1), pol, ids, out, k + 1)
    assert len(draws.k) == c["n_learn"] * n * (2 * n + 1), "the reference took %d draws, not 2 n + 1 per agent and call" % len(draws.k)
    try:
        next(draws.it)
        raise AssertionError("draws left over")
    except StopIteration:
        pass
    for j, a in enumerate(ids):
        now = t2n(pol.agents[a].critic.state_dict())
        for k in mo.FROZEN_KEYS:
            assert np.array_equal(now[k], frozen0[j][k]), "%s agent %d: %s moved" % (name, j, k)
    # what was drawn: [call][updating agent][set] -> indices [B]
    dk = [[[draws.k[(k * n + i) * (2 * n + 1) + s] for s in range(2 * n + 1)] for i in range(n)] for k in range(c["n_learn"])]
    for j in range(n):
        A = c["dims"][j][1]
        seen = np.concatenate([dk[k][i][s] for k in range(c["n_learn"]) for i in range(n) for s in (j, n + j)] + [dk[k][j][2 * n] for k in range(c["n_learn"])])
        assert set(seen.tolist()) == set(range(A)), "%s agent %d: drawn only %s of %d actions" % (name, j, sorted(set(seen.tolist())), A)
        differ = float(np.mean([np.mean(dk[k][j][n + j] != dk[k][j][2 * n]) for k in range(c["n_learn"])]))
        assert differ >= 0.25, "%s agent %d: draw 1 != draw 2 on only %.0f %% of its rows" % (name, j, 100 * differ)
    nv = np.array(norms.v, np.float64).reshape(c["n_learn"], n, 2)
    assert (nv[:, :, 0] > 0.5).any() and (nv[:, :, 0] < 0.5).any(), "%s: critic pre-clip norms on one side of 0.5 only: %s" % (name, nv[:, :, 0])
    am = max(a for _, a in c["dims"])
    out[name + "/idx"] = np.stack(inp["idx"])
    out[name + "/eps"] = np.stack([mo.pad_eps(inp["eps"][k], n, B, am) for k in range(c["n_learn"])])
    out[name + "/critic_loss"] = np.array([l["update_critic"] for l in losses], np.float32).T       # [calls, n]
    out[name + "/actor_loss"] = np.array([l["update_actor"] for l in losses], np.float32).T
    out[name + "/critic_norm"], out[name + "/actor_norm"] = nv[:, :, 0], nv[:, :, 1]
    print("%-8s critic loss %s\n         actor loss %s\n         critic norms %s\n         actor norms %s" %
          (name, np.round(out[name + "/critic_loss"][0], 4), np.round(out[name + "/actor_loss"][0], 4), np.round(nv[:, :, 0], 3).tolist(),
           np.round(nv[:, :, 1], 4).tolist()))


def conditions():
    """what only the oracle can show: the attention's spread, and that the switches matter"""
    for name in GOLDEN_CASES:
        c = mo.case(name)
        if len(c["dims"]) < 3:
            continue
        inp = mo.inputs(c)
        o = mo.make(c, inp, np.float64)
        outs = [o.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"]) for k in range(c["n_learn"])]
        sp = np.array([x["att_spread"] for x in outs]).mean(axis=0)
        assert (sp >= 0.10).all(), "%s: attention weights differ by >= 0.05 on only %s of the rows" % (name, sp)
        print("%-8s attention weights differ by >= 0.05 on %s of each agent's rows" % (name, np.round(sp, 2).tolist()))
    for sw in ("own_attention", "final_attention", "one_draw", "stale_actors", "detach_probs"):
        best = max(mo.switch_gap(name, sw) for name in GOLDEN_CASES)
        print("%-16s moves a compared quantity by %.3g x its tolerance" % (sw, best))
        assert best >= 10, "switch %s moves every compared quantity by < 10 x its tolerance (%.3g)" % (sw, best)


def gen():
    multinomial_rule()
    mod = import_reference("MAAC_file", "MAAC_discrete")
    out = {}
    for name in GOLDEN_CASES:
        run_case(mod, name, out)
    conditions()
    np.savez_compressed(os.path.join(HERE, "maac.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen()
    print("wrote maac.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "maac.npz")))
