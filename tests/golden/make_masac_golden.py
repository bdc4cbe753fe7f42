#!/usr/bin/env python3
"""Golden OUTPUT vectors of MASAC (MAAC_file/MASAC.py), by running the imported reference class (PyTorch CPU) on the seeded cases of
tests/masac_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_masac_golden

A case's nets are `Actor(O, A, H, H)` and `Critic(dim_info, H, H)` with PCG64 parameters through `load_state_dict` (the `clamp` case's
log_std_layer rescaled the same way).  The ring of 300 rows goes in through `add()`; every `sample()` takes its rows from
`np.random.choice` and every `rsample()` its draw from `torch.distributions.normal._standard_normal`, both fed the oracle's PCG64
streams and recorded again in the fixture.  Per call the fixture holds both losses, both pre-clip gradient norms (what
`clip_grad_norm_` returns) and alpha per agent; after the 1st and the 3rd call digests of every online and target net and of Adam's
first moments, and log_alpha with its Adam state.  Outputs only, no program text.

The generator ASSERTS what the cases are for (see `conditions`): clamped and open log-stds in `clamp`, both critic heads the minimum
on >= 10 % of the rows, critic norms on both sides of the clip, and in `seq` the three oracle switches moving every compared
actor quantity by >= 10 x the GPU test's tolerance.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import masac_oracle as mo  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import CPU, adam_state, feeder, inject, load, t2n, wrap_losses  # noqa: E402

LOSS_TOL, NORM_RTOL, PARAM_TOL = (1e-4, 1e-6), 1e-3, (5e-4, 5e-6)      # the GPU test's (tests/test_gpu_masac.py)


def ids_of(c):
    return ["agent_%d" % j for j in range(len(c["dims"]))]


def build(mod, c, inp):
    ids = ids_of(c)
    dim_info = {a: list(c["dims"][j]) for j, a in enumerate(ids)}
    pol = mod.MASAC(copy.deepcopy(dim_info), True, c["actor_lr"], c["critic_lr"], c["n_table"], CPU)
    H = c["hidden"]
    for j, a in enumerate(ids):
        ag = pol.agents[a]
        ag.actor = mod.Actor(dim_info[a][0], dim_info[a][1], H, H)
        ag.critic = mod.Critic(dim_info, H, H)
        load(ag.actor, inp["actor"][j])
        load(ag.critic, inp["critic"][j])
        ag.actor_optimizer = torch.optim.Adam(ag.actor.parameters(), lr=c["actor_lr"])
        ag.critic_optimizer = torch.optim.Adam(ag.critic.parameters(), lr=c["critic_lr"])
        ag.actor_target, ag.critic_target = copy.deepcopy(ag.actor), copy.deepcopy(ag.critic)
        if c["alpha0"]:      # through the Alpha object, as a user would
            pol.alphas[a] = mod.Alpha(dim_info[a][1], alpha=c["alpha0"][j], requires_grad=True, is_continue=True)
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


def pack_net(prefix, tensors, names, out):
    out[prefix + "/stats"], out[prefix + "/sample"] = mo.compact_digest(tensors, names)


def pack_state(pre, pol, ids, out):
    for j, a in enumerate(ids):
        ag = pol.agents[a]
        for key in ("actor", "critic", "actor_target", "critic_target"):
            pack_net("%s/%d/%s" % (pre, j, key), t2n(getattr(ag, key).state_dict()), mo.ACTOR_NAMES if "actor" in key else mo.CRITIC_NAMES, out)
        for key, opt, net in (("actor", ag.actor_optimizer, ag.actor), ("critic", ag.critic_optimizer, ag.critic)):
            m, _, step = adam_state(opt, net)
            pack_net("%s/%d/%s_m" % (pre, j, key), m, mo.ACTOR_NAMES if key == "actor" else mo.CRITIC_NAMES, out)
            out["%s/%d/%s_step" % (pre, j, key)] = np.int64(step)
        al = pol.alphas[a]
        st = al.log_alpha_optimizer.state[al.log_alpha]
        out["%s/%d/alpha_state" % (pre, j)] = np.array([float(al.log_alpha), float(st["exp_avg"]), float(st["exp_avg_sq"]), float(al.alpha), float(st["step"])], np.float64)


def run_case(mod, name, out):
    c = mo.case(name)
    inp = mo.inputs(c)
    t = inp["table"]
    pol, ids = build(mod, c, inp)
    n, B = len(ids), c["batch"]
    for i in range(c["n_table"]):
        add_row(pol, ids, t, i)
    assert all(0 < x["done"].mean() < 1 for x in t), "done of both values"
    losses = [wrap_losses(pol.agents[a], ["update_critic", "update_actor"]) for a in ids]
    norms = Norms()
    flat_idx = [ix for per_call in inp["idx"] for ix in per_call]
    # the reference's draw order per updating agent: n target rsamples (sample()), n online ones (the actor loss), the entropy's
    flat_eps = [torch.as_tensor(e) for per_call in inp["eps"] for per_agent in per_call for e in per_agent]
    fed = feeder(flat_eps)

    def std_normal(shape, dtype, device):
        e = fed()
        assert tuple(e.shape) == tuple(shape), (tuple(e.shape), tuple(shape))
        return e.to(dtype)
    alphas = []
    with inject(np.random, "choice", feeder(flat_idx)), inject(torch.nn.utils, "clip_grad_norm_", norms.clip), \
            inject(torch.distributions.normal, "_standard_normal", std_normal):
        for k in range(c["n_learn"]):
            pol.learn(B, c["gamma"], c["tau"])
            alphas.append([float(pol.alphas[a].alpha.detach()) for a in ids])
            if k + 1 in mo.RECORD_AFTER:
                pack_state("%s/after%d" % (name, k + 1), pol, ids, out)
    try:
        fed()
        raise AssertionError("draws left over: the reference took fewer than 2 n + 1 per agent")
    except StopIteration:
        pass
    nv = np.array(norms.v, np.float64).reshape(c["n_learn"], n, 2)
    am = max(a for _, a in c["dims"])
    out[name + "/idx"] = np.stack(inp["idx"])
    out[name + "/eps"] = np.stack([mo.pad_eps(inp["eps"][k], n, B, am) for k in range(c["n_learn"])])
    out[name + "/critic_loss"] = np.array([l["update_critic"] for l in losses], np.float32).T       # [calls, n]
    out[name + "/actor_loss"] = np.array([l["update_actor"] for l in losses], np.float32).T
    out[name + "/critic_norm"], out[name + "/actor_norm"] = nv[:, :, 0], nv[:, :, 1]
    out[name + "/alpha"] = np.array(alphas, np.float64)
    print("%-8s critic loss %s\n         actor loss %s\n         critic norms %s\n         actor norms %s\n         alpha %s" %
          (name, np.round(out[name + "/critic_loss"][0], 4), np.round(out[name + "/actor_loss"][0], 4), np.round(nv[:, :, 0], 3).tolist(),
           np.round(nv[:, :, 1], 4).tolist(), np.round(alphas[-1], 6)))
    return nv


def run_oracle(name, dtype=np.float64, **sw):
    c = mo.case(name)
    inp = mo.inputs(c)
    o = mo.make(c, inp, dtype, **sw)
    return o, [o.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"]) for k in range(c["n_learn"])]


def switch_factors(name="seq"):
    """per switch, with the switch on through all the case's calls: the smallest, over the compared agents (1.. ; mean_twins: 0.. too), of
    |switched - true| / tolerance for the last call's actor loss and actor pre-clip norm and for the actor's parameters after it (their
    99th percentile under the parameter tolerance, as _assert_net counts).  (After ONE call the parameters could not tell: Adam's first
    step is lr x sign(gradient) whatever the gradient's size.)"""
    c = mo.case(name)
    n = len(c["dims"])
    inp = mo.inputs(c)
    res = {}
    for sw in ("stale_actors", "one_draw", "mean_twins"):
        o = mo.make(c, inp, np.float64)
        x = mo.make(c, inp, np.float64, **{sw: True})
        for k in range(c["n_learn"]):
            a, b = o.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"]), x.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"])
        f = dict(loss=np.inf, norm=np.inf, param=np.inf)
        for i in range(0 if sw == "mean_twins" else 1, n):
            f["loss"] = min(f["loss"], abs(float(a["actor_loss"][i]) - float(b["actor_loss"][i])) / (LOSS_TOL[1] + LOSS_TOL[0] * abs(float(a["actor_loss"][i]))))
            f["norm"] = min(f["norm"], abs(a["actor_norm"][i] - b["actor_norm"][i]) / (NORM_RTOL * abs(a["actor_norm"][i])))
            worst = max(float(np.quantile(np.abs(o.actor[i][k] - x.actor[i][k]) / (PARAM_TOL[1] + PARAM_TOL[0] * np.abs(o.actor[i][k])), 0.99)) for k in o.actor[i])
            f["param"] = min(f["param"], worst)
        res[sw] = f
    return res


def conditions(out, all_norms):
    cn = np.concatenate([v[:, :, 0].reshape(-1) for v in all_norms.values()])
    an = np.concatenate([v[:, :, 1].reshape(-1) for v in all_norms.values()])
    assert (cn > 0.5).any() and (cn < 0.5).any(), "critic pre-clip norms on both sides of 0.5 across agents"
    print("cases whose own critic norms sit on both sides of 0.5: %s" % [nm for nm, nv in all_norms.items() if (nv[:, :, 0] > 0.5).any() and (nv[:, :, 0] < 0.5).any()])
    print("critic norms on both sides of the clip in every case: yes; actor norms above / below 0.5 anywhere: %s / %s (largest %.4g)" %
          ((an > 0.5).any(), (an < 0.5).any(), an.max()))
    for name in mo.CASES:
        _, outs = run_oracle(name)
        for key in ("head0_target", "head0_actor"):      # over the case's rows: every call's, every agent's (equal batches: the mean of the shares)
            fr = float(np.mean([o[key] for o in outs]))
            assert 0.1 <= fr <= 0.9, "%s %s: a critic head is the minimum on < 10 %% of the case's rows (Q1: %.3f)" % (name, key, fr)
            print("%-8s %s: Q1 is the minimum on %.0f %% of the rows" % (name, key, 100 * fr))
    _, outs = run_oracle("clamp")
    raw = np.concatenate([r.reshape(-1) for o in outs for r in o["raw_log_std"]])
    assert (raw > 2).any() and (raw < -20).any() and ((raw >= -20) & (raw <= 2)).any(), "clamp: log-stds above +2, below -20 and open"
    print("clamp: %d of %d actor-stage log-stds clamped at +2, %d at -20" % ((raw > 2).sum(), raw.size, (raw < -20).sum()))
    fac = switch_factors()
    for sw, f in fac.items():
        print("seq, %-12s moves actor loss / norm / parameters by %.3g / %.3g / %.3g x the tolerance" % (sw, f["loss"], f["norm"], f["param"]))
        assert min(f.values()) >= 10, "seq: switch %s moves a compared quantity by only %s x its tolerance" % (sw, f)


def gen():
    mod = import_reference("MAAC_file", "MASAC")
    out, all_norms = {}, {}
    for name in mo.CASES:
        all_norms[name] = run_case(mod, name, out)
    conditions(out, all_norms)
    np.savez_compressed(os.path.join(HERE, "masac.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    if "--conditions" in sys.argv:       # the oracle-only conditions (choosing seeds and scales): no reference needed
        print(switch_factors())
    else:
        gen()
        print("wrote masac.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "masac.npz")))
