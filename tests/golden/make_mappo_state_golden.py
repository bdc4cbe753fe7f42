#!/usr/bin/env python3
"""Golden OUTPUT vectors of MAPPO_file/MAPPO_for_mask_action_state.py, by running the imported reference (PyTorch CPU) on the seeded
cases and the toy environment of tests/mappo_state_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_mappo_state_golden       # mappo_state.npz and loop_mappo_state.npz

The recipe is make_mappo_mask_golden.py's: the same smacv2 stub and `mod.device = "cpu"`, parameters through `load_state_dict`, rows
(and their states) through `add`, np.random's permutations recorded as drawn, `adv` / `v_target` read from learn()'s frame, the Agent's
update methods wrapped for the losses.

Conditions checked here, on the reference's own numbers, and fatal when missed: in every case the reference's first critic loss (the
POSITION pairing, :371-373) is what the oracle's POSITION pairing gives and differs by more than 1e-3 relative - ten times the loss
tolerance - both from what the SAMPLE pairing gives and from the loss with the state block zeroed; the masked maker's conditions on
masks (>= 50 % of the written rows with 2 .. A-1 open actions, the stored action open) and on Huber (delta < 1: >= 10 % of the first
critic step's errors on each side); in the episode run the winning p / q of every draw exceeds the runner-up by >= 1e-3 relative.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import mappo_oracle as mo  # noqa: E402
from tests import mappo_state_oracle as ms  # noqa: E402
from tests.golden import make_mappo_mask_golden as mask_maker  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import load, t2n  # noqa: E402
from tests.golden.make_mappo_golden import adam_state, ref_trick  # noqa: E402


def import_state():
    mask_maker.import_masked()           # (installs the smacv2 stub)
    mod = import_reference("MAPPO_file", "MAPPO_for_mask_action_state")
    mod.device = "cpu"
    return mod


def construct(mod, c, inp):
    agents = ["agent_%d" % i for i in range(len(c["dims"]))]
    dim_info = {a: list(d) for a, d in zip(agents, c["dims"])}
    nets = (mod.Actor, mod.Actor_discrete, mod.Critic)
    old = [k.__init__.__defaults__ for k in nets]
    for k, d in zip(nets, old):
        k.__init__.__defaults__ = (c["hidden"], c["hidden"]) + (None,) * (len(d) - 2)
    try:
        algo = mod.MAPPO(dim_info, c["cont"], c["actor_lr"], c["critic_lr"], c["horizon"], "cpu", trick=ref_trick(c), state_dim=c["state_dim"])
    finally:
        for k, d in zip(nets, old):
            k.__init__.__defaults__ = d
    for i, a in enumerate(agents):
        load(algo.agents[a].actor, inp["actors"][i])
        load(algo.agents[a].critic, inp["critics"][i])
    return algo, agents


def add_rows(algo, agents, rows, state, count):
    for t in range(count):
        col = lambda key, sq=False: {a: (rows[i][key][t][0] if sq else rows[i][key][t]) for i, a in enumerate(agents)}
        algo.add(col("obs"), col("act"), col("rew", True), col("next_obs"), col("done", True), col("logp"), col("adv_done", True), col("mask"), state[t])


def rel(a, b):
    return abs(a - b) / abs(a)


def run_case(mod, name, out):
    c = ms.case(name)
    inp = ms.inputs(c)
    algo, agents = construct(mod, c, inp)
    n, T, K = len(agents), c["horizon"], c["k_epochs"]
    fill = T if c["fill"] is None else c["fill"]
    mask_maker.check_masks(c, name, inp["rows"], fill)
    states = np.concatenate([inp["state"][:fill]] + ([ms.second_rows(c)[1]] if c["second"] else []))
    for t in range(len(states)):         # "distinct from every observation"
        assert not any(np.isin(states[t], r["obs"]).any() for r in inp["rows"])
    add_rows(algo, agents, inp["rows"], inp["state"], fill)
    assert all(np.array_equal(algo.buffers[a].states, ms.ring_state(c, inp).astype(np.float64)) for a in agents)
    ring = ms.mm.ring(c, inp)
    with torch.no_grad():
        vs0 = [algo.agents[a].critic([torch.as_tensor(r["obs"]) for r in ring], torch.as_tensor(ms.ring_state(c, inp))).numpy() for a in agents]
    losses = {a: [] for a in agents}
    for a in agents:
        ag = algo.agents[a]

        def wrap_a(l, _a=a, _f=ag.update_actor):
            losses[_a].append([float(l), None])
            _f(l)

        def wrap_c(l, _a=a, _f=ag.update_critic):
            losses[_a][-1][1] = float(l)
            _f(l)
        ag.update_actor, ag.update_critic = wrap_a, wrap_c
    drawn, seen, keep = [], [], []
    real_perm = np.random.permutation

    def perm(x):
        p = real_perm(x)
        drawn.append(np.asarray(p).copy())
        return p

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "learn":
            return None

        def local(fr, ev, ar):
            loc = fr.f_locals
            vt = loc.get("v_target")
            if ev == "line" and vt is not None and not any(vt is k for k in keep):
                keep.append(vt)
                seen.append((torch.as_tensor(loc["adv"]).detach().numpy().astype(np.float32).copy(), vt.detach().numpy().copy()))
            return local
        return local

    def learn():
        sys.settrace(tracer)
        try:
            # (the minibatch_size argument is ignored by the reference: :313)
            algo.learn(7, c["gamma"], c["lmbda"], c["clip"], K, c["ent_coef"], c["huber_delta"])
        finally:
            sys.settrace(None)
    np.random.seed(c["seed"] + 1000)
    np.random.permutation = perm
    try:
        learn()
        if c["second"]:
            second, second_state = ms.second_rows(c)
            mask_maker.check_masks(c, name, second, c["second"])
            add_rows(algo, agents, second, second_state, c["second"])
            learn()
    finally:
        np.random.permutation = real_perm
    calls = ms.calls(c)
    perms = np.stack(drawn).reshape(calls, n, K, T)
    assert np.array_equal(perms, ms.perms(c)), "the oracle's permutations are not np.random's"
    assert len(seen) == calls and algo.horizon == T
    out[name + "/perms"] = perms.astype(np.int64)
    out[name + "/adv"] = seen[-1][0].reshape(T, n).astype(np.float32)
    out[name + "/v_target"] = seen[-1][1].reshape(T, n).astype(np.float32)
    out[name + "/trace"] = np.array([losses[a] for a in agents], np.float64)
    vt0 = seen[0][1].reshape(T, n)
    small = [float((np.abs(vt0 - vs0[i]) <= c["huber_delta"]).mean()) for i in range(n)]
    out[name + "/frac_small"] = np.array(small)
    if c["trick"]["huber_loss"] and c["huber_delta"] < 1:
        assert all(0.1 <= s <= 0.9 for s in small), "%s: Huber branches %s" % (name, small)
    # the pairing and the state block are observable in the first critic loss
    got = [losses[a][0][1] for a in agents]
    ours = ms.run(c, calls_max=1).trace[:, 0, 1]
    sample = ms.run(dict(c, state_rows="sample"), calls_max=1).trace[:, 0, 1]
    zeroed = ms.run(c, calls_max=1, zero_state=True).trace[:, 0, 1]
    out[name + "/first_critic_loss_sample"] = np.array(sample, np.float64)
    out[name + "/first_critic_loss_zero_state"] = np.array(zeroed, np.float64)
    for g, o, s, z in zip(got, ours, sample, zeroed):
        assert rel(g, o) <= 1e-5, "%s: the oracle's POSITION pairing is not the reference's (%r vs %r)" % (name, g, o)
        assert rel(g, s) > 1e-3, "%s: the two pairings are within 1e-3 (%r vs %r)" % (name, g, s)
        assert rel(g, z) > 1e-3, "%s: the state block moves the loss by under 1e-3 (%r vs %r)" % (name, g, z)
    for i, a in enumerate(agents):
        ag = algo.agents[a]
        for tag, module, opt in (("actor", ag.actor, ag.actor_optimizer), ("critic", ag.critic, ag.critic_optimizer)):
            key = "%s/%d/%s" % (name, i, tag)
            sd = t2n(module.state_dict())
            m, v, step = adam_state(opt, module)
            assert all(np.isfinite(x).all() for x in sd.values()), key
            flat = lambda d: mo.flat(c, tag, d)
            if name in ms.FULL_CASES:
                out[key + "/p"] = flat(sd)
            out[key + "/digest"] = np.stack([mo.digest(flat(sd)), mo.digest(flat(m)), mo.digest(flat(v))])
            out[key + "/step"] = np.int64(step)
    print("%-8s first critic loss %s  sample %s  zero state %s  small %s" % (name, [round(x, 5) for x in got], [round(float(x), 5) for x in sample],
                                                                          [round(float(x), 5) for x in zeroed], [round(s, 2) for s in small]))


def gen_loop(mod):
    """the reference CLASS on the toy environment: every step's actions and log-probs, the Exp(1) draws, the final digests"""
    c = ms.LOOP
    inp = ms.inputs(c)
    algo, agents = construct(mod, c, inp)
    env = ms.ToyEnv(c)
    draws = [[] for _ in agents]
    margins = []

    def on_step(obs, avail):
        # what select_action is about to draw: one exponential_ of the row's shape per agent, from a copy of torch's generator state
        state = torch.get_rng_state()
        for i, a in enumerate(agents):
            q = torch.empty(1, c["dims"][i][1]).exponential_(1)
            draws[i].append(q.numpy()[0].copy())
            with torch.no_grad():
                dist = mod.CategoricalMasked(logits=algo.agents[a].actor(torch.as_tensor(obs[a], dtype=torch.float32).reshape(1, -1)),
                                             masks=torch.as_tensor(avail[a], dtype=torch.bool).reshape(1, -1))
                v = (dist.probs / q).numpy()[0]
            top = np.sort(v)[-2:]
            margins.append((top[1] - top[0]) / top[1])
        after = torch.get_rng_state()
        torch.set_rng_state(state)
        return after
    states = []
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"] + 1000)
    real_select = algo.select_action

    def select(obs, avail):
        out = real_select(obs, avail)
        assert torch.equal(torch.get_rng_state(), states[-1]), "select_action does not consume one exponential_ draw per agent"
        return out
    algo.select_action = select
    acts, lps = ms.run_loop(algo, env, on_step=lambda o, m: states.append(on_step(o, m)))
    assert min(margins) >= 1e-3, "the episode run has a draw within 1e-3 of a tie (%g): pick another seed" % min(margins)
    out = {"actions": acts, "logp": lps, "min_margin": np.float64(min(margins))}
    for i, a in enumerate(agents):
        out["q/%d" % i] = np.stack(draws[i]).astype(np.float32)
        out["%d/actor/digest" % i] = mo.digest(mo.flat(c, "actor", t2n(algo.agents[a].actor.state_dict())))
        out["%d/critic/digest" % i] = mo.digest(mo.flat(c, "critic", t2n(algo.agents[a].critic.state_dict())))
    np.savez_compressed(os.path.join(HERE, "loop_mappo_state.npz"), **out)
    print("loop     %d steps, smallest margin %.3g, actions[:4] %s" % (len(acts), min(margins), acts[:4].tolist()))


def gen():
    mod = import_state()
    out = {}
    for name in ms.CASES:
        run_case(mod, name, out)
    np.savez_compressed(os.path.join(HERE, "mappo_state.npz"), **out)
    gen_loop(mod)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen()
    for f in ("mappo_state.npz", "loop_mappo_state.npz"):
        print("wrote %s (%d bytes)" % (f, os.path.getsize(os.path.join(HERE, f))))
