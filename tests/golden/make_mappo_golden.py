#!/usr/bin/env python3
"""Golden OUTPUT vectors of MAPPO_file/MAPPO.py and IPPO.py's `learn`, by running the imported reference (PyTorch CPU) on the seeded
cases of tests/mappo_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_mappo_golden            # mappo.npz and the two loop fixtures
    python -m tests.golden.make_mappo_golden loops      # loop_mappo_spread.npz and loop_ippo_spread.npz only

Per case: every agent's nets take the oracle module's PCG64 parameters through `load_state_dict`, the rows go in through `add`, the
minibatch permutations are np.random's after `np.random.seed(case seed + 1000)` (recorded as drawn).  Recorded: the advantages before
normalisation and the value targets (read from learn()'s frame on the line after `v_target = adv + vs`), the (actor, critic) loss of
every step (the Agent's update methods are wrapped), per net the final parameters (in full for mappo_oracle.FULL_CASES) and digests of
them and of Adam's two moments, the step counts.

Conditions checked here, on the reference's own numbers, and fatal when missed: a Huber case has >= 10 % of the first critic step's
errors on each side of delta; a ValueClip case has >= 25 % of that step's rows clamped.  `Critic.id_num` (IPPO.py:119-126) is a class
counter: it is reset before every construction, which is what a fresh process gives the script.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import mappo_oracle as mo  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import load, t2n  # noqa: E402


def adam_state(opt, module):
    """exp_avg / exp_avg_sq of `module`'s parameters (MAPPO's one optimiser holds the actor's and the critic's), and the step count"""
    names = {id(p): n for n, p in module.named_parameters()}
    m, v, step = {}, {}, 0
    for group in opt.param_groups:
        for p in group["params"]:
            st = opt.state.get(p, None)
            if st and id(p) in names:
                m[names[id(p)]] = st["exp_avg"].numpy().copy()
                v[names[id(p)]] = st["exp_avg_sq"].numpy().copy()
                step = int(st["step"])
    return m, v, step


def ref_trick(c):
    t = dict(ObsNorm=False, reward_norm=False, reward_scaling=False, orthogonal_init=False, lr_decay=False)
    t.update(c["trick"])
    return t


def build(mod, c, inp):
    agents = ["agent_%d" % i for i in range(len(c["dims"]))]
    dim_info = {a: list(d) for a, d in zip(agents, c["dims"])}
    if c["kind"] == "ippo":
        mod.Critic.id_num = 0
    cls = mod.MAPPO if c["kind"] == "mappo" else mod.IPPO
    # the nets' width is a default argument of their constructors (hidden_1 = hidden_2 = 128) that Agent never passes: the case's width
    # goes in there for the construction
    nets = (mod.Actor, mod.Actor_discrete, mod.Critic)
    old = [k.__init__.__defaults__ for k in nets]
    for k in nets:
        k.__init__.__defaults__ = (c["hidden"], c["hidden"], None)
    try:
        algo = cls(dim_info, c["cont"], c["actor_lr"], c["critic_lr"], c["horizon"], "cpu", trick=ref_trick(c))
    finally:
        for k, d in zip(nets, old):
            k.__init__.__defaults__ = d
    for i, a in enumerate(agents):
        load(algo.agents[a].actor, inp["actors"][i])
        load(algo.agents[a].critic, inp["critics"][i])
    for t in range(c["horizon"]):
        col = lambda key, sq=False: {a: (inp["rows"][i][key][t][0] if sq else inp["rows"][i][key][t]) for i, a in enumerate(agents)}
        algo.add(col("obs"), col("act"), col("rew", True), col("next_obs"), col("done", True), col("logp"), col("adv_done", True))
    return algo, agents


def run_case(mods, name, out):
    c = mo.case(name)
    inp = mo.inputs(c)
    algo, agents = build(mods[c["kind"]], c, inp)
    n, T, mb = len(agents), c["horizon"], c["minibatch"]
    # V(s) of every critic before learn(): the first critic step's errors are v_target[index] - this
    with torch.no_grad():
        vs0 = [algo.agents[a].critic([torch.as_tensor(r["obs"]) for r in inp["rows"]] if c["kind"] == "mappo" else torch.as_tensor(inp["rows"][i]["obs"])).numpy()
               for i, a in enumerate(agents)]
    losses = {a: [] for a in agents}
    for a in agents:
        ag = algo.agents[a]
        if c["kind"] == "mappo":
            def wrap(al, cl, _a=a, _f=ag.update_ac):
                losses[_a].append((float(al), float(cl)))
                _f(al, cl)
            ag.update_ac = wrap
        else:
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
    np.random.seed(c["seed"] + 1000)
    np.random.permutation = perm
    sys.settrace(tracer)
    try:
        algo.learn(mb, c["gamma"], c["lmbda"], c["clip"], c["k_epochs"], c["ent_coef"], c["huber_delta"])
    finally:
        sys.settrace(None)
        np.random.permutation = real_perm
    perms = np.stack(drawn).reshape(n, c["k_epochs"], T)
    assert np.array_equal(perms, mo.perms(c)), "the oracle's permutations are not np.random's"
    if c["kind"] == "mappo":
        assert len(seen) == 1
        adv, vt = seen[0][0].reshape(T, n), seen[0][1].reshape(T, n)
    else:
        assert len(seen) == n
        adv = np.concatenate([s[0].reshape(T, 1) for s in seen], axis=1)
        vt = np.concatenate([s[1].reshape(T, 1) for s in seen], axis=1)
    out[name + "/perms"] = perms.astype(np.int64)
    out[name + "/adv"] = adv.astype(np.float32)
    out[name + "/v_target"] = vt.astype(np.float32)
    out[name + "/trace"] = np.array([losses[a] for a in agents], np.float64)
    # the conditions of the Huber and ValueClip cases, on the first critic step of every agent
    small, clamped = [], []
    for i in range(n):
        ix = perms[i][0][:mb]
        e = np.abs((vt[ix] if c["kind"] == "mappo" else vt[ix][:, i:i + 1]) - vs0[i][ix])
        small.append(float((e <= c["huber_delta"]).mean()))
        clamped.append(float((e > c["clip"]).mean()))
    out[name + "/frac_small"] = np.array(small)
    out[name + "/frac_clamped"] = np.array(clamped)
    if c["trick"]["huber_loss"] and c["huber_delta"] < 1:
        assert all(0.1 <= s <= 0.9 for s in small), "%s: Huber branches %s" % (name, small)
    if c["trick"]["ValueClip"]:
        assert all(f >= 0.25 for f in clamped), "%s: clamped rows %s" % (name, clamped)
    full = c["hidden"] <= 32 and name in mo.FULL_CASES
    for i, a in enumerate(agents):
        ag = algo.agents[a]
        opts = (ag.ac_optimizer, ag.ac_optimizer) if c["kind"] == "mappo" else (ag.actor_optimizer, ag.critic_optimizer)
        for tag, module, opt in (("actor", ag.actor, opts[0]), ("critic", ag.critic, opts[1])):
            key = "%s/%d/%s" % (name, i, tag)
            sd = t2n(module.state_dict())
            m, v, step = adam_state(opt, module)
            assert all(np.isfinite(x).all() for x in sd.values()), key
            flat = lambda d: mo.flat(c, tag, d)
            if full:
                out[key + "/p"] = flat(sd)
            out[key + "/digest"] = np.stack([mo.digest(flat(sd)), mo.digest(flat(m)), mo.digest(flat(v))])
            out[key + "/step"] = np.int64(step)
    print("%-18s first (actor, critic) loss %s  small %s clamped %s" % (name, [round(x, 6) for x in losses[agents[0]][0]],
                                                                           [round(s, 2) for s in small], [round(s, 2) for s in clamped]))


def gen():
    mods = dict(mappo=import_reference("MAPPO_file", "MAPPO"), ippo=import_reference("MAPPO_file", "IPPO"))
    out = {}
    for name in mo.CASES:
        run_case(mods, name, out)
    np.savez_compressed(os.path.join(HERE, "mappo.npz"), **out)


# the scripts' own loops on SpreadEnv: their defaults except a short run with three learn() calls inside it, the in-repo environment
# (continuous actions) and the CPU
LOOP_FLAGS = ("--env_name simple_spread_v3 --N 3 --seed 100 --horizon 50 --max_episodes 6 --K_epochs 2 --minibatch_size 50 "
              "--continuous_actions True --device cpu")
LOOPS = {"loop_mappo_spread": ("MAPPO_file", "MAPPO", LOOP_FLAGS), "loop_ippo_spread": ("MAPPO_file", "IPPO", LOOP_FLAGS)}


def gen_loops():
    """tests/golden/make_loop_golden.py's recipe (its Recorder around SpreadEnv, its fixture layout) on the two scripts"""
    from tests.golden import synth
    from tests.golden.make_loop_golden import run_reference
    for name, (directory, script, flags) in LOOPS.items():
        log, returns, sd, npy_name, ckpt_name = run_reference(directory, script, flags)
        out = {"flags": np.array(flags), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
               "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
        for a, d in sd.items():
            synth.pack_digest("ckpt/" + a, {k: v.numpy() for k, v in d.items()}, out, full_limit=0)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-20s steps %5d returns[:3] %s -> %.1f KB" % (name, len(log["actions"]), np.round(np.asarray(returns).reshape(-1)[:3], 3),
                                                              os.path.getsize(path) / 1024))


if __name__ == "__main__":
    torch.set_num_threads(1)
    if sys.argv[1:] == ["loops"]:
        gen_loops()
        sys.exit(0)
    gen()
    gen_loops()
    print("wrote mappo.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "mappo.npz")))
