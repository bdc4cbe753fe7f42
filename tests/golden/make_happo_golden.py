#!/usr/bin/env python3
"""Golden OUTPUT vectors of MAPPO_file/HAPPO.py's `learn`, by running the imported reference (PyTorch CPU) on the seeded cases of
tests/happo_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_happo_golden            # happo.npz and the loop fixture
    python -m tests.golden.make_happo_golden loops      # loop_happo_spread.npz only

Per case, as tests/golden/make_mappo_golden.py does it: the nets take the oracle module's PCG64 parameters through `load_state_dict`
(their width through the constructors' defaults), the rows go in through `add`, np.random is seeded with the case seed + 1000 and
torch with the case seed + 2000, the
Agent's update methods are wrapped for the losses, and a frame tracer reads `adv`, `v_target` and every value `factor` takes.
`torch.randperm` is wrapped: the order it returns is recorded, or replaced by the case's imposed order.  For the `_ident` case only,
`np.random.permutation` returns `arange`.  Recorded: the order, the permutations by agent id, the advantages before normalisation,
the value targets, the factors by visiting position, the (actor, critic) loss of every step, per net the final parameters (in full
for happo_oracle.FULL_CASES) and digests of them and of Adam's two moments, the step counts.  For the two discrete cases with real
minibatches the reference raises RuntimeError at HAPPO.py:453 (new log-probabilities of the last minibatch against old ones of the
whole horizon): that it does is asserted and stored, with the order it drew.

Conditions checked here on the reference's own numbers, fatal when missed: in every 3-agent continuous case at least 50 % of the
last visited agent's factor entries differ from 1 by more than 1e-2; the Huber case has >= 10 % of the first critic step's errors on
each side of delta; `order_a` and `order_b` end with different parameters for every actor.  The NumPy oracle's worst deviation from
the reference is printed per quantity and case (profiles/happo/README.md keeps the table).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import happo_oracle as ho  # noqa: E402
from tests import mappo_oracle as mo  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import load, t2n  # noqa: E402
from tests.golden.make_mappo_golden import adam_state, ref_trick  # noqa: E402


def build(mod, c, inp):
    agents = ["agent_%d" % i for i in range(len(c["dims"]))]
    dim_info = {a: list(d) for a, d in zip(agents, c["dims"])}
    nets = (mod.Actor, mod.Actor_discrete, mod.Critic)
    old = [k.__init__.__defaults__ for k in nets]
    for k in nets:
        k.__init__.__defaults__ = (c["hidden"], c["hidden"], None)
    try:
        algo = mod.HAPPO(dim_info, c["cont"], c["actor_lr"], c["critic_lr"], c["horizon"], "cpu", trick=ref_trick(c))
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


def run_case(mod, name, out, report):
    c = ho.case(name)
    inp = ho.inputs(c)
    algo, agents = build(mod, c, inp)
    n, T, mb, K = len(agents), c["horizon"], c["minibatch"], c["k_epochs"]
    with torch.no_grad():
        vs0 = [algo.agents[a].critic([torch.as_tensor(r["obs"]) for r in inp["rows"]]).numpy() for a in agents]
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
    drawn, orders, seen, factors = [], [], [], []
    real_perm, real_randperm = np.random.permutation, torch.randperm

    def perm(x):
        p = np.arange(x) if c["ident"] else real_perm(x)
        drawn.append(np.asarray(p).copy())
        return p

    def randperm(k, *a, **kw):
        o = real_randperm(k, *a, **kw)
        if c["order"] is not None:
            o = torch.as_tensor(c["order"], dtype=o.dtype)
        orders.append(o.numpy().copy())
        return o

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "learn":
            return None

        def local(fr, ev, ar):
            loc = fr.f_locals
            vt, f = loc.get("v_target"), loc.get("factor")
            if ev == "line" and vt is not None and not seen:
                seen.append((torch.as_tensor(loc["adv"]).detach().numpy().astype(np.float32).copy(), vt.detach().numpy().copy()))
            if ev in ("line", "return") and f is not None and not (factors and np.array_equal(factors[-1], np.asarray(f).reshape(-1))):
                factors.append(np.asarray(f, np.float32).reshape(-1).copy())
            return local
        return local
    np.random.seed(c["seed"] + 1000)
    torch.manual_seed(c["seed"] + 2000)           # (what torch.randperm draws the order from)
    np.random.permutation, torch.randperm = perm, randperm
    sys.settrace(tracer)
    raised = False
    try:
        algo.learn(mb, c["gamma"], c["lmbda"], c["clip"], K, c["ent_coef"], c["huber_delta"])
    except RuntimeError as ex:
        raised = True
        assert "must match the size of tensor" in str(ex), ex
    finally:
        sys.settrace(None)
        np.random.permutation, torch.randperm = real_perm, real_randperm
    assert raised == c["ref_raises"], "%s: reference raised = %s" % (name, raised)
    assert len(orders) == 1
    order = orders[0].astype(np.int64)
    out[name + "/order"] = order
    out[name + "/ref_raises"] = np.bool_(raised)
    o = ho.run(c, order, inp)                     # (the oracle's run: what the discrete cases' expected values are, and the deviation report)
    assert len(seen) == 1
    adv, vt = seen[0][0].reshape(T, n), seen[0][1].reshape(T, n)
    dev = dict(adv=float(np.abs(o.adv_raw - adv).max()), v_target=float(np.abs(o.v_target - vt).max()))
    if raised:
        # K permutations were drawn for the first visited agent before the exception; nothing after it is the reference's
        assert np.array_equal(np.stack(drawn), ho.perms(c, order)[order[0]])
        report.append((name, dev))
        print("%-18s the reference raises RuntimeError; order %s" % (name, order))
        return
    perms = np.zeros((n, K, T), np.int64)
    perms[order] = np.stack(drawn).reshape(n, K, T)
    assert np.array_equal(perms, ho.perms(c, order)), "the oracle's permutations are not np.random's"
    assert len(factors) == n and np.all(factors[0] == 1), len(factors)
    fac = np.stack(factors)
    out[name + "/perms"] = perms
    out[name + "/adv"] = adv.astype(np.float32)
    out[name + "/v_target"] = vt.astype(np.float32)
    out[name + "/factor"] = fac
    trace = np.array([losses[a] for a in agents], np.float64)
    out[name + "/trace"] = trace
    far = float((np.abs(fac[-1] - 1) > 1e-2).mean()) if n > 1 else 0.0
    out[name + "/frac_far"] = np.float64(far)
    if n == 3 and c["cont"]:
        assert far >= 0.5, "%s: only %.0f %% of the last factor's entries differ from 1 by more than 1e-2" % (name, 100 * far)
    small = []
    for i in range(n):
        e = np.abs(vt[perms[i][0][:mb]] - vs0[i][perms[i][0][:mb]])
        small.append(float((e <= c["huber_delta"]).mean()))
    out[name + "/frac_small"] = np.array(small)
    if c["trick"]["huber_loss"] and c["huber_delta"] < 1:
        assert all(0.1 <= s <= 0.9 for s in small), "%s: Huber branches %s" % (name, small)      # (a critic reads no other net: V before learn() is its first step's)
    dev.update(trace=float(np.abs(o.trace - trace).max()), trace_rel=float((np.abs(o.trace - trace) / (1e-6 / 1e-4 + np.abs(trace))).max()),
               factor=float(np.abs(o.factors - fac).max()), factor_rel=float((np.abs(o.factors - fac) / (1e-6 / 1e-4 + np.abs(fac))).max()))
    full = name in ho.FULL_CASES
    worst_p = worst_m = 0.0
    for i, a in enumerate(agents):
        ag = algo.agents[a]
        for tag, module, opt, mine, mopt in (("actor", ag.actor, ag.actor_optimizer, o.actors[i], o.aopt[i]),
                                             ("critic", ag.critic, ag.critic_optimizer, o.critics[i], o.copt[i])):
            key = "%s/%d/%s" % (name, i, tag)
            sd = t2n(module.state_dict())
            m, v, step = adam_state(opt, module)
            assert all(np.isfinite(x).all() for x in sd.values()), key
            flat = lambda d: mo.flat(c, tag, d)
            if full:
                out[key + "/p"] = flat(sd)
            out[key + "/digest"] = np.stack([mo.digest(flat(sd)), mo.digest(flat(m)), mo.digest(flat(v))])
            out[key + "/step"] = np.int64(step)
            d = np.abs(flat(mine).astype(np.float64) - flat(sd))
            worst_p = max(worst_p, float((d / (5e-6 + 5e-4 * np.abs(flat(sd)))).max()))
            worst_m = max(worst_m, float(np.abs(flat(mopt.m).astype(np.float64) - flat(m)).max() / np.abs(flat(m)).max()))
    dev.update(param_in_tol_units=worst_p, m_rel_to_max=worst_m)
    report.append((name, dev))
    print("%-18s order %s first losses %s  far %.2f small %s range %.3g..%.3g" % (name, order, [round(x, 6) for x in losses[agents[order[0]]][0]], far,
                                                                                 [round(s, 2) for s in small], fac[-1].min(), fac[-1].max()))


def gen():
    mod = import_reference("MAPPO_file", "HAPPO")
    out, report = {}, []
    for name in ho.CASES:
        run_case(mod, name, out, report)
    a, b = "happo_c_order_a", "happo_c_order_b"
    for i in range(3):
        assert not np.array_equal(out["%s/%d/actor/p" % (a, i)], out["%s/%d/actor/p" % (b, i)]), "orders a and b give actor %d the same parameters" % i
    np.savez_compressed(os.path.join(HERE, "happo.npz"), **out)
    print("\nthe NumPy oracle against the reference (worst absolute / tolerance-relative deviation):")
    for name, dev in report:
        print("  %-18s %s" % (name, "  ".join("%s %.3g" % kv for kv in dev.items())))


# HAPPO.py's own loop on SpreadEnv: make_mappo_golden's flags with the script's spelling of the switch
LOOP_FLAGS = ("--env_name simple_spread_v3 --N 3 --seed 100 --horizon 50 --max_episodes 6 --K_epochs 2 --minibatch_size 50 "
              "--continuous_actions 1 --device cpu")


def gen_loops():
    from tests.golden import synth
    from tests.golden.make_loop_golden import run_reference
    name = "loop_happo_spread"
    log, returns, sd, npy_name, ckpt_name = run_reference("MAPPO_file", "HAPPO", LOOP_FLAGS)
    out = {"flags": np.array(LOOP_FLAGS), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
           "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
    for a, d in sd.items():
        synth.pack_digest("ckpt/" + a, {k: v.numpy() for k, v in d.items()}, out, full_limit=0)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-20s steps %5d returns shape %s -> %.1f KB" % (name, len(log["actions"]), np.asarray(returns).shape, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    torch.set_num_threads(1)
    if sys.argv[1:] == ["loops"]:
        gen_loops()
        sys.exit(0)
    gen()
    gen_loops()
    print("wrote happo.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "happo.npz")))
