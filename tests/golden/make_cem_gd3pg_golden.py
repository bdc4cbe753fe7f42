#!/usr/bin/env python3
"""Golden OUTPUT vectors of CEM_GD3PG.learn (CEM_GD3PG_file/CEM_GD3PG.py) and of sepCEM (CEM_GD3PG_file/ES.py), by running the imported
reference (PyTorch CPU, NumPy) on the seeded cases of tests/cem_gd3pg_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_cem_gd3pg_golden

A case's nets are `Actor(O, A, H, H)` / `Critic(O, A, H, H)` swapped in for the constructor's default width, with PCG64 parameters
through `load_state_dict` (the targets drifted from their online nets, so that both branches of the minimum are taken); both tables go
in through `add()`; every `learn()` draws its rows from NumPy's seeded global stream through the reference's own `sample()`.  The
fixture records what each call drew, the three losses, the three pre-clip gradient norms (what `clip_grad_norm_` returns), KL, and
digests of the six nets and Adam's moments after call 1 and after call 3.

Asserted here, from the reference alone (a seed that misses one is skipped, the next one tried):
  * each branch of min(Q1', Q2') is taken on at least 20 % of the rows of every call, and min |Q1' - Q2'| >= 100 eps32 max |Q'|;
  * KL > 0 on every call; both `done` values occur among every call's rows;
  * every LeakyReLU pre-activation of every critic forward of a call (both target passes, the TD pass, both actors' passes through the
    stepped critic) is further from 0 than 16 eps32 sum |w x| of its unit;
and across the cases: the critic's, the guided actor's and the unguided actor's pre-clip norms each lie on both sides of 0.5; one case
has is_F1_more false; one samples rows of `buffer` that were never written.  Last, every switch of the oracle moves a compared
quantity of every case by at least 10 x its tolerance (tests/test_cem_gd3pg_golden.py holds the switched oracles to "misses"); the one
exception is arithmetic: `kl_ba` divides by B A instead of B, which is the same number on `pend`'s one-column action.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import cem_gd3pg_oracle as co  # noqa: E402
from tests.golden._ref_import import REF_ROOT, import_reference  # noqa: E402
from tests.golden.make_golden import CPU, adam_state, inject, load, t2n, wrap_losses  # noqa: E402

N_SEEDS = 4000          # (the walker case's ~10^6 LeakyReLU pre-activations all clear the margin on about one seed in 300)
EPS32 = float(np.finfo(np.float32).eps)
LOSS_TOL, NORM_RTOL = (1e-4, 1e-6), 1e-3          # what the tests compare with


def reference():
    return import_reference("CEM_GD3PG_file", "CEM_GD3PG")


def build(mod, c, inp):
    O, A, H = c["obs_dim"], c["act_dim"], c["hidden"]
    pol = mod.CEM_GD3PG([O, A], True, c["actor_lr"], c["critic_lr"], c["cap"], CPU)
    ag = pol.agent
    for key in ("actor_1", "actor_2", "actor_domain", "actor_1_target", "actor_2_target"):
        setattr(ag, key, mod.Actor(O, A, H, H))
        load(getattr(ag, key), inp[key])
    for key in ("critic", "critic_target"):
        setattr(ag, key, mod.Critic(O, A, H, H))
        load(getattr(ag, key), inp[key])
    ag.actor_1_optimizer = torch.optim.Adam(ag.actor_1.parameters(), lr=c["actor_lr"])
    ag.actor_2_optimizer = torch.optim.Adam(ag.actor_2.parameters(), lr=c["actor_lr"])
    ag.critic_optimizer = torch.optim.Adam(ag.critic.parameters(), lr=c["critic_lr"])
    for buf, key in ((pol.buffer, "table0"), (pol.buffer_domain, "table1")):
        t = inp[key]
        for i in range(len(t["done"])):
            pol.add(buf, t["obs"][i], t["act"][i], float(t["rew"][i]), t["next_obs"][i], bool(t["done"][i]))
    return pol


def leaky_margin(critic, x):
    """min over the critic's hidden units and rows of |z| / (16 eps32 sum |w x|): > 1 means no unit is within rounding of its kink"""
    worst = np.inf
    h = x.double()
    for lin in (critic.l1, critic.l2):
        w, b = lin.weight.detach().double(), lin.bias.detach().double()
        z = h @ w.T + b
        bound = h.abs() @ w.abs().T + b.abs()
        worst = min(worst, float((z.abs() / (16 * EPS32 * bound)).min()))
        h = torch.nn.functional.leaky_relu(z)
    return worst


class Rejected(Exception):
    pass


class Recorder:
    """Per learn() call: the two index draws, the three clip norms (critic, then the two actors in the order the reference steps them), KL,
    and the conditions the generator asserts."""

    def __init__(self, pol, c):
        self.pol, self.c = pol, c
        self.idx, self.norms, self.kl, self.why = [], [], [], None
        self._choice, self._clip, self._sqrt = np.random.choice, torch.nn.utils.clip_grad_norm_, torch.sqrt
        self._draws = []

    def choice(self, *a, **k):
        out = self._choice(*a, **k)
        self._draws.append(np.asarray(out, np.int64).copy())
        return out

    def clip(self, params, max_norm, *a, **k):
        total = self._clip(params, max_norm, *a, **k)
        self.norms.append(float(total))
        return total

    def sqrt(self, x):
        out = self._sqrt(x)
        self.kl.append(float(out.detach()))
        return out

    def fail(self, why):
        self.why = why
        raise Rejected(why)          # (the rest of the seed's run would be thrown away)

    def learn(self):
        pol, c, ag = self.pol, self.c, self.pol.agent
        self._draws = []
        seen = {}

        def update_critic(loss, _orig=ag.update_critic):
            _orig(loss)
            with torch.no_grad():          # the stepped critic on (s, actor_j(s)): what both actor steps go through
                obs = seen["obs"]
                for actor in (ag.actor_1, ag.actor_2):
                    if leaky_margin(ag.critic, torch.cat([obs, actor(obs)], 1)) <= 1:
                        self.fail("a LeakyReLU unit of the stepped critic within rounding of 0")

        def sample(batch, _orig=pol.sample):
            out = _orig(batch)
            obs, act, rew, nobs, done = out
            seen["obs"] = obs
            with torch.no_grad():
                a1, a2 = ag.actor_1_target(nobs), ag.actor_2_target(nobs)
                q1, q2 = ag.critic_target(nobs, a1), ag.critic_target(nobs, a2)
                share = float((q1 < q2).float().mean())
                if min(share, 1 - share) < 0.2:
                    self.fail("a branch of the minimum on %.2f of the rows" % min(share, 1 - share))
                if float((q1 - q2).abs().min()) < 100 * EPS32 * float(torch.max(q1.abs().max(), q2.abs().max())):
                    self.fail("Q1' and Q2' of a row within rounding")
                if len(set(done.reshape(-1).tolist())) != 2:
                    self.fail("one done value only")
                for x in (torch.cat([nobs, a1], 1), torch.cat([nobs, a2], 1)):
                    if leaky_margin(ag.critic_target, x) <= 1:
                        self.fail("a LeakyReLU unit of the target critic within rounding of 0")
                if leaky_margin(ag.critic, torch.cat([obs, act], 1)) <= 1:
                    self.fail("a LeakyReLU unit of the critic within rounding of 0")
            return out

        with inject(np.random, "choice", self.choice), inject(torch.nn.utils, "clip_grad_norm_", self.clip), inject(torch, "sqrt", self.sqrt), \
                inject(pol, "sample", sample), inject(ag, "update_critic", update_critic):
            pol.learn(c["batch"], c["gamma"], c["tau"], c["f1_more"], c["delta"], ag.actor_domain)
        assert len(self._draws) == 2
        self.idx.append(np.stack(self._draws))
        if not self.kl[-1] > 0:
            self.fail("KL == 0")


def pack_state(prefix, pol, out):
    """digests (tests/cem_gd3pg_oracle.py: digest) of the seven nets and of the three optimisers' first and second moments"""
    ag = pol.agent
    states = {key: t2n(getattr(ag, key).state_dict()) for key in ("actor_1", "actor_2", "critic", "actor_1_target", "actor_2_target", "critic_target", "actor_domain")}
    for key, opt in (("actor_1", ag.actor_1_optimizer), ("actor_2", ag.actor_2_optimizer), ("critic", ag.critic_optimizer)):
        states[key + "_m"], states[key + "_v"], step = adam_state(opt, getattr(ag, key))
        out[prefix + "/" + key + "_step"] = np.int64(step)
    for key, p in states.items():
        out[prefix + "/" + key + "/sums"], out[prefix + "/" + key + "/sample"] = co.digest(p)


def run_case(mod, c, seed):
    inp = co.inputs(c, seed=seed)
    pol = build(mod, c, inp)
    np.random.seed(seed)
    torch.manual_seed(seed)
    losses = wrap_losses(pol.agent, ["update_critic", "update_actor_1", "update_actor_2"])
    rec = Recorder(pol, c)
    out = {}
    try:
        for k in range(c["n_learn"]):
            rec.learn()
            if k in (0, c["n_learn"] - 1):
                pack_state("call%d" % (k + 1), pol, out)
    except Rejected:
        pass
    return rec, losses, out


def record(rec, losses, c):
    """[calls][8] in the oracle's OUT order"""
    n = c["n_learn"]
    norms = np.array(rec.norms, np.float64).reshape(n, 3)
    # the reference steps the unguided actor first (:201-216): f1_more -> actor_1 then actor_2, else actor_2 then actor_1
    a1n, a2n = (norms[:, 1], norms[:, 2]) if c["f1_more"] else (norms[:, 2], norms[:, 1])
    rows = 2 * (min(c["n1"], c["batch"]) // 2)
    return np.stack([np.array(losses["update_critic"], np.float64), norms[:, 0], np.array(losses["update_actor_1"], np.float64), a1n,
                     np.array(losses["update_actor_2"], np.float64), a2n, np.array(rec.kl, np.float64), np.full(n, float(rows))], axis=1)


def moved(ref, got):
    """does `got` [calls][8] differ from the record by at least 10 x the tolerance the tests compare with, somewhere?"""
    for col in range(7):
        rtol, atol = (NORM_RTOL, 0.0) if col in (1, 3, 5) else LOSS_TOL
        if np.any(np.abs(got[:, col] - ref[:, col]) > 10 * (atol + rtol * np.abs(ref[:, col]))):
            return True
    return False


def gen_learn(out):
    mod = reference()
    sides = {"critic": [], "guided": [], "unguided": []}
    for name in co.CASES:
        c = co.case(name)
        for k in range(N_SEEDS):
            seed = c["seed"] + k
            rec, losses, state = run_case(mod, c, seed)
            if rec.why is None:
                break
        else:
            raise SystemExit("%s: no seed in %d meets the conditions" % (name, N_SEEDS))
        ref = record(rec, losses, c)
        inp = co.inputs(c, seed=seed)
        inp["idx"] = rec.idx
        for sw in co.SWITCHES:
            if sw == "kl_ba" and c["act_dim"] == 1:          # B A == B: the switch is the identity on a one-column action
                continue
            _, got = co.run(c, inp, switches=(sw,))
            assert moved(ref, got), "%s: the switch %s moves nothing by 10 x its tolerance" % (name, sw)
        _, plain = co.run(c, inp)
        assert not moved(ref, plain), "%s: the float32 oracle itself is 10 x its tolerance off the record" % name
        g = 5 if c["f1_more"] else 3          # OUT column of the guided actor's norm
        sides["critic"] += list(ref[:, 1]); sides["guided"] += list(ref[:, g]); sides["unguided"] += list(ref[:, 8 - g])
        out[name + "/seed"] = np.int64(seed)
        out[name + "/out"] = ref
        out[name + "/idx"] = np.stack(rec.idx)
        for k2, v in state.items():
            out[name + "/" + k2] = v
        print("%-8s seed %d  critic %.5g .. %.5g norm %s | actor_1 norm %s | actor_2 norm %s | KL %s" %
              (name, seed, ref[0, 0], ref[-1, 0], np.round(ref[:, 1], 3), np.round(ref[:, 3], 3), np.round(ref[:, 5], 3), np.round(ref[:, 6], 3)))
    for key, v in sides.items():
        assert min(v) < 0.5 < max(v), "%s norms on one side of 0.5: %s" % (key, np.round(v, 3))
    assert any(not co.case(n)["f1_more"] for n in co.CASES)
    short = co.case("short")
    assert short["n0"] < short["n1"] and out["short/idx"][:, 0].max() >= short["n0"], "no unwritten row of `buffer` was sampled"


# ------------------------------------------------------------------------------------ sepCEM
def gen_sepcem(out):
    sys.path.insert(0, os.path.join(REF_ROOT, "CEM_GD3PG_file"))
    try:
        import ES
    finally:
        sys.path.pop(0)
    for name, cfg in co.SEPCEM.items():
        for k, v in co.sepcem_script(ES.sepCEM, cfg, co.SEPCEM_SEED).items():
            out["sepcem/%s/%s" % (name, k)] = v


if __name__ == "__main__":
    torch.set_num_threads(1)
    fixture = {}
    gen_learn(fixture)
    gen_sepcem(fixture)
    path = os.path.join(HERE, "cem_gd3pg.npz")
    np.savez_compressed(path, **fixture)
    print("wrote cem_gd3pg.npz: %d bytes" % os.path.getsize(path))
