#!/usr/bin/env python3
"""Golden OUTPUT vectors of envelope multi-objective DQN (ENVELOPE_MORL_file/ENVELOPE_DQN.py), by running the imported
reference (PyTorch CPU) on the seeded cases of tests/envelope_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_envelope_golden

The script imports `mo_gymnasium`, which only its training loop uses: an empty module stands in for it.  A case's net is
`MLP(O, A, R, H, H)` swapped in for the constructor's default width, with PCG64 parameters through `load_state_dict`; the table
goes in through `add()` (which also fills `priority_mem`), and every `learn()` draws its rows (`np.random.choice` over the
priorities) and preference vectors (`np.random.randn`) from NumPy's seeded global stream.  The fixture records what each call
drew, the losses, and digests of the net, the target and Adam's moments.

a' = argmax_a w . Q_online(s', w)[a] is an argmax: a near-tie would let two correct float32 implementations take different
branches.  A seed is therefore kept only if the reference's gap between the two largest w . Q_online(s') is at least
envelope_oracle.MARGIN over every row of every call (the class case: also at every select_action); the smallest gap is stored.
The class case's seed must also draw the same rows when every priority is scaled by an independent factor in [1 - 1e-4, 1 + 1e-4].
"""
import os
import sys
import types
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import envelope_oracle as eo  # noqa: E402
from tests.golden import synth  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import CPU, adam_state, inject, load, t2n, wrap_losses  # noqa: E402

N_SEEDS = 48          # seeds tried per case


def reference():
    sys.modules.setdefault("mo_gymnasium", types.ModuleType("mo_gymnasium"))
    return import_reference("ENVELOPE_MORL_file", "ENVELOPE_DQN")


def build(mod, c, inp, capacity):
    pol = mod.ENVELOPE([c["obs_dim"], c["n_act"], c["rdim"]], False, c["lr"], capacity, CPU, c["beta"], c.get("max_episodes", 1000))
    H = c["hidden"]
    pol.agent.Qnet = mod.MLP(c["obs_dim"], c["n_act"], c["rdim"], H, H)
    load(pol.agent.Qnet, inp["params"])
    pol.agent.Qnet_target = deepcopy(pol.agent.Qnet)
    pol.agent.Qnet_optimizer = torch.optim.Adam(pol.agent.Qnet.parameters(), lr=c["lr"])
    return pol


class Recorder:
    """What a learn() call drew — the rows (through buffer.sample) and the preference vectors (through np.random.randn) — and the
    reference's smallest gap between the two largest w . Q_online(s') over the call's rows."""

    def __init__(self, pol):
        self.pol, self.idx, self.weights, self.min_gap = pol, [], [], np.inf
        self._sample, self._randn = pol.buffer.sample, np.random.randn

    def sample(self, indices):
        self.idx.append(np.asarray(indices, np.int64).copy())
        return self._sample(indices)

    def randn(self, *shape):
        raw = self._randn(*shape)
        w = (np.abs(raw) / np.linalg.norm(raw, ord=1, axis=1, keepdims=True)).astype(np.float32)
        self.weights.append(w)
        pol, idx = self.pol, self.idx[-1]
        with torch.no_grad():
            nobs = torch.as_tensor(pol.buffer.next_obs[idx], dtype=torch.float32).repeat(len(w), 1)
            wb = torch.as_tensor(w.repeat(len(idx), axis=0))
            s = torch.einsum("nar,nr->na", pol.agent.Qnet(nobs, wb), wb)
            top = torch.sort(s, dim=1).values
            self.min_gap = min(self.min_gap, float((top[:, -1] - top[:, -2]).min()))
        return raw

    def learn(self, c):
        with inject(self.pol.buffer, "sample", self.sample), inject(np.random, "randn", self.randn):
            self.pol.learn(c["batch"], c["gamma"], c["tau"], c["weight_num"], 1)


def pack_state(name, pol, out):
    synth.pack_digest(name + "/net", t2n(pol.agent.Qnet.state_dict()), out)
    synth.pack_digest(name + "/target", t2n(pol.agent.Qnet_target.state_dict()), out)
    m, v, step = adam_state(pol.agent.Qnet_optimizer, pol.agent.Qnet)
    synth.pack_digest(name + "/m", m, out)
    synth.pack_digest(name + "/v", v, out)
    out[name + "/step"] = np.int64(step)


def run_case(mod, c, seed):
    inp = eo.inputs(c, seed=seed)
    t = inp["table"]
    pol = build(mod, c, inp, len(t["done"]))
    np.random.seed(seed)
    torch.manual_seed(seed)
    for i in range(len(t["done"])):
        pol.add(t["obs"][i], int(t["act"][i, 0]), t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"])
    pol.beta = c["beta"]                 # the cases pin beta: the table's done rows have moved the homotopy
    losses = wrap_losses(pol.agent, ["update_Qnet"])
    rec = Recorder(pol)
    for _ in range(c["n_learn"]):
        rec.learn(c)
    return pol, rec, np.array(losses["update_Qnet"], np.float32)


def run_class(mod, c, seed):
    """The class case (envelope_oracle.CLASS): select_action + add per step, learn() on the schedule; -> None when a
    select_action gap is under the margin or a perturbed priority list draws other rows."""
    inp = eo.inputs(c, seed=seed)
    t = inp["table"]
    pol = build(mod, c, inp, c["capacity"])
    np.random.seed(seed)
    torch.manual_seed(seed)
    losses = wrap_losses(pol.agent, ["update_Qnet"])
    rec = Recorder(pol)
    prefs, choices, prios, betas, gaps = [], [], [], [], []
    randn = torch.randn

    def torch_randn(*a, **k):
        p = randn(*a, **k)
        prefs.append((torch.abs(p) / torch.norm(p, p=1)).numpy().copy())
        return p
    learn_at = set(eo.class_schedule(c))
    pert = np.random.default_rng(seed + 7)
    with inject(torch, "randn", torch_randn):
        for i in range(c["n_steps"]):
            choices.append(int(pol.select_action(t["obs"][i])))
            with torch.no_grad():
                w = torch.as_tensor(prefs[-1]).reshape(1, -1)
                s = (pol.agent.Qnet(torch.as_tensor(t["obs"][i]).reshape(1, -1), w)[0] @ w[0]).sort().values
                gaps.append(float(s[-1] - s[-2]))
            pol.add(t["obs"][i], int(t["act"][i, 0]), t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"])
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
    if min(gaps) < eo.MARGIN:
        return None
    extra = dict(pref=np.array(prefs, np.float32), choice=np.array(choices, np.int64), priority=np.array(prios, np.float64),
                 beta=np.array(betas, np.float64), final_priority=np.array(pol.priority_mem, np.float64),
                 select_gap=np.float64(min(gaps)))
    return pol, rec, np.array(losses["update_Qnet"], np.float32), extra


def gen():
    mod = reference()
    out = {}
    for name in list(eo.CASES) + ["class"]:
        c = eo.case(name)
        for k in range(N_SEEDS):
            seed = c["seed"] + k
            got = run_class(mod, c, seed) if name == "class" else run_case(mod, c, seed)
            if got is not None and got[1].min_gap >= eo.MARGIN:
                break
        else:
            raise SystemExit("%s: no seed in %d meets the argmax margin" % (name, N_SEEDS))
        pol, rec, losses = got[:3]
        assert rec.min_gap >= eo.MARGIN and len(losses) == c["n_learn"]
        out[name + "/seed"] = np.int64(seed)
        out[name + "/min_gap"] = np.float64(rec.min_gap)
        out[name + "/loss"] = losses
        out[name + "/idx"] = np.stack(rec.idx)
        out[name + "/weights"] = np.stack(rec.weights)
        pack_state(name, pol, out)
        if name == "class":
            for k2, v in got[3].items():
                out["class/" + k2] = v
        print("%-16s seed %d  min gap %.3g  loss %.6g .. %.6g" % (name, seed, rec.min_gap, losses[0], losses[-1]))
    np.savez_compressed(os.path.join(HERE, "envelope_dqn.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen()
    print("wrote envelope_dqn.npz")
