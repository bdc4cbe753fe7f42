"""Time of one HAPPO `learn()` (kernels_happo.hip) at the reference script's shape:

  3 agents x (18 obs, 5 continuous actions), hidden 128, horizon 256 in one minibatch of 256, K_epochs 15, every trick on

Per population P three sides, run ALTERNATELY, block by block, in this one command (tools/mappo_bench.py's scheme: a block is a few
calls between two synchronisations, host clock, after a warm-up call of each side): `frl_happo_learn` with the order and the
permutations drawn by the engine; `frl_mappo_learn` on a MAPPO engine of the same shape, rows and Adam settings (the parallel update
HAPPO gives up); and HAPPO.learn written with torch on the same device, eager (MAPPO_file/HAPPO.py:339-458 with the horizon-wide new
log-probabilities for both kinds), P learners one after the other.  Prints one JSON line per (P, side).
    python tools/happo_bench.py [--no-torch] [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402
from mappo_bench import A, DELTA, H, HYPER, K, LR, MB, NA, O, T, _block, _rows  # noqa: E402

BLOCKS = 3
KW = dict(HYPER, actor_lr=LR, critic_lr=LR, adam_eps=1e-5, clip_norm=0.5, adv_norm=True, value_clip=True, huber_delta=DELTA)


def _engine(algo, P, rows):
    e = Engine(algo, [O] * NA, [A] * NA, T, n_learners=P, hidden=H, batch_max=MB, extra_cols=NA * A + NA)
    e.net_norm_set(True, True)
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            w = (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32)
            if net % 2 == 0:
                w[-A:] = 0
            e.set_params(net, w, learner=p)
    f = lambda x: x.reshape(P * T, -1)
    recs = np.concatenate([f(rows["obs"]), f(rows["act"]), f(rows["rew"]), f(rows["done"]), f(rows["nobs"]), f(rows["logp"]), f(rows["adv_done"])], axis=1)
    e.add_batch(recs, learners=np.repeat(np.arange(P), T).astype(np.int32))
    e.flush()
    return e


def _hip_call(e, learn):
    def call():
        for p in range(e.P):                 # learn() clears the counters only; the rows stay
            e.set_cursor(p, 0, T)
        learn(T, MB, K, **KW)
    return call


def _torch_call(P, rows):
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from torch.distributions import Normal
    dev = torch.device("cuda")
    torch.manual_seed(0)
    R = {k: torch.as_tensor(v, device=dev) for k, v in rows.items()}

    class Net(nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.l1, self.l2, self.l3 = nn.Linear(i, H), nn.Linear(H, H), nn.Linear(H, o)
            self.log_std = nn.Parameter(torch.zeros(1, o))

        def forward(self, x):
            x = F.layer_norm(x, x.size()[1:])
            x = F.layer_norm(F.relu(self.l1(x)), (H,))
            x = F.layer_norm(F.relu(self.l2(x)), (H,))
            return self.l3(x)
    actors = [[Net(O, A).to(dev) for _ in range(NA)] for _ in range(P)]
    critics = [[Net(NA * O, 1).to(dev) for _ in range(NA)] for _ in range(P)]
    aopt = [[torch.optim.Adam(actors[p][i].parameters(), lr=LR, eps=1e-5) for i in range(NA)] for p in range(P)]
    copt = [[torch.optim.Adam(critics[p][i].parameters(), lr=LR, eps=1e-5) for i in range(NA)] for p in range(P)]
    huber = lambda e: torch.where(e.abs() <= DELTA, e * e / 2, DELTA * (e.abs() - DELTA / 2))

    def learn(p):
        cobs = lambda key, ix=slice(None): R[key][p, ix].reshape(-1, NA * O)
        dist_of = lambda a, ix=slice(None): Normal(torch.tanh(a(R["obs"][p, ix, i])), torch.exp(a.log_std.clamp(-20, 2)))
        with torch.no_grad():
            vs = torch.cat([critics[p][i](cobs("obs")) for i in range(NA)], dim=1)
            vs_ = torch.cat([critics[p][i](cobs("nobs")) for i in range(NA)], dim=1)
            td = R["rew"][p] + HYPER["gamma"] * (1 - R["done"][p]) * vs_ - vs
            adv, gae = torch.zeros(T, NA, device=dev), 0
            for t in reversed(range(T)):
                gae = td[t] + HYPER["gamma"] * HYPER["lmbda"] * gae * (1 - R["adv_done"][p, t])
                adv[t] = gae
            vt = adv + vs
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        factor = torch.ones(T, 1, device=dev)
        for pos, i in enumerate(torch.randperm(NA).tolist()):
            a = actors[p][i]
            if pos != NA - 1:
                with torch.no_grad():
                    old = dist_of(a).log_prob(R["act"][p, :, i]).sum(1, keepdim=True)
            for _ in range(K):
                perm = torch.randperm(T, device=dev)
                for s in range(0, T, MB):
                    ix = perm[s:s + MB]
                    dist = dist_of(a, ix)
                    ratio = torch.exp(dist.log_prob(R["act"][p, ix, i]).sum(1, keepdim=True) - R["logp"][p, ix, i].sum(1, keepdim=True))
                    aloss = -(factor[ix] * torch.min(ratio * adv[ix], ratio.clamp(1 - HYPER["clip"], 1 + HYPER["clip"]) * adv[ix])).mean() \
                        - HYPER["ent_coef"] * dist.entropy().sum(1).mean()
                    aopt[p][i].zero_grad()
                    aloss.backward()
                    nn.utils.clip_grad_norm_(a.parameters(), 0.5)
                    aopt[p][i].step()
                    v = critics[p][i](cobs("obs", ix)).repeat(1, NA)
                    y = vt[ix]
                    closs = torch.max(huber(y - v).mean(), huber(y.clamp(v - HYPER["clip"], v + HYPER["clip"]) - v).mean())
                    copt[p][i].zero_grad()
                    closs.backward()
                    nn.utils.clip_grad_norm_(critics[p][i].parameters(), 0.5)
                    copt[p][i].step()
            if pos != NA - 1:
                with torch.no_grad():
                    factor = factor * torch.exp(dist_of(a).log_prob(R["act"][p, :, i]).sum(1, keepdim=True) - old)

    def call():
        for p in range(P):
            learn(p)
    return call, torch.cuda.synchronize


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    for P in ps:
        rows = _rows(P, 2)
        eh, em = _engine(N.ALGO_HAPPO, P, rows), _engine(N.ALGO_MAPPO, P, rows)
        sides = [("happo_hip", _hip_call(eh, eh.happo_learn), eh.sync, 10 if P == 1 else 5),
                 ("mappo_hip", _hip_call(em, em.mappo_learn), em.sync, 10 if P == 1 else 5)]
        if with_torch:
            call, sync = _torch_call(P, rows)
            sides.append(("happo_torch_eager", call, sync, 3 if P == 1 else 1))
        total = {s[0]: 0.0 for s in sides}
        for _, fn, sync, _n in sides:
            _block(sync, fn, 1)                                  # warm-up
        for _ in range(BLOCKS):                                  # the sides alternately
            for side, fn, sync, n in sides:
                total[side] += _block(sync, fn, n)
        ms = {side: 1e3 * total[side] / (BLOCKS * n) for side, _fn, _sync, n in sides}
        for side, _fn, _sync, n in sides:
            e = dict(happo_hip=eh, mappo_hip=em).get(side)
            print(json.dumps(dict(algo="happo", side=side, P=P, agents=NA, obs=O, act=A, hidden=H, horizon=T, minibatch=MB, k_epochs=K,
                                  calls=BLOCKS * n, call_ms=round(ms[side], 3), ratio_to_mappo_hip=round(ms[side] / ms["mappo_hip"], 3),
                                  finite=all(np.isfinite(e.get_params(net)).all() for net in range(e.n_nets)) if e else None,
                                  lds_rc=e.lds_bytes() if e else None)), flush=True)
        eh.close()
        em.close()


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
