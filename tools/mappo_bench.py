"""Time of one MAPPO / IPPO `learn()` (kernels_mappo.hip) at the reference scripts' shape:

  3 agents x (18 obs, 5 continuous actions), hidden 128, horizon 256 in one minibatch of 256, K_epochs 15, every trick on

Per engine kind and population P: `frl_mappo_learn` with device-drawn permutations, and beside it the same update written with torch
on the same device, eager — the restatement of `MAPPO.learn` / `IPPO.learn` (MAPPO_file/MAPPO.py:357-482, IPPO.py:252-322: the value
pass, the GAE loop over the horizon on device tensors, K x minibatch actor and critic steps per agent), P learners one after the other,
rows already on the device.  The two sides run ALTERNATELY, block by block, in this one command; a block is a few calls between two
synchronisations (host clock), after a warm-up call of each side.  An eager call is 90 backward passes per learner, so its blocks are
short: the call counts are printed with every figure.  Prints one JSON line per (kind, P, side).
    python tools/mappo_bench.py [--no-torch] [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

NA, O, A, H, T, MB, K = 3, 18, 5, 128, 256, 256, 15
HYPER = dict(gamma=0.95, lmbda=0.95, clip=0.2, ent_coef=0.01)
LR, DELTA, BLOCKS = 1e-3, 10.0, 3


def _rows(P, seed):
    g = np.random.default_rng(seed)
    obs = g.standard_normal((P, T, NA, O)).astype(np.float32)
    return dict(obs=obs, nobs=(obs + 0.3 * g.standard_normal(obs.shape)).astype(np.float32),
                act=(0.8 * g.standard_normal((P, T, NA, A))).astype(np.float32), logp=(-1 + 0.3 * g.standard_normal((P, T, NA, A))).astype(np.float32),
                rew=g.standard_normal((P, T, NA)).astype(np.float32), done=np.zeros((P, T, NA), np.float32),
                adv_done=(np.arange(T) % 25 == 24).astype(np.float32)[None, :, None].repeat(P, 0).repeat(NA, 2))


def _engine(kind, P, rows):
    e = Engine(N.ALGO_MAPPO if kind == "mappo" else N.ALGO_IPPO, [O] * NA, [A] * NA, T, n_learners=P, hidden=H, batch_max=MB, extra_cols=NA * A + NA)
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


def _hip_call(kind, e):
    kw = dict(HYPER, actor_lr=LR, adv_norm=True, value_clip=True, huber_delta=DELTA)
    kw.update(dict(critic_lr=LR, adam_eps=1e-5, clip_norm=0.0) if kind == "mappo" else dict(critic_lr=LR, adam_eps=1e-5, clip_norm=0.5))

    def call():
        for p in range(e.P):                 # learn() clears the counters only; the rows stay
            e.set_cursor(p, 0, T)
        e.mappo_learn(T, MB, K, **kw)
    return call


def _torch_call(kind, P, rows):
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
    cin = NA * O if kind == "mappo" else O
    actors = [[Net(O, A).to(dev) for _ in range(NA)] for _ in range(P)]
    critics = [[Net(cin, 1).to(dev) for _ in range(NA)] for _ in range(P)]
    if kind == "mappo":
        opts = [[(torch.optim.Adam(list(actors[p][i].parameters()) + list(critics[p][i].parameters()), lr=LR, eps=1e-5),) for i in range(NA)] for p in range(P)]
    else:
        opts = [[(torch.optim.Adam(actors[p][i].parameters(), lr=LR, eps=1e-5), torch.optim.Adam(critics[p][i].parameters(), lr=LR, eps=1e-5))
                 for i in range(NA)] for p in range(P)]
    huber = lambda e: torch.where(e.abs() <= DELTA, e * e / 2, DELTA * (e.abs() - DELTA / 2))

    def learn(p):
        cobs = lambda key, i, ix=slice(None): R[key][p, ix].reshape(-1, NA * O) if kind == "mappo" else R[key][p, ix, i]
        with torch.no_grad():
            vs = torch.cat([critics[p][i](cobs("obs", i)) for i in range(NA)], dim=1)
            vs_ = torch.cat([critics[p][i](cobs("nobs", i)) for i in range(NA)], dim=1)
            td = R["rew"][p] + HYPER["gamma"] * (1 - R["done"][p]) * vs_ - vs
            adv, gae = torch.zeros(T, NA, device=dev), 0
            for t in reversed(range(T)):
                gae = td[t] + HYPER["gamma"] * HYPER["lmbda"] * gae * (1 - R["adv_done"][p, t])
                adv[t] = gae
            vt = adv + vs
            adv = (adv - adv.mean()) / (adv.std() + 1e-8) if kind == "mappo" else (adv - adv.mean(0)) / (adv.std(0) + 1e-8)
        for i in range(NA):
            cols = slice(None) if kind == "mappo" else slice(i, i + 1)
            for _ in range(K):
                perm = torch.randperm(T, device=dev)
                for s in range(0, T, MB):
                    ix = perm[s:s + MB]
                    a = actors[p][i]
                    dist = Normal(torch.tanh(a(R["obs"][p, ix, i])), torch.exp(a.log_std.clamp(-20, 2)))
                    ratio = torch.exp(dist.log_prob(R["act"][p, ix, i]).sum(1, keepdim=True) - R["logp"][p, ix, i].sum(1, keepdim=True))
                    A_ = adv[ix][:, cols]
                    aloss = -torch.min(ratio * A_, ratio.clamp(1 - HYPER["clip"], 1 + HYPER["clip"]) * A_).mean() - HYPER["ent_coef"] * dist.entropy().sum(1).mean()
                    v = critics[p][i](cobs("obs", i, ix)).repeat(1, A_.shape[1])
                    y = vt[ix][:, cols]
                    closs = torch.max(huber(y - v).mean(), huber(y.clamp(v - HYPER["clip"], v + HYPER["clip"]) - v).mean())
                    for o in opts[p][i]:
                        o.zero_grad()
                    aloss.backward()
                    closs.backward()
                    if kind == "ippo":
                        nn.utils.clip_grad_norm_(a.parameters(), 0.5)
                        nn.utils.clip_grad_norm_(critics[p][i].parameters(), 0.5)
                    for o in opts[p][i]:
                        o.step()

    def call():
        for p in range(P):
            learn(p)
    return call, torch.cuda.synchronize


def _block(sync, fn, n):
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return time.perf_counter() - t0


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    for kind in ("mappo", "ippo"):
        for P in ps:
            rows = _rows(P, 2)
            e = _engine(kind, P, rows)
            sides = [("hip", _hip_call(kind, e), e.sync, 20 if P == 1 else 5)]
            if with_torch:
                call, sync = _torch_call(kind, P, rows)
                sides.append(("torch_eager", call, sync, 3 if P == 1 else 1))
            total = {s[0]: 0.0 for s in sides}
            for _, fn, sync, _n in sides:
                _block(sync, fn, 1)                                  # warm-up
            for _ in range(BLOCKS):                                  # the two sides alternately
                for side, fn, sync, n in sides:
                    total[side] += _block(sync, fn, n)
            finite = all(np.isfinite(e.get_params(net)).all() for net in range(e.n_nets))
            for side, _fn, _sync, n in sides:
                ms = 1e3 * total[side] / (BLOCKS * n)
                print(json.dumps(dict(algo=kind, side=side, P=P, agents=NA, obs=O, act=A, hidden=H, horizon=T, minibatch=MB, k_epochs=K,
                                      calls=BLOCKS * n, call_ms=round(ms, 3), steps_per_s=round(P * NA * K * 2 / ms * 1e3, 1),
                                      finite=finite if side == "hip" else None, lds_rc=e.lds_bytes() if side == "hip" else None)), flush=True)
            e.close()


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
