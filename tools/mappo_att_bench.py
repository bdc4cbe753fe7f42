"""Time of one MAPPO_attention `learn()` (kernels_mappo_att.hip, frl_mappo_att_learn) at the reference script's settings:

  n x (18 obs, 5 continuous actions) for n = 3 and n = 8, hidden 128, horizon 256 in one minibatch of 256, K_epochs 15, every trick on

Per shape and population P, run ALTERNATELY block by block in this one command (tools/mappo_bench.py's scheme: a block is a few calls
between two synchronisations, host clock, after a warm-up call of each side): `frl_mappo_att_learn`; `frl_mappo_learn` on a plain MAPPO
engine of the same shape, rows and Adam settings (the joint-observation critic, all agents side by side); and, at P = 1, the same update
in eager torch float32 on the same device (the restatement below; eager torch runs learners one after another, so P learners cost P
times that).  Prints one JSON line per (shape, P, side).
    python tools/mappo_att_bench.py [--no-torch] [P ...]      (default P = 1 64)
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402
from mappo_bench import A, DELTA, H, HYPER, K, LR, MB, O, T, _block  # noqa: E402

BLOCKS = 3
KW = dict(HYPER, actor_lr=LR, critic_lr=LR, adam_eps=1e-5, clip_norm=0.5, adv_norm=True, value_clip=True, huber_delta=DELTA)


def _rows(P, na, seed):
    g = np.random.default_rng(seed)
    obs = g.standard_normal((P, T, na, O)).astype(np.float32)
    return dict(obs=obs, nobs=(obs + 0.3 * g.standard_normal(obs.shape)).astype(np.float32),
                act=(0.8 * g.standard_normal((P, T, na, A))).astype(np.float32), logp=(-1 + 0.3 * g.standard_normal((P, T, na, A))).astype(np.float32),
                rew=g.standard_normal((P, T, na)).astype(np.float32), done=np.zeros((P, T, na), np.float32),
                adv_done=(np.arange(T) % 25 == 24).astype(np.float32)[None, :, None].repeat(P, 0).repeat(na, 2))


def _engine(algo, na, P, rows):
    e = Engine(algo, [O] * na, [A] * na, T, n_learners=P, hidden=H, batch_max=MB, extra_cols=na * A + na)
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


def _torch_call(na, rows):
    """learner 0's learn() in eager torch: the actors' clipped surrogate and the attention critics, agents as the outer loop"""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from torch.distributions import Normal
    dev = torch.device("cuda")
    torch.manual_seed(0)
    R = {k: torch.as_tensor(v[0], device=dev) for k, v in rows.items()}
    ln = lambda x: F.layer_norm(x, x.shape[1:])

    class Actor(nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.l2, self.l3, self.log_std = nn.Linear(O, H), nn.Linear(H, H), nn.Linear(H, A), nn.Parameter(torch.zeros(1, A))

        def forward(self, x):
            return torch.tanh(self.l3(ln(F.relu(self.l2(ln(F.relu(self.l1(ln(x)))))))))

    class Critic(nn.Module):
        def __init__(self, i, att):
            super().__init__()
            self.i, self.att, self.enc, self.l1, self.l3 = i, att, nn.Linear(O, H), nn.Linear(2 * H, H), nn.Linear(H, 1)

        def forward(self, obs):                  # obs [rows, na, O]
            s = ln(obs.reshape(obs.shape[0], -1)).reshape(obs.shape)
            e = self.enc(s)
            others = e[:, [j for j in range(na) if j != self.i]]
            hd = lambda x: x.reshape(x.shape[0], -1, 4, H // 4)
            q, k, v = hd(self.att["q"](e[:, self.i])), hd(self.att["k"](others)), hd(F.leaky_relu(self.att["v"](others), 0.01))
            w = torch.softmax((q * k).sum(-1) / (H // 4) ** 0.5, dim=1)
            x = torch.cat([e[:, self.i], self.att["o"]((w.unsqueeze(-1) * v).sum(1).reshape(-1, H))], dim=1)
            return self.l3(ln(F.relu(self.l1(x))))
    att = nn.ModuleDict(dict(q=nn.Linear(H, H, bias=False), k=nn.Linear(H, H, bias=False), v=nn.Linear(H, H), o=nn.Linear(H, H))).to(dev)
    actors, critics = [Actor().to(dev) for _ in range(na)], [Critic(i, att).to(dev) for i in range(na)]
    aopt = [torch.optim.Adam(a.parameters(), lr=LR, eps=1e-5) for a in actors]
    copt = [torch.optim.Adam(c.parameters(), lr=LR, eps=1e-5) for c in critics]
    huber = lambda e: torch.where(e.abs() <= DELTA, e * e / 2, DELTA * (e.abs() - DELTA / 2))

    def call():
        with torch.no_grad():
            vs = torch.cat([c(R["obs"]) for c in critics], dim=1)
            vs_ = torch.cat([c(R["nobs"]) for c in critics], dim=1)
            td = R["rew"] + HYPER["gamma"] * (1 - R["done"]) * vs_ - vs
            adv, gae = torch.zeros_like(td), 0
            for t in reversed(range(T)):
                gae = td[t] + HYPER["gamma"] * HYPER["lmbda"] * gae * (1 - R["adv_done"][t])
                adv[t] = gae
            vt = adv + vs
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        for i in range(na):
            for _ in range(K):
                perm = torch.randperm(T, device=dev)
                for s in range(0, T, MB):
                    ix = perm[s:s + MB]
                    dist = Normal(actors[i](R["obs"][ix, i]), torch.exp(actors[i].log_std.clamp(-20, 2)))
                    ratio = torch.exp(dist.log_prob(R["act"][ix, i]).sum(1, keepdim=True) - R["logp"][ix, i].sum(1, keepdim=True))
                    aloss = -torch.min(ratio * adv[ix], ratio.clamp(1 - HYPER["clip"], 1 + HYPER["clip"]) * adv[ix]).mean() \
                        - HYPER["ent_coef"] * dist.entropy().sum(1).mean()
                    aopt[i].zero_grad()
                    aloss.backward()
                    nn.utils.clip_grad_norm_(actors[i].parameters(), 0.5)
                    aopt[i].step()
                    v, y = critics[i](R["obs"][ix]).repeat(1, na), vt[ix]
                    closs = torch.max(huber(y - v).mean(), huber(y.clamp(v - HYPER["clip"], v + HYPER["clip"]) - v).mean())
                    copt[i].zero_grad()
                    closs.backward()
                    nn.utils.clip_grad_norm_(critics[i].parameters(), 0.5)
                    copt[i].step()
    return call, torch.cuda.synchronize


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    for na in (3, 8):
        for P in ps:
            rows = _rows(P, na, 2)
            ea, em = _engine(N.ALGO_MAPPO_ATT, na, P, rows), _engine(N.ALGO_MAPPO, na, P, rows)
            sides = [("mappo_att_hip", _hip_call(ea, ea.mappo_att_learn), ea.sync, 3 if P == 1 else 1),
                     ("mappo_hip", _hip_call(em, em.mappo_learn), em.sync, 10 if P == 1 else 5)]
            if with_torch and P == 1:
                call, sync = _torch_call(na, rows)
                sides.append(("mappo_att_torch_eager", call, sync, 1))
            total = {s[0]: 0.0 for s in sides}
            for _, fn, sync, _n in sides:
                _block(sync, fn, 1)                                  # warm-up
            for _ in range(BLOCKS):                                  # the sides alternately
                for side, fn, sync, n in sides:
                    total[side] += _block(sync, fn, n)
            ms = {side: 1e3 * total[side] / (BLOCKS * n) for side, _fn, _sync, n in sides}
            for side, _fn, _sync, n in sides:
                e = dict(mappo_att_hip=ea, mappo_hip=em).get(side)
                print(json.dumps(dict(algo="mappo_attention", side=side, P=P, agents=na, obs=O, act=A, hidden=H, horizon=T, minibatch=MB, k_epochs=K,
                                      calls=BLOCKS * n, call_ms=round(ms[side], 3), ratio_to_mappo_hip=round(ms[side] / ms["mappo_hip"], 3),
                                      finite=all(np.isfinite(e.get_params(net)).all() for net in range(e.n_nets)) if e else None,
                                      lds_rc=e.lds_bytes() if e else None)), flush=True)
            ea.close()
            em.close()


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
