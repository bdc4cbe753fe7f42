"""MAPPO_attention's critic and whole `learn()` in torch on the CPU, float64 by default, written from the method's description (ISSUE
"What the reference does"; DESIGN.md "MAPPO_attention"): autograd, clip_grad_norm_ and n torch.optim.Adam sharing one attention block.
Parameters, rows and permutations are injected; tests/test_gpu_mappo_attention.py runs the kernels on the same inputs."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import mappo_oracle as M

H, HEADS = 128, 4
ON = dict(M.TRICKS_ON)
OFF = dict(M.TRICKS_OFF)
CASES = {
    "pair": dict(dims=((7, 2),) * 2, cont=True, horizon=5, minibatch=5, k_epochs=2, trick=OFF, seed=51, actor_lr=1e-3, critic_lr=1e-3),
    "trio": dict(dims=((18, 5),) * 3, cont=True, horizon=40, minibatch=16, k_epochs=2, trick=ON, seed=52, actor_lr=1e-3, critic_lr=3e-3,
                 reward_scale=0.0125, value_scale=0.125),      # small values and rewards: the critics' gradient norms straddle the 0.5 clip
    "octet": dict(dims=((10, 3),) * 8, cont=False, horizon=33, minibatch=33, k_epochs=1, trick=dict(OFF, LayerNorm=True), seed=53,
                  actor_lr=1e-3, critic_lr=1e-3),
}
OWN = ("encoder_fc_s", "l1", "l3")
ATT = ("attention.query.weight", "attention.key.weight", "attention.value.0.weight", "attention.value.0.bias",
       "attention.fc_out.weight", "attention.fc_out.bias")


def case(name):
    return dict(dict(reward_scale=1.0, value_scale=1.0), **CASES[name], name=name, kind="ippo", hidden=H, gamma=0.95, lmbda=0.95, clip=0.2,
                ent_coef=0.01, huber_delta=10.0, reward_same=False, dead_agent=None)


def inputs(c, seed=None):
    """MAPPO's seeded actors and rows (tests/mappo_oracle.py) + attention critics and one block, float32 NumPy"""
    inp = M.inputs(dict(c, horizon=max(c["horizon"], 16)), seed)       # (its `done` rows need 16; `pair` keeps the first 5)
    inp["rows"] = [{k: v[:c["horizon"]] for k, v in r.items()} for r in inp["rows"]]
    rng = np.random.Generator(np.random.PCG64((c["seed"] if seed is None else seed) + 7))
    O = c["dims"][0][0]
    inp["critics"] = [M.net_params(rng, OWN, [(H, O), (H, 2 * H), (1, H)]) for _ in c["dims"]]
    for p in inp["critics"]:
        p["l3.weight"] *= np.float32(c["value_scale"])
        p["l3.bias"] *= np.float32(c["value_scale"])
    lin = lambda: M._linear(rng, H, H, scale=3.0)          # (wide enough that the softmax is far from uniform)
    (q, _), (k, _), (v, vb), (o, ob) = lin(), lin(), lin(), lin()
    inp["attention"] = dict(zip(ATT, (q, k, v, vb, o, ob)))
    return inp


def _ln(x, on):
    return F.layer_norm(x, x.shape[1:]) if on else x


class Oracle:
    def __init__(self, c, inp, dtype=torch.float64, device="cpu"):
        self.c, self.t, self.n, self.dt = c, c["trick"], len(c["dims"]), dtype
        P = lambda d: {k: torch.tensor(np.asarray(v), dtype=dtype, device=device, requires_grad=True) for k, v in d.items()}
        self.actors, self.critics, self.att = [P(p) for p in inp["actors"]], [P(p) for p in inp["critics"]], P(inp["attention"])
        self.rows = [{k: torch.tensor(v, dtype=dtype, device=device) for k, v in r.items()} for r in inp["rows"]]
        eps = 1e-5 if self.t["adam_eps"] else 1e-8
        self.aopt = [torch.optim.Adam(list(p.values()), lr=c["actor_lr"], eps=eps) for p in self.actors]
        self.cparams = [list(p.values()) + list(self.att.values()) for p in self.critics]
        self.copt = [torch.optim.Adam(ps, lr=c["critic_lr"], eps=eps) for ps in self.cparams]
        self.weights = []                                   # attention weights [rows, heads, n - 1] of every critic forward

    def value(self, i, obs):
        """obs: one [rows, O] per agent -> V_i [rows, 1]"""
        p, a, O = self.critics[i], self.att, self.c["dims"][0][0]
        s = _ln(torch.cat(list(obs), dim=1), self.t["feature_norm"])
        e = [F.linear(s[:, j * O:(j + 1) * O], p["encoder_fc_s.weight"], p["encoder_fc_s.bias"]) for j in range(self.n)]
        others = torch.stack([e[j] for j in range(self.n) if j != i], dim=1)                              # [rows, n - 1, H]
        heads = lambda x: x.reshape(x.shape[0], -1, HEADS, H // HEADS)
        q = heads(F.linear(e[i], a[ATT[0]]))                                                              # [rows, 1, heads, 32]
        k = heads(F.linear(others, a[ATT[1]]))
        v = heads(F.leaky_relu(F.linear(others, a[ATT[2]], a[ATT[3]]), 0.01))
        w = torch.softmax((q * k).sum(-1) / math.sqrt(H // HEADS), dim=1)                                 # [rows, n - 1, heads]
        self.weights.append(w.detach())
        att = F.linear((w.unsqueeze(-1) * v).sum(1).reshape(-1, H), a[ATT[4]], a[ATT[5]])
        x = _ln(F.relu(F.linear(torch.cat([e[i], att], dim=1), p["l1.weight"], p["l1.bias"])), self.t["LayerNorm"])
        return F.linear(x, p["l3.weight"], p["l3.bias"])

    def logp_entropy(self, i, ix):
        p, r, c = self.actors[i], self.rows[i], self.c
        names = M.actor_names(c)
        x = _ln(r["obs"][ix], self.t["feature_norm"])
        for nm in names[:2]:
            x = _ln(F.relu(F.linear(x, p[nm + ".weight"], p[nm + ".bias"])), self.t["LayerNorm"])
        z = F.linear(x, p[names[2] + ".weight"], p[names[2] + ".bias"])
        if c["cont"]:
            d = torch.distributions.Normal(torch.tanh(z), torch.exp(torch.clamp(p["log_std"], -20, 2)).expand_as(z))
            return d.log_prob(r["act"][ix]).sum(1, keepdim=True), d.entropy().sum(1, keepdim=True)
        d = torch.distributions.Categorical(probs=torch.softmax(z, dim=1))
        return d.log_prob(r["act"][ix].reshape(-1)).reshape(-1, 1), d.entropy().reshape(-1, 1)

    def learn(self, perm, independent=False):
        """perm [n][K][T] -> (losses, pre-clip norms), both [n][K * n_mb][2] (actor, critic).  independent: every agent's critic starts
        from the attention block as it stood before the call (what the method does NOT do: the order-dependence check)"""
        c, T, mb, n = self.c, self.c["horizon"], self.c["minibatch"], self.n
        obs, nobs = [r["obs"] for r in self.rows], [r["next_obs"] for r in self.rows]
        with torch.no_grad():
            vs = torch.cat([self.value(i, obs) for i in range(n)], dim=1)
            vs_ = torch.cat([self.value(i, nobs) for i in range(n)], dim=1)
            cat = lambda k: torch.cat([r[k] for r in self.rows], dim=1)
            td = cat("rew") + c["gamma"] * (1 - cat("done")) * vs_ - vs
            adv, gae = torch.zeros_like(td), 0
            for t in reversed(range(T)):
                gae = td[t] + c["gamma"] * c["lmbda"] * gae * (1 - cat("adv_done")[t])
                adv[t] = gae
            v_target = adv + vs
            if self.t["adv_norm"]:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            block0 = [x.detach().clone() for x in self.att.values()]
        huber = lambda e: torch.where(e.abs() <= c["huber_delta"], 0.5 * e * e, c["huber_delta"] * (e.abs() - 0.5 * c["huber_delta"]))
        loss_of = lambda y, v: huber(y - v).mean() if self.t["huber_loss"] else F.mse_loss(y, v)
        losses, norms = np.zeros((n, c["k_epochs"] * math.ceil(T / mb), 2)), np.zeros((n, c["k_epochs"] * math.ceil(T / mb), 2))

        def step(opt, params, loss):
            opt.zero_grad()
            loss.backward()
            g = float(torch.nn.utils.clip_grad_norm_(params, 0.5))
            opt.step()
            return float(loss.detach()), g
        for i in range(n):
            if independent:
                with torch.no_grad():
                    for x, x0 in zip(self.att.values(), block0):
                        x.copy_(x0)
            j = 0
            for k in range(c["k_epochs"]):
                for s in range(0, T, mb):
                    ix = torch.as_tensor(np.asarray(perm[i][k][s:s + mb]), dtype=torch.long, device=adv.device)
                    lp, ent = self.logp_entropy(i, ix)
                    ratio = torch.exp(lp - self.rows[i]["logp"][ix].sum(1, keepdim=True))
                    surr = torch.min(ratio * adv[ix], torch.clamp(ratio, 1 - c["clip"], 1 + c["clip"]) * adv[ix])
                    losses[i, j, 0], norms[i, j, 0] = step(self.aopt[i], list(self.actors[i].values()), -surr.mean() - c["ent_coef"] * ent.mean())
                    v = self.value(i, [o[ix] for o in obs]).repeat(1, n)
                    loss = loss_of(v_target[ix], v)
                    if self.t["ValueClip"]:
                        loss = torch.max(loss, loss_of(torch.clamp(v_target[ix], v - c["clip"], v + c["clip"]), v))
                    losses[i, j, 1], norms[i, j, 1] = step(self.copt[i], self.cparams[i], loss)
                    j += 1
        return losses, norms

    def flat(self, d, keys=None):
        return np.concatenate([d[k].detach().cpu().numpy().reshape(-1) for k in (keys or d)])

    def adam_m(self, opt):
        return np.concatenate([opt.state[p]["exp_avg"].numpy().reshape(-1) for p in opt.param_groups[0]["params"]])
