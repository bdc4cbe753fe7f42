"""Discrete SAC (SAC_file/SAC_add_discrete.py:179-348, the `hands_on` nets) restated in NumPy, and the seeded inputs
of its golden cases.  The golden generator (tests/golden/make_sacd_golden.py) runs the reference on exactly these
inputs; the CPU test holds this oracle to its output and the GPU test holds the HIP engine to both.
"""
import numpy as np

from oracle import nn
from oracle.buffer import Buffer
from oracle.normalization import NormalizationBatch
from tests.golden import synth

F32 = np.float32

# 25 learn() calls per case; the table is the ring (no wrap), one np.random.choice draw per call
CASES = {
    "o4_a2": dict(obs_dim=4, n_act=2, batch=64, hidden=128, bn=False, seed=7100),
    "o8_a4_bn": dict(obs_dim=8, n_act=4, batch=256, hidden=128, bn=True, seed=7200),
    "o11_a20": dict(obs_dim=11, n_act=20, batch=200, hidden=128, bn=False, seed=7300),
    "o6_a3_h256": dict(obs_dim=6, n_act=3, batch=128, hidden=256, bn=False, seed=7400),
}
COMMON = dict(n_table=600, n_learn=25, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=3e-4, alpha0=0.01, alpha_lr=1e-4)
LONG = dict(obs_dim=8, n_act=4, batch=256, hidden=128, bn=False, seed=7500, n_learn=200)


def case(name):
    c = dict(COMMON)
    c.update(LONG if name == "long" else CASES[name])
    return c


def actor_layers(c):
    H, O, A = c["hidden"], c["obs_dim"], c["n_act"]
    return [("l1", H, O), ("l2", H, H), ("l3", A, H)]


def critic_layers(c):
    H, O, A = c["hidden"], c["obs_dim"], c["n_act"]
    return [("l1", H, O), ("l2", H, H), ("l3", A, H), ("l4", H, O), ("l5", H, H), ("l6", A, H)]


def inputs(c, n_learn=None, table_size=None):
    """Parameters (PCG64), the transition table and the per-call sample indices of a case."""
    n = table_size or c["n_table"]
    calls = c["n_learn"] if n_learn is None else n_learn
    s = c["seed"]
    return dict(actor=synth.mlp_params(s, actor_layers(c)), critic=synth.mlp_params(s + 1, critic_layers(c)),
                table=synth.transitions(s + 2, n, c["obs_dim"], 1, n_discrete=c["n_act"]),
                idx=[synth.indices(s + 100 + i, n, c["batch"]) for i in range(calls)])


def softmax(z):
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m).astype(F32)
    return (e * (F32(1) / e.sum(axis=1, keepdims=True, dtype=F32))).astype(F32)


class SACDiscrete:
    """One learner: actor l1..l3 (softmax head), critic l1..l6 (two heads on obs only), deep-copied targets, Adam with
    clip_grad_norm_(0.5) on both nets, adaptive alpha (alpha0 0.01, Adam lr 1e-4, target 0.6 * -log(1/A))."""

    def __init__(self, actor_p, critic_p, obs_dim, n_act, actor_lr, critic_lr, capacity, alpha0=0.01, alpha_lr=1e-4,
                 batch_obs_norm=False):
        self.A = n_act
        self.bn = NormalizationBatch(obs_dim) if batch_obs_norm else None
        self.actor, self.actor_t = nn.copy_params(actor_p), nn.copy_params(actor_p)
        self.critic, self.critic_t = nn.copy_params(critic_p), nn.copy_params(critic_p)
        self.pi = nn.MLP(["l1", "l2", "l3"])
        self.q1, self.q2 = nn.MLP(["l1", "l2", "l3"]), nn.MLP(["l4", "l5", "l6"])
        self.actor_opt = nn.Adam(self.actor, actor_lr)
        self.critic_opt = nn.Adam(self.critic, critic_lr)
        self.alpha_p = {"log_alpha": np.array(np.log(alpha0), dtype=F32)}
        self.alpha_opt = nn.Adam(self.alpha_p, alpha_lr)
        self.alpha = F32(np.exp(self.alpha_p["log_alpha"]))
        self.target_entropy = F32(0.6) * -np.log(F32(1.0) / F32(n_act), dtype=F32)
        self.buffer = Buffer(capacity, obs_dim, 1)

    def add(self, *a):
        self.buffer.add(*a)

    def probs(self, p, x):
        z, acts = self.pi.forward(p, x)
        return softmax(z), acts

    def learn_with(self, idx, gamma, tau):
        """One learn() on the rows `idx`; returns (critic_loss, actor_loss, alpha_loss)."""
        obs, act, rew, nobs, done = self.buffer.sample(idx)
        if self.bn is not None:                         # sample(): :276-285
            obs = self.bn(obs)
            nobs = self.bn(nobs, update=False)
        B = obs.shape[0]
        a = act.reshape(-1).astype(np.int64)
        rows = np.arange(B)
        # target (:294-306): the ONLINE actor on s', the target critic
        pn, _ = self.probs(self.actor, nobs)
        ent_n = -np.sum(pn * np.log(pn + F32(1e-8)), axis=1, keepdims=True, dtype=F32)
        v1t, _ = self.q1.forward(self.critic_t, nobs)
        v2t, _ = self.q2.forward(self.critic_t, nobs)
        vn = np.sum(pn * np.minimum(v1t, v2t), axis=1, keepdims=True, dtype=F32)
        y = rew.reshape(-1, 1) + F32(gamma) * (F32(1) - done.reshape(-1, 1)) * (vn + self.alpha * ent_n)
        # critic (:310-314)
        v1, c1 = self.q1.forward(self.critic, obs)
        v2, c2 = self.q2.forward(self.critic, obs)
        e1, e2 = v1[rows, a][:, None] - y, v2[rows, a][:, None] - y
        closs = F32(np.mean(e1 * e1, dtype=F32) + np.mean(e2 * e2, dtype=F32))
        d1, d2 = np.zeros_like(v1), np.zeros_like(v2)
        d1[rows, a] = (e1 * F32(2.0 / B))[:, 0]
        d2[rows, a] = (e2 * F32(2.0 / B))[:, 0]
        _, g1 = self.q1.backward(self.critic, c1, d1, need_dx=False)
        _, g2 = self.q2.backward(self.critic, c2, d2, need_dx=False)
        g = {**g1, **g2}
        g = {k: g[k] for k in self.critic}
        nn.clip_grad_norm(g, 0.5)
        self.critic_opt.step(self.critic, g)
        # actor (:319-330) with the updated critic
        p, acts = self.probs(self.actor, obs)
        logp = np.log(p + F32(1e-8))
        ent = -np.sum(p * logp, axis=1, keepdims=True, dtype=F32)
        m = np.minimum(self.q1.forward(self.critic, obs)[0], self.q2.forward(self.critic, obs)[0])
        q = np.sum(p * m, axis=1, keepdims=True, dtype=F32)
        aloss = F32(np.mean(-q - self.alpha * ent, dtype=F32))
        gp = (-m + self.alpha * (logp + p / (p + F32(1e-8)))) * F32(1.0 / B)
        dz = p * (gp - np.sum(p * gp, axis=1, keepdims=True, dtype=F32))
        _, ga = self.pi.backward(self.actor, acts, dz.astype(F32), need_dx=False)
        ga = {k: ga[k] for k in self.actor}
        nn.clip_grad_norm(ga, 0.5)
        self.actor_opt.step(self.actor, ga)
        nn.soft_update(self.critic_t, self.critic, tau)
        nn.soft_update(self.actor_t, self.actor, tau)
        # alpha (:333-336): H detached
        mean_term = F32(np.mean(ent - self.target_entropy, dtype=F32))
        alpha_loss = F32(self.alpha * mean_term)
        self.alpha_opt.step(self.alpha_p, {"log_alpha": np.array(self.alpha * mean_term, dtype=F32)})
        self.alpha = F32(np.exp(self.alpha_p["log_alpha"]))
        return closs, aloss, alpha_loss


def make(c, inp):
    o = SACDiscrete(inp["actor"], inp["critic"], c["obs_dim"], c["n_act"], c["actor_lr"], c["critic_lr"],
                    len(inp["table"]["rew"]), c["alpha0"], c["alpha_lr"], batch_obs_norm=c["bn"])
    t = inp["table"]
    for i in range(len(t["rew"])):
        o.add(t["obs"][i], t["act"][i], float(t["rew"][i]), t["next_obs"][i], bool(t["done"][i]))
    return o


def run(c, inp, n_learn=None):
    """-> (oracle, losses [calls, 3], alphas [calls])"""
    o = make(c, inp)
    losses, alphas = [], []
    for i in range(c["n_learn"] if n_learn is None else n_learn):
        losses.append(o.learn_with(inp["idx"][i], c["gamma"], c["tau"]))
        alphas.append(o.alpha)
    return o, np.array(losses, dtype=F32), np.array(alphas, dtype=F32)
