"""Envelope multi-objective DDPG (ENVELOPE_MORL_file/ENVELOPE_DDPG.py:40-320) restated in NumPy, and the seeded inputs of its
golden cases.  The golden generator (tests/golden/make_envelope_ddpg_golden.py) runs the reference on exactly these inputs; the CPU
test holds this oracle to its output and the GPU test holds the HIP engine to both.

One learn() trains on N = B W rows: row j is sample idx[j % B] (tensor.repeat(W, 1)) under preference w[j // B]
(np.repeat(B, axis=0)).  `dtype=np.float64` runs the same arithmetic in float64 (the float64 mode).

Kept as the reference has them: the TD target's a' comes from the ONLINE actor (:284); the actor's loss is the plain mean of the
critic's R outputs, not weighted by w (:303); both gradient clips run after backward() and do clip (:105-115); actor_target is
maintained and never read.
"""
import numpy as np

from oracle import nn
from tests.golden import synth

F32 = np.float32

# (O, A, R, H, B, W) as the issue lists them; 8 learn() calls per case on a table that is the ring (no wrap)
CASES = {
    "o5_a3_r2": dict(obs_dim=5, act_dim=3, rdim=2, hidden=32, batch=16, weight_num=4, seed=8100),
    "o8_a2_r3_h256": dict(obs_dim=8, act_dim=2, rdim=3, hidden=256, batch=32, weight_num=8, seed=8200),     # the reference's width
    # the critic's head scaled up until the actor's gradient norm passes the clip at 0.5 (found with this oracle; at the default
    # init the actor's norm is 0.002-0.05 and its clip never acts)
    "scaled_head": dict(obs_dim=5, act_dim=3, rdim=2, hidden=32, batch=16, weight_num=4, seed=8300, critic_head_scale=20.0),
}
COMMON = dict(n_table=120, n_learn=8, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, beta=0.95, done_p=0.05)
# the class case: ENVELOPE_DDPG's host side (priorities, the homotopy on beta, prioritised draws, select_action) on a ring of 40
# rows that wraps: 70 add() calls, a learn() every 5 steps from step 30 on (8 calls, the last four on the wrapped ring)
CLASS = dict(obs_dim=4, act_dim=2, rdim=2, hidden=32, batch=8, weight_num=3, seed=8900, capacity=40, n_steps=70, learn_from=30,
             learn_every=5, beta=0.9, max_episodes=20, done_p=0.1)
CLIP = 0.5
NAMES = ["l1", "l2", "l3"]


def case(name):
    c = dict(COMMON)
    c.update(CLASS if name == "class" else CASES[name])
    return c


def actor_layers(c):
    H, O, A, R = c["hidden"], c["obs_dim"], c["act_dim"], c["rdim"]
    return [("l1", H, O + R), ("l2", H, H), ("l3", A, H)]


def critic_layers(c):
    H, O, A, R = c["hidden"], c["obs_dim"], c["act_dim"], c["rdim"]
    return [("l1", H, O + A + R), ("l2", H, H), ("l3", R, H)]


def table(seed, n, c):
    """obs, next_obs ~ N(0,1), act ~ U(-1,1) [n, A], reward vectors ~ N(0,1) [n, R], done ~ Bernoulli(done_p)."""
    g = np.random.default_rng(seed)
    obs = g.standard_normal((n, c["obs_dim"])).astype(F32)
    next_obs = g.standard_normal((n, c["obs_dim"])).astype(F32)
    act = g.uniform(-1, 1, (n, c["act_dim"])).astype(F32)
    rew = g.standard_normal((n, c["rdim"])).astype(F32)
    done = g.random(n) < c["done_p"]
    return dict(obs=obs, act=act, rew=rew, next_obs=next_obs, done=done)


def weights(seed, weight_num, rdim):
    """np.abs(randn) / L1 norm in float64, cast to float32 (:269-271), from a PCG64 stream."""
    w = np.random.default_rng(seed).standard_normal((weight_num, rdim))
    return (np.abs(w) / np.linalg.norm(w, ord=1, axis=1, keepdims=True)).astype(F32)


def inputs(c, n_learn=None, seed=None):
    """Both nets' parameters (PCG64), the transition table and every call's sample indices and preference vectors."""
    s = c["seed"] if seed is None else seed
    calls = c["n_learn"] if n_learn is None else n_learn
    n = c.get("n_steps", c["n_table"])
    critic = synth.mlp_params(s + 1, critic_layers(c))
    scale = c.get("critic_head_scale")
    if scale:
        critic["l3.weight"] = (critic["l3.weight"] * F32(scale)).astype(F32)
    return dict(actor=synth.mlp_params(s, actor_layers(c)), critic=critic, table=table(s + 2, n, c),
                idx=[synth.indices(s + 100 + i, n, c["batch"]) for i in range(calls)],
                weights=[weights(s + 200 + i, c["weight_num"], c["rdim"]) for i in range(calls)])


def clip_grad_norm(grads, max_norm, dt):
    """torch.nn.utils.clip_grad_norm_: the L2 norm of the per-tensor L2 norms, coef = max_norm / (total + 1e-6) capped at 1.
    -> the pre-clip norm; `grads` scaled in place."""
    norms = np.array([np.sqrt(np.sum(g.astype(dt) ** 2, dtype=dt)) for g in grads.values()], dtype=dt)
    total = np.sqrt(np.sum(norms ** 2, dtype=dt))
    coef = min(dt(max_norm) / (total + dt(1e-6)), dt(1.0))
    for k in grads:
        grads[k] = grads[k] * dt(coef)
    return float(total)


class EnvelopeDDPG:
    """One learner: actor l1..l3 on [obs | w] (tanh head), critic l1..l3 on [obs | act | w] (R linear outputs), a deep-copied
    target of each, Adam (torch defaults) behind a global-norm clip at 0.5 for each, soft update of both targets on every call."""

    def __init__(self, actor, critic, obs_dim, act_dim, rdim, actor_lr, critic_lr, capacity, dtype=F32):
        self.O, self.A, self.R, self.dt = obs_dim, act_dim, rdim, dtype
        cp = lambda p: {k: np.array(v, dtype=dtype) for k, v in p.items()}
        self.actor, self.actor_t, self.critic, self.critic_t = cp(actor), cp(actor), cp(critic), cp(critic)
        self.anet = nn.MLP(NAMES, out_act="tanh")
        self.cnet = nn.MLP(NAMES)
        self.aopt = nn.Adam(self.actor, actor_lr)
        self.copt = nn.Adam(self.critic, critic_lr)
        self.capacity = capacity
        self.obs = np.zeros((capacity, obs_dim), dtype)
        self.act = np.zeros((capacity, act_dim), dtype)
        self.rew = np.zeros((capacity, rdim), dtype)
        self.nobs = np.zeros((capacity, obs_dim), dtype)
        self.done = np.zeros(capacity, dtype)
        self.index = self.size = 0
        self.critic_norms, self.actor_norms = [], []          # pre-clip gradient norms, one per learn_with()

    def add(self, obs, act, rew, nobs, done):
        i = self.index
        self.obs[i], self.act[i], self.rew[i], self.nobs[i], self.done[i] = obs, act, rew, nobs, float(done)
        self.index = (i + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def pi(self, p, obs, w):
        return self.anet.forward(p, np.concatenate([obs, w], axis=1).astype(self.dt))

    def q(self, p, obs, act, w):
        return self.cnet.forward(p, np.concatenate([obs, act, w], axis=1).astype(self.dt))

    # ---- the class's host side
    def choose(self, obs, pref):
        """actor(obs, w) (select_action / evaluate_action, :143-180) -> the action [A]"""
        return self.pi(self.actor, np.asarray(obs, self.dt).reshape(1, -1), np.asarray(pref, self.dt).reshape(1, -1))[0][0]

    def priority(self, obs, act, rew, nobs, done, gamma, pref):
        """|w.r + gamma w.critic(s', actor(s', w), w) - w.critic(s, a, w)| + 1e-5 on the online nets, and |w.r - w.Q| + 1e-5 on
        done (:201-236)"""
        dt = self.dt
        w = np.asarray(pref, dt)
        w1 = w.reshape(1, -1)
        wq = w @ self.q(self.critic, np.asarray(obs, dt).reshape(1, -1), np.asarray(act, dt).reshape(1, -1), w1)[0][0]
        wr = w @ np.asarray(rew, dt)
        if done:
            return abs(wr - wq) + 1e-5
        n1 = np.asarray(nobs, dt).reshape(1, -1)
        hq = self.q(self.critic, n1, self.pi(self.actor, n1, w1)[0], w1)[0][0]
        return abs(wr + dt(gamma) * (w @ hq) - wq) + 1e-5

    # ---- learn
    def learn_with(self, idx, w, gamma, tau, beta):
        """One learn() on the rows `idx` [B] under the preferences `w` [W, R]; -> (critic loss, actor loss); the pre-clip gradient
        norms are appended to critic_norms / actor_norms."""
        dt = self.dt
        idx = np.asarray(idx, np.int64)
        B, W = idx.size, len(w)
        N = B * W
        rows = np.tile(idx, W)                                          # row j: sample idx[j % B]
        wr = np.repeat(np.asarray(w, dt), B, axis=0)                    # ... under w[j // B]
        rew, done = self.rew[rows], self.done[rows][:, None]
        # a' = actor(s', w) (ONLINE), T = r + gamma critic_target(s', a', w) (1 - done) (:284-287)
        a2, _ = self.pi(self.actor, self.nobs[rows], wr)
        qt, _ = self.q(self.critic_t, self.nobs[rows], a2, wr)
        T = rew + dt(gamma) * qt * (dt(1) - done)
        # Q = critic(s, a, w); loss = beta mse(w.Q, w.T) + (1 - beta) mse(Q, T) (:290-297)
        Q, acts = self.q(self.critic, self.obs[rows], self.act[rows], wr)
        d = np.sum(Q * wr, axis=1, dtype=dt) - np.sum(T * wr, axis=1, dtype=dt)
        E = Q - T
        closs = dt(beta) * np.mean(d * d, dtype=dt) + dt(1 - beta) * np.mean(E * E, dtype=dt)
        dQ = dt(beta) * dt(2.0 / N) * d[:, None] * wr + dt(1 - beta) * dt(2.0 / (N * self.R)) * E
        _, g = self.cnet.backward(self.critic, acts, dQ, need_dx=False)
        g = {k: g[k] for k in self.critic}
        self.critic_norms.append(clip_grad_norm(g, CLIP, dt))
        self.copt.step(self.critic, g)
        # actor: loss = -mean_{j,k} critic(s, actor(s, w), w)_k through the updated critic (:302-304)
        a, aacts = self.pi(self.actor, self.obs[rows], wr)
        Q2, cacts = self.q(self.critic, self.obs[rows], a, wr)
        aloss = -np.mean(Q2, dtype=dt)
        dx, _ = self.cnet.backward(self.critic, cacts, np.full((N, self.R), dt(-1.0 / (N * self.R)), dt), need_dx=True)
        _, ga = self.anet.backward(self.actor, aacts, dx[:, self.O:self.O + self.A], need_dx=False)
        ga = {k: ga[k] for k in self.actor}
        self.actor_norms.append(clip_grad_norm(ga, CLIP, dt))
        self.aopt.step(self.actor, ga)
        nn.soft_update(self.critic_t, self.critic, tau)
        nn.soft_update(self.actor_t, self.actor, tau)
        return dt(closs), dt(aloss)


def make(c, inp, dtype=F32):
    t = inp["table"]
    o = EnvelopeDDPG(inp["actor"], inp["critic"], c["obs_dim"], c["act_dim"], c["rdim"], c["actor_lr"], c["critic_lr"],
                     c.get("capacity", len(t["done"])), dtype)
    if "capacity" not in c:             # the table is the ring
        for i in range(len(t["done"])):
            o.add(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]))
    return o


def run(c, inp, n_learn=None, dtype=F32):
    """-> (oracle, critic losses [calls], actor losses [calls])"""
    o = make(c, inp, dtype)
    out = [o.learn_with(inp["idx"][i], inp["weights"][i], c["gamma"], c["tau"], c["beta"])
           for i in range(c["n_learn"] if n_learn is None else n_learn)]
    return o, np.array([x[0] for x in out], dtype=dtype), np.array([x[1] for x in out], dtype=dtype)


def class_schedule(c):
    """The class case's script: per step `select_action(obs)`, `add(...)` of the table's transition, and a learn() every
    `learn_every` steps from `learn_from` on -> list of the steps after whose add() a learn() runs."""
    return [t for t in range(c["n_steps"]) if t + 1 >= c["learn_from"] and (t + 1 - c["learn_from"]) % c["learn_every"] == 0][:c["n_learn"]]
