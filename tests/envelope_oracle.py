"""Envelope multi-objective DQN (ENVELOPE_MORL_file/ENVELOPE_DQN.py:36-266) restated in NumPy, and the seeded inputs of its
golden cases.  The golden generator (tests/golden/make_envelope_golden.py) runs the reference on exactly these inputs; the CPU
test holds this oracle to its output and the GPU test holds the HIP engine to both.

One learn() trains on N = B W rows: row j is sample idx[j % B] (tensor.repeat(W, 1)) under preference w[j // B]
(np.repeat(B, axis=0)).  `dtype=np.float64` runs the same arithmetic in float64 (the float64 mode).
"""
import numpy as np

from oracle import nn
from tests.golden import synth

F32 = np.float32

# 8 learn() calls per case on a table that is the ring (no wrap); (O, A, R, H, B, W) as the issue lists them
CASES = {
    "o5_a3_r2": dict(obs_dim=5, n_act=3, rdim=2, hidden=32, batch=6, weight_num=3, seed=8100),        # N = 18: three weights in one partial chunk
    "o8_a4_r4": dict(obs_dim=8, n_act=4, rdim=4, hidden=48, batch=37, weight_num=5, seed=8200),       # N = 185: chunks straddle both boundaries
    "o2_a4_r2": dict(obs_dim=2, n_act=4, rdim=2, hidden=64, batch=64, weight_num=4, seed=8300),       # aligned
    "o11_a6_r3_h256": dict(obs_dim=11, n_act=6, rdim=3, hidden=256, batch=33, weight_num=3, seed=8400),
    "o6_a16_r4": dict(obs_dim=6, n_act=16, rdim=4, hidden=64, batch=16, weight_num=2, seed=8500),     # A R = 64, the widest head
    "beta0": dict(obs_dim=5, n_act=3, rdim=2, hidden=32, batch=12, weight_num=3, seed=8600, beta=0.0),
    "beta1": dict(obs_dim=5, n_act=3, rdim=2, hidden=32, batch=12, weight_num=3, seed=8700, beta=1.0),
    "done20": dict(obs_dim=4, n_act=3, rdim=3, hidden=32, batch=20, weight_num=4, seed=8800, done_p=0.2),
}
COMMON = dict(n_table=120, n_learn=8, gamma=0.99, tau=0.01, lr=1e-3, beta=0.95, done_p=0.05)
# the class case: ENVELOPE's host side (priorities, the homotopy on beta, prioritised draws, select_action) on a ring of 40 rows
# that wraps: 70 add() calls, a learn() every 5 steps from step 30 on (8 calls, the last four on the wrapped ring)
CLASS = dict(obs_dim=4, n_act=3, rdim=2, hidden=32, batch=8, weight_num=3, seed=8900, capacity=40, n_steps=70, learn_from=30,
             learn_every=5, beta=0.9, max_episodes=20, done_p=0.1)
MARGIN = 1e-4       # smallest admitted gap between the two largest w . Q_online(s') of any row of any call


def case(name):
    c = dict(COMMON)
    c.update(CLASS if name == "class" else CASES[name])
    return c


def layers(c):
    H, O, A, R = c["hidden"], c["obs_dim"], c["n_act"], c["rdim"]
    return [("l1", H, O + R), ("l2", H, H), ("l3", A * R, H)]


def table(seed, n, c):
    """obs, next_obs ~ N(0,1), act an index, reward vectors ~ N(0,1) [n, R], done ~ Bernoulli(done_p)."""
    g = np.random.default_rng(seed)
    obs = g.standard_normal((n, c["obs_dim"])).astype(F32)
    next_obs = g.standard_normal((n, c["obs_dim"])).astype(F32)
    act = g.integers(0, c["n_act"], (n, 1)).astype(F32)
    rew = g.standard_normal((n, c["rdim"])).astype(F32)
    done = g.random(n) < c["done_p"]
    return dict(obs=obs, act=act, rew=rew, next_obs=next_obs, done=done)


def weights(seed, weight_num, rdim):
    """np.abs(randn) / L1 norm in float64, cast to float32 (:221-223), from a PCG64 stream."""
    w = np.random.default_rng(seed).standard_normal((weight_num, rdim))
    return (np.abs(w) / np.linalg.norm(w, ord=1, axis=1, keepdims=True)).astype(F32)


def inputs(c, n_learn=None, seed=None):
    """Parameters (PCG64), the transition table and every call's sample indices and preference vectors."""
    s = c["seed"] if seed is None else seed
    calls = c["n_learn"] if n_learn is None else n_learn
    n = c.get("n_steps", c["n_table"])
    return dict(params=synth.mlp_params(s, layers(c)), table=table(s + 2, n, c),
                idx=[synth.indices(s + 100 + i, n, c["batch"]) for i in range(calls)],
                weights=[weights(s + 200 + i, c["weight_num"], c["rdim"]) for i in range(calls)])


class EnvelopeDQN:
    """One learner: Q-net l1..l3 on [obs | w] with a deep-copied target, Adam (torch defaults), no gradient clipping (the
    reference's clip_grad_norm_ runs before backward() and clips nothing), soft update on every call."""

    def __init__(self, params, obs_dim, n_act, rdim, lr, capacity, dtype=F32):
        self.O, self.A, self.R, self.dt = obs_dim, n_act, rdim, dtype
        self.q = {k: np.array(v, dtype=dtype) for k, v in params.items()}
        self.q_t = {k: np.array(v, dtype=dtype) for k, v in params.items()}
        self.net = nn.MLP(["l1", "l2", "l3"])
        self.opt = nn.Adam(self.q, lr)
        self.capacity = capacity
        self.obs = np.zeros((capacity, obs_dim), dtype)
        self.act = np.zeros(capacity, np.int64)
        self.rew = np.zeros((capacity, rdim), dtype)
        self.nobs = np.zeros((capacity, obs_dim), dtype)
        self.done = np.zeros(capacity, dtype)
        self.index = self.size = 0
        self.min_gap = np.inf

    def add(self, obs, act, rew, nobs, done):
        i = self.index
        self.obs[i], self.act[i], self.rew[i], self.nobs[i], self.done[i] = obs, int(np.asarray(act).reshape(-1)[0]), rew, nobs, float(done)
        self.index = (i + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def forward(self, p, obs, w):
        """-> (Q [n, A, R], activations)"""
        out, acts = self.net.forward(p, np.concatenate([obs, w], axis=1).astype(self.dt))
        return out.reshape(-1, self.A, self.R), acts

    # ---- the class's host side
    def choose(self, obs, pref):
        """argmax_a w . Q(obs, w)[a] (select_action / evaluate_action, :102-136) -> (action, gap to the runner-up)"""
        q, _ = self.forward(self.q, np.asarray(obs, self.dt).reshape(1, -1), np.asarray(pref, self.dt).reshape(1, -1))
        s = q[0] @ np.asarray(pref, self.dt)
        top = np.sort(s)
        return int(np.argmax(s)), float(top[-1] - top[-2])

    def priority(self, obs, act, rew, nobs, done, gamma, pref):
        """|w.r + gamma w.Q(s')[a*] - w.Q(s)[a]| + 1e-5, and |w.r - w.Q(s)[a]| + 1e-5 on done (:157-186)"""
        w = np.asarray(pref, self.dt)
        q, _ = self.forward(self.q, np.asarray(obs, self.dt).reshape(1, -1), w.reshape(1, -1))
        wq = w @ q[0, int(act)]
        wr = w @ np.asarray(rew, self.dt)
        if done:
            return abs(wr - wq) + 1e-5
        qn, _ = self.forward(self.q, np.asarray(nobs, self.dt).reshape(1, -1), w.reshape(1, -1))
        hq = qn[0, int(np.argmax(qn[0] @ w))]
        return abs(wr + self.dt(gamma) * (w @ hq) - wq) + 1e-5

    # ---- learn
    def learn_with(self, idx, w, gamma, tau, beta):
        """One learn() on the rows `idx` [B] under the preferences `w` [W, R]; returns the loss."""
        dt = self.dt
        idx = np.asarray(idx, np.int64)
        B, W = idx.size, len(w)
        N = B * W
        rows = np.tile(idx, W)                                          # row j: sample idx[j % B]
        wr = np.repeat(np.asarray(w, dt), B, axis=0)                    # ... under w[j // B]
        ar = np.arange(N)
        rew, done = self.rew[rows], self.done[rows][:, None]
        # a' = argmax_a w . Q_online(s', w)[a] (first maximum), T = r + gamma Q_target(s', w)[a'] (1 - done) (:232-240)
        qn, _ = self.forward(self.q, self.nobs[rows], wr)
        s = np.einsum("nar,nr->na", qn, wr)
        a2 = np.argmax(s, axis=1)
        if self.A > 1:
            top = np.sort(s, axis=1)
            self.min_gap = min(self.min_gap, float(np.min(top[:, -1] - top[:, -2])))
        qt, _ = self.forward(self.q_t, self.nobs[rows], wr)
        T = rew + dt(gamma) * qt[ar, a2] * (dt(1) - done)
        # Q = Q_online(s, w)[a]; loss = beta mse(w.Q, w.T) + (1 - beta) mse(Q, T) (:242-249)
        qa, acts = self.forward(self.q, self.obs[rows], wr)
        a = self.act[rows]
        Q = qa[ar, a]
        d = np.sum(Q * wr, axis=1, dtype=dt) - np.sum(T * wr, axis=1, dtype=dt)
        E = Q - T
        loss = dt(beta) * np.mean(d * d, dtype=dt) + dt(1 - beta) * np.mean(E * E, dtype=dt)
        dQ = dt(beta) * dt(2.0 / N) * d[:, None] * wr + dt(1 - beta) * dt(2.0 / (N * self.R)) * E
        dy = np.zeros((N, self.A, self.R), dt)
        dy[ar, a] = dQ
        _, g = self.net.backward(self.q, acts, dy.reshape(N, -1), need_dx=False)
        self.opt.step(self.q, {k: g[k] for k in self.q})               # no clipping
        nn.soft_update(self.q_t, self.q, tau)
        return dt(loss)


def make(c, inp, dtype=F32):
    t = inp["table"]
    o = EnvelopeDQN(inp["params"], c["obs_dim"], c["n_act"], c["rdim"], c["lr"], c.get("capacity", len(t["done"])), dtype)
    if "capacity" not in c:             # the table is the ring
        for i in range(len(t["done"])):
            o.add(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]))
    return o


def run(c, inp, n_learn=None, dtype=F32):
    """-> (oracle, losses [calls])"""
    o = make(c, inp, dtype)
    losses = [o.learn_with(inp["idx"][i], inp["weights"][i], c["gamma"], c["tau"], c["beta"])
              for i in range(c["n_learn"] if n_learn is None else n_learn)]
    return o, np.array(losses, dtype=dtype)


def class_schedule(c):
    """The class case's script: per step `select_action(obs)`, `add(...)` of the table's transition, and a learn() every
    `learn_every` steps from `learn_from` on -> list of the steps after whose add() a learn() runs."""
    return [t for t in range(c["n_steps"]) if t + 1 >= c["learn_from"] and (t + 1 - c["learn_from"]) % c["learn_every"] == 0][:c["n_learn"]]
