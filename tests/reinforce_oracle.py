"""REINFORCE (REINFORCE_file/REINFORCE.py:32-127) restated in NumPy, and the seeded inputs of its golden cases.  The golden
generator (tests/golden/make_reinforce_golden.py) runs the reference on exactly these inputs; the CPU test holds this oracle
to its output and the GPU test holds the HIP engine to both.

Two settings: float32 wherever the reference is float32 (the default), and dtype=np.float64 for everything after the
return scan — used only to size tolerances (what float32 rounding alone does to a loss or a normalised return).
"""
import numpy as np

from tests.golden import synth

F32 = np.float32
EPS = np.finfo(np.float32).eps          # Categorical(probs=) clamps at the eps of the probabilities' dtype (float32 in the reference)

# One learner, >= 12 learn() calls per case, T (the stored steps) changing from call to call
_T_EDGES = [17, 2, 500, 15, 64, 33, 16, 200, 31, 65, 32, 63]
_T_MIXED = [40, 7, 100, 33, 64, 18, 129, 2, 50, 96, 31, 77]
CASES = {
    "o4_a2": dict(obs_dim=4, n_act=2, hidden=128, seed=9100, Ts=_T_EDGES),          # CartPole's dims
    "o17_a3": dict(obs_dim=17, n_act=3, hidden=128, seed=9200, Ts=_T_MIXED),        # two k-tiles in the first layer
    "o8_a20": dict(obs_dim=8, n_act=20, hidden=128, seed=9300, Ts=_T_MIXED),        # two head tiles
    "o8_a4_h256": dict(obs_dim=8, n_act=4, hidden=256, seed=9400, Ts=_T_MIXED),
    # two and three episodes per call; the flags are the episodes' ends, and an episode that ends truncated carries no flag
    "multi": dict(obs_dim=4, n_act=2, hidden=128, seed=9500, kind="multi",
                  episodes=[[(20, 1), (13, 1)], [(9, 0), (30, 1), (11, 1)], [(40, 1), (25, 0)], [(5, 1), (5, 1), (50, 1)],
                            [(33, 0), (31, 1)], [(16, 1), (16, 0), (16, 1)], [(64, 1), (2, 1)], [(100, 0), (7, 1)],
                            [(12, 1), (45, 1), (3, 0)], [(70, 1), (70, 1)], [(21, 0), (22, 0), (23, 1)], [(8, 1), (90, 1)]]),
    "flat": dict(obs_dim=4, n_act=2, hidden=128, seed=9600, kind="flat", gamma=0.0, Ts=_T_MIXED),   # all returns equal: std = 0
    "clamp": dict(obs_dim=6, n_act=4, hidden=128, seed=9700, kind="clamp", Ts=_T_MIXED),
}
COMMON = dict(gamma=0.99, lr=1e-3, kind="plain")
LONG = dict(obs_dim=4, n_act=2, hidden=128, seed=9800, n_learn=150)


def case(name):
    c = dict(COMMON)
    c.update(LONG if name == "long" else CASES[name])
    if name == "long":
        g = np.random.default_rng(c["seed"] + 5)
        c["Ts"] = [int(t) for t in g.integers(8, 201, c["n_learn"])]
    if c["kind"] == "multi":
        c["Ts"] = [sum(n for n, _ in eps) for eps in c["episodes"]]
    c["n_learn"] = len(c["Ts"])
    return c


def layers(c):
    return [("l1", c["hidden"], c["obs_dim"]), ("l2", c["n_act"], c["hidden"])]


def inputs(c):
    """Parameters (PCG64) and, per call, the stored steps: obs [T, O], act [T], rew [T], done [T]."""
    s, O, A = c["seed"], c["obs_dim"], c["n_act"]
    params = synth.mlp_params(s, layers(c))
    if c["kind"] == "clamp":
        # a head bias of +20 / -20 on actions 0 / 1: p[0] > 1 - eps, every other p < eps.  Hidden unit 0 reads the last obs
        # column alone (an indicator, 0 or 1) and feeds -20 / +20 back into the two logits, so rows with the indicator set are
        # ordinary rows
        params["l2.bias"][:] = 0
        params["l2.bias"][0], params["l2.bias"][1] = 20.0, -20.0
        params["l1.weight"][0, :] = 0
        params["l1.weight"][0, O - 1] = 1.0
        params["l1.bias"][0] = 0
        params["l1.weight"][1:, O - 1] = 0
        params["l2.weight"][:, 0] = 0
        params["l2.weight"][0, 0], params["l2.weight"][1, 0] = -20.0, 20.0
    calls = []
    for k, T in enumerate(c["Ts"]):
        t = synth.transitions(s + 10 + k, T, O, 1, n_discrete=A)
        obs, act, rew, done = t["obs"], t["act"][:, 0].astype(np.int64), t["rew"], t["done"].copy()
        if c["kind"] == "multi":
            done[:] = False
            pos = 0
            for n, term in c["episodes"][k]:
                pos += n
                done[pos - 1] = bool(term)
        elif c["kind"] == "flat":
            rew = np.ones(T, F32)
            done[:] = False
        elif c["kind"] == "clamp":
            g = np.random.default_rng(s + 500 + k)
            obs[:, O - 1] = (g.random(T) < 0.4).astype(F32)        # 40 % ordinary rows
            act = g.integers(0, A, T).astype(np.int64)             # forced actions on both sides of the clamp
            act[:2] = [0, 1]                                       # ... both sides in every call, T = 2 included
            obs[:2, O - 1] = 0
        calls.append(dict(obs=obs, act=act, rew=rew, done=done))
    return dict(params=params, calls=calls)


def returns64(rew, done, gamma):
    """The reference's scan (:108-112), in Python floats."""
    out, G = [0.0] * len(rew), 0
    for t in reversed(range(len(rew))):
        G = float(rew[t]) + gamma * G * (1 - bool(done[t]))
        out[t] = G
    return np.array(out, np.float64)


class Reinforce:
    """One learner: Policy_MLP l1 (ReLU) l2 (softmax), Adam (eps 1e-8), no gradient clipping."""

    def __init__(self, params, lr, dtype=F32):
        self.dt = dtype
        self.p = {k: np.array(v, dtype=dtype) for k, v in params.items()}
        self.lr, self.t = float(lr), 0
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}

    def probs(self, x):
        dt = self.dt
        h = np.maximum(x.astype(dt) @ self.p["l1.weight"].T + self.p["l1.bias"], dt(0))
        z = h @ self.p["l2.weight"].T + self.p["l2.bias"]
        e = np.exp(z - z.max(axis=1, keepdims=True)).astype(dt)
        p = (e / e.sum(axis=1, keepdims=True, dtype=dt)).astype(dt)                 # F.softmax
        return (p / p.sum(axis=1, keepdims=True, dtype=dt)).astype(dt), h           # Categorical: probs / probs.sum(-1)

    def log_prob(self, q, act):
        qa = q[np.arange(len(act)), act]
        return np.log(np.clip(qa, dt_eps(self.dt), self.dt(1) - dt_eps(self.dt))).astype(self.dt), qa

    def learn_with(self, obs, act, rew, done, gamma):
        """One learn() on the given steps -> dict(loss, s, ghat, logp)."""
        dt = self.dt
        G = returns64(rew, done, gamma).astype(F32).astype(dt)                     # cast to float32 once (:114)
        with np.errstate(invalid="ignore", divide="ignore"):
            ghat = ((G - G.mean(dtype=dt)) / (G.std(ddof=1, dtype=dt) + dt(1e-8))).astype(dt)     # torch.std: n - 1
        q, h = self.probs(obs)
        logp, qa = self.log_prob(q, act)
        terms = (-logp * ghat).astype(dt)
        loss = np.cumsum(terms, dtype=dt)[-1]                                       # `loss += ...` step by step (:119-121)
        open_ = (qa >= dt_eps(dt)) & (qa <= dt(1) - dt_eps(dt))                     # the clamp passes no gradient outside
        onehot = np.zeros_like(q)
        onehot[np.arange(len(act)), act] = 1
        dz = ((q - onehot) * (ghat * open_)[:, None]).astype(dt)
        g = {"l2.weight": dz.T @ h, "l2.bias": dz.sum(axis=0)}
        dh = (dz @ self.p["l2.weight"]) * (h > 0)
        g["l1.weight"], g["l1.bias"] = dh.T @ obs.astype(dt), dh.sum(axis=0)
        self._adam(g)
        return dict(loss=dt(loss), s=float(np.abs(terms.astype(np.float64)).sum()), ghat=ghat, logp=logp)

    def _adam(self, g):
        dt = self.dt
        self.t += 1
        bc1, bc2 = 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t
        for k in self.p:
            m, v = self.m[k], self.v[k]
            m += (g[k] - m) * dt(1.0 - 0.9)
            v *= dt(0.999)
            v += dt(1.0 - 0.999) * g[k] * g[k]
            self.p[k] -= dt(self.lr / bc1) * (m / (np.sqrt(v) / dt(np.sqrt(bc2)) + dt(1e-8)))


def dt_eps(dt):
    return dt(EPS)          # the clamp bound is float32's eps in both settings: the float64 mode sizes float32 rounding, not another clamp


def run(c, inp, dtype=F32, n_learn=None):
    """-> (oracle, [per-call dict of learn_with])"""
    o = Reinforce(inp["params"], c["lr"], dtype)
    outs = []
    for call in inp["calls"][:n_learn]:
        outs.append(o.learn_with(call["obs"], call["act"], call["rew"], call["done"], c["gamma"]))
    return o, outs
