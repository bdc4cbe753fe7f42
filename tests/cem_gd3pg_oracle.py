"""CEM_GD3PG.learn (CEM_GD3PG_file/CEM_GD3PG.py:94-231) restated in NumPy, and the seeded inputs of its golden cases.  The golden
generator (tests/golden/make_cem_gd3pg_golden.py) runs the reference on exactly these inputs; the CPU tests hold this oracle to torch
autograd and to the recording, the GPU test holds the HIP engine to both.

One learn() trains on B = 2 half rows, half = min(len(buffer_domain), batch) // 2: `half` rows of `buffer`, then `half` rows of
`buffer_domain`, both drawn below len(buffer_domain); rows of `buffer` that were never written are zeros.  `dtype=np.float64` runs the
same arithmetic in float64.

`switches` names the near misses a correct implementation must be told apart from (each moves a compared quantity of every golden case):
    mean_q        the TD target takes the mean of the two target critic values instead of their minimum
    kl_ba         KL = sqrt(sum c^2 / (B A)) instead of sqrt(sum c^2 / B)
    wrong_guide   the penalty lands on the actor that did better
    unstepped     the actor steps go through the critic as it was BEFORE this call's critic step
    relu          the critic's hidden activation is ReLU instead of LeakyReLU(0.01)
    bound_buffer  (draw() only) the first draw is bounded by len(buffer) instead of len(buffer_domain)
"""
import numpy as np

from oracle import nn
from tests.golden import synth

F32 = np.float32
NAMES = ["l1", "l2", "l3"]
CLIP = 0.5
LAMBDA = 10.0
SLOPE = 0.01
SWITCHES = ("mean_q", "kl_ba", "wrong_guide", "unstepped", "relu")

# dims, hidden, batch, rows of each ring (n0 `buffer`, n1 `buffer_domain`; capacity = cap); `short`: the ring bound wins (70 over 30 rows)
# and `buffer` holds fewer rows than `buffer_domain`, so its draws reach rows that were never written.  reward_scale puts the critic's
# pre-clip norm on both sides of 0.5 across the cases, delta / critic_head_scale the two actors' norms (found with this oracle and
# asserted by the generator).
CASES = {
    "pend": dict(obs_dim=3, act_dim=1, hidden=32, batch=10, cap=64, n0=64, n1=40, f1_more=True, delta=0.6, reward_scale=0.05, seed=7100),
    "odd": dict(obs_dim=24, act_dim=4, hidden=128, batch=33, cap=96, n0=96, n1=96, f1_more=False, delta=0.01, reward_scale=1.0, seed=7200),
    "short": dict(obs_dim=5, act_dim=2, hidden=32, batch=70, cap=48, n0=12, n1=30, f1_more=True, delta=0.6, reward_scale=1.0, seed=7300,
                  critic_head_scale=40.0),
    "walker": dict(obs_dim=24, act_dim=4, hidden=128, batch=256, cap=600, n0=600, n1=560, f1_more=True, delta=0.3, reward_scale=1.0, seed=7400),
}
COMMON = dict(n_learn=3, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, done_p=0.3, target_jitter=0.3)


def case(name):
    return dict(COMMON, **CASES[name])


def actor_layers(c):
    return [("l1", c["hidden"], c["obs_dim"]), ("l2", c["hidden"], c["hidden"]), ("l3", c["act_dim"], c["hidden"])]


def critic_layers(c):
    return [("l1", c["hidden"], c["obs_dim"] + c["act_dim"]), ("l2", c["hidden"], c["hidden"]), ("l3", 1, c["hidden"])]


def table(seed, n, c):
    """obs, next_obs ~ N(0,1), act ~ U(-1,1), reward ~ reward_scale N(0,1), done ~ Bernoulli(done_p)."""
    g = np.random.default_rng(seed)
    obs = g.standard_normal((n, c["obs_dim"])).astype(F32)
    next_obs = g.standard_normal((n, c["obs_dim"])).astype(F32)
    act = g.uniform(-1, 1, (n, c["act_dim"])).astype(F32)
    rew = (g.standard_normal(n) * c.get("reward_scale", 1.0)).astype(F32)
    done = g.random(n) < c["done_p"]
    return dict(obs=obs, act=act, rew=rew, next_obs=next_obs, done=done)


def _jitter(seed, p, rel):
    """A target net that has drifted from its online net: every element scaled by U(1 - rel, 1 + rel)."""
    g = np.random.default_rng(seed)
    return {k: (v * g.uniform(1 - rel, 1 + rel, v.shape)).astype(F32) for k, v in p.items()}


def inputs(c, n_learn=None, seed=None):
    """The seven nets (PCG64), both rings' tables and every call's two index draws (both below n1, `half` rows each)."""
    s = c["seed"] if seed is None else seed
    calls = c["n_learn"] if n_learn is None else n_learn
    critic = synth.mlp_params(s + 2, critic_layers(c))
    scale = c.get("critic_head_scale")
    if scale:
        critic["l3.weight"] = (critic["l3.weight"] * F32(scale)).astype(F32)
    a1, a2 = synth.mlp_params(s, actor_layers(c)), synth.mlp_params(s + 1, actor_layers(c))
    j = c.get("target_jitter", 0.0)
    half = min(c["n1"], c["batch"]) // 2
    return dict(actor_1=a1, actor_2=a2, critic=critic, actor_domain=synth.mlp_params(s + 3, actor_layers(c)),
                actor_1_target=_jitter(s + 4, a1, j), actor_2_target=_jitter(s + 5, a2, j), critic_target=_jitter(s + 6, critic, j),
                table0=table(s + 10, c["n0"], c), table1=table(s + 11, c["n1"], c),
                idx=[np.stack([synth.indices(s + 100 + 2 * i, c["n1"], half), synth.indices(s + 101 + 2 * i, c["n1"], half)]) for i in range(calls)])


# ---------------------------------------------------------------------------------- nets
def _act(z, kind, dt):
    if kind == "tanh":
        return np.tanh(z)
    if kind == "leaky":
        return np.where(z > 0, z, dt(SLOPE) * z)
    if kind == "relu":
        return np.maximum(z, dt(0))
    return z


def _act_grad(h, kind, dt):
    """from the activation's OUTPUT"""
    if kind == "tanh":
        return dt(1) - h * h
    if kind == "leaky":
        return np.where(h > 0, dt(1), dt(SLOPE))
    if kind == "relu":
        return (h > 0).astype(dt)
    return np.ones_like(h)


def forward(p, x, hidden, out, dt):
    acts = [x]
    for i, n in enumerate(NAMES):
        z = acts[-1] @ p[n + ".weight"].T + p[n + ".bias"]
        acts.append(_act(z, hidden if i < 2 else out, dt).astype(dt))
    return acts[-1], acts


def backward(p, acts, dy, hidden, out, dt, need_dx=False):
    grads, d = {}, dy
    for i in (2, 1, 0):
        n = NAMES[i]
        d = (d * _act_grad(acts[i + 1], hidden if i < 2 else out, dt)).astype(dt)
        grads[n + ".weight"] = d.T @ acts[i]
        grads[n + ".bias"] = d.sum(axis=0)
        if i > 0 or need_dx:
            d = d @ p[n + ".weight"]
    return (d if need_dx else None), {k: grads[k] for k in p}


def clip_grad_norm(grads, max_norm, dt):
    """torch.nn.utils.clip_grad_norm_: -> the pre-clip norm; `grads` scaled in place."""
    norms = np.array([np.sqrt(np.sum(g.astype(dt) ** 2, dtype=dt)) for g in grads.values()], dtype=dt)
    total = np.sqrt(np.sum(norms ** 2, dtype=dt))
    coef = min(dt(max_norm) / (total + dt(1e-6)), dt(1.0))
    for k in grads:
        grads[k] = grads[k] * dt(coef)
    return float(total)


class Adam(nn.Adam):
    """oracle.nn.Adam with its float32 constants taken in the oracle's dtype"""

    def __init__(self, params, lr, dt):
        super().__init__(params, lr)
        self.dt = dt

    def step(self, params, grads):
        dt = self.dt
        self.t += 1
        bc1, bc2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for k in params:
            g, m, v = grads[k], self.m[k], self.v[k]
            m += (g - m) * dt(1.0 - self.b1)
            v *= dt(self.b2)
            v += dt(1.0 - self.b2) * g * g
            params[k] -= dt(self.lr / bc1) * (m / (np.sqrt(v) / dt(np.sqrt(bc2)) + dt(self.eps)))


class CemGd3pg:
    """One learner: two online actors, the frozen domain actor, one critic, the three targets, three Adams behind clips at 0.5, two rings."""

    def __init__(self, inp, c, dtype=F32, switches=()):
        unknown = set(switches) - set(SWITCHES) - {"bound_buffer"}
        assert not unknown, unknown
        self.dt, self.sw, self.c = dtype, set(switches), c
        cp = lambda p: {k: np.array(v, dtype=dtype) for k, v in p.items()}
        self.actor = [cp(inp["actor_1"]), cp(inp["actor_2"])]
        self.actor_t = [cp(inp.get("actor_1_target", inp["actor_1"])), cp(inp.get("actor_2_target", inp["actor_2"]))]
        self.critic, self.critic_t = cp(inp["critic"]), cp(inp.get("critic_target", inp["critic"]))
        self.domain = cp(inp["actor_domain"])
        self.aopt = [Adam(self.actor[0], c["actor_lr"], dtype), Adam(self.actor[1], c["actor_lr"], dtype)]
        self.copt = Adam(self.critic, c["critic_lr"], dtype)
        cap, O, A = c["cap"], c["obs_dim"], c["act_dim"]
        self.cap = cap
        self.ring = [dict(obs=np.zeros((cap, O), dtype), act=np.zeros((cap, A), dtype), rew=np.zeros(cap, dtype), next_obs=np.zeros((cap, O), dtype),
                          done=np.zeros(cap, dtype), index=0, size=0) for _ in range(2)]
        for r, key in ((0, "table0"), (1, "table1")):
            t = inp.get(key)
            for i in range(len(t["done"]) if t else 0):
                self.add(r, t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]))

    def add(self, r, obs, act, rew, nobs, done):
        g = self.ring[r]
        i = g["index"]
        g["obs"][i], g["act"][i], g["rew"][i], g["next_obs"][i], g["done"][i] = obs, act, rew, nobs, float(done)
        g["index"] = (i + 1) % self.cap
        g["size"] = min(g["size"] + 1, self.cap)

    def draw(self, batch):
        """sample()'s two np.random.choice calls (:161-166) -> (ring 0's rows, ring 1's rows)"""
        total = self.ring[1]["size"]
        half = min(total, batch) // 2
        first = self.ring[0]["size"] if "bound_buffer" in self.sw else total
        return np.random.choice(first, half, replace=False), np.random.choice(total, half, replace=False)

    def pi(self, p, obs):
        return forward(p, obs, "tanh", "tanh", self.dt)

    def q(self, p, obs, act):
        return forward(p, np.concatenate([obs, act], axis=1).astype(self.dt), "relu" if "relu" in self.sw else "leaky", None, self.dt)

    def learn_with(self, idx, gamma, tau, f1_more, delta):
        """One learn() on ring 0's rows idx[0] and ring 1's rows idx[1] -> dict in the order of frl_cem_gd3pg_args::out"""
        dt, A = self.dt, self.c["act_dim"]
        hk = "relu" if "relu" in self.sw else "leaky"
        cat = lambda key: np.concatenate([self.ring[0][key][np.asarray(idx[0], np.int64)], self.ring[1][key][np.asarray(idx[1], np.int64)]])
        obs, act, nobs = cat("obs"), cat("act"), cat("next_obs")
        rew, done = cat("rew")[:, None], cat("done")[:, None]
        B = len(obs)
        # ---- critic (:185-194)
        q1 = self.q(self.critic_t, nobs, self.pi(self.actor_t[0], nobs)[0])[0]
        q2 = self.q(self.critic_t, nobs, self.pi(self.actor_t[1], nobs)[0])[0]
        qn = (q1 + q2) * dt(0.5) if "mean_q" in self.sw else np.minimum(q1, q2)
        T = rew + dt(gamma) * qn * (dt(1) - done)
        Q, cacts = self.q(self.critic, obs, act)
        E = Q - T
        closs = np.mean(E * E, dtype=dt)
        old_critic = {k: v.copy() for k, v in self.critic.items()}
        _, g = backward(self.critic, cacts, E * dt(2.0 / B), hk, None, dt)
        cnorm = clip_grad_norm(g, CLIP, dt)
        self.copt.step(self.critic, g)
        through = old_critic if "unstepped" in self.sw else self.critic
        # ---- actors (:198-216)
        guided = (1 if f1_more else 0) ^ (1 if "wrong_guide" in self.sw else 0)
        adom = self.pi(self.domain, obs)[0]
        out = dict(critic_loss=float(closs), critic_norm=cnorm, KL=0.0, rows=float(B))
        steps = []
        for j in (0, 1):
            a, aacts = self.pi(self.actor[j], obs)
            Qp, qacts = self.q(through, obs, a)
            loss = -np.mean(Qp, dtype=dt)
            dx, _ = backward(through, qacts, np.full((B, 1), dt(-1.0 / B), dt), hk, None, dt, need_dx=True)
            da = dx[:, -A:]
            if j == guided:
                cdiff = a - adom
                c2 = np.sum(cdiff * cdiff, dtype=dt)
                kl = np.sqrt(c2 / dt(B * A if "kl_ba" in self.sw else B))
                loss = loss + dt(LAMBDA) * dt(delta) * kl
                out["KL"] = float(kl)
                if c2 > 0:          # (torch: NaN gradients at c2 == 0; the engine's departure: no penalty gradient)
                    da = da + dt(LAMBDA) * dt(delta) * cdiff / (dt(B * A if "kl_ba" in self.sw else B) * kl)
            _, ga = backward(self.actor[j], aacts, da.astype(dt), "tanh", "tanh", dt)
            steps.append((j, ga))
            out["actor_%d_loss" % (j + 1)] = float(loss)
        for j, ga in steps:
            out["actor_%d_norm" % (j + 1)] = clip_grad_norm(ga, CLIP, dt)
            self.aopt[j].step(self.actor[j], ga)
        # ---- soft updates (:221-231)
        for tg, src in ((self.critic_t, self.critic), (self.actor_t[0], self.actor[0]), (self.actor_t[1], self.actor[1])):
            for k in tg:
                tg[k] = tg[k] * dt(1.0 - tau) + src[k] * dt(tau)
        return out


def digest(p, n_sample=64):
    """A net's (or a moment's) fingerprint, tensors in NAMES order, weight then bias: (sum and abs-sum of each tensor, float64 [6][2]; a
    strided sample of up to n_sample elements of each, concatenated, float32) — two arrays per state keep the fixture small"""
    sums, sample = [], []
    for n in NAMES:
        for suffix in (".weight", ".bias"):
            flat = np.asarray(p[n + suffix]).reshape(-1).astype(np.float64)
            sums.append([flat.sum(), np.abs(flat).sum()])
            sample.append(flat[::max(1, flat.size // n_sample)][:n_sample])
    return np.array(sums, np.float64), np.concatenate(sample).astype(F32)


OUT = ("critic_loss", "critic_norm", "actor_1_loss", "actor_1_norm", "actor_2_loss", "actor_2_norm", "KL", "rows")


def run(c, inp, n_learn=None, dtype=F32, switches=()):
    """-> (oracle, [calls][8] in OUT's order)"""
    o = CemGd3pg(inp, c, dtype, switches)
    calls = c["n_learn"] if n_learn is None else n_learn
    res = [o.learn_with(inp["idx"][i], c["gamma"], c["tau"], c["f1_more"], c["delta"]) for i in range(calls)]
    return o, np.array([[r[k] for k in OUT] for r in res], np.float64)


# ------------------------------------------------------------------------------------ sepCEM
# the script both the reference's class (the generator) and freerl_amd.CEM_GD3PG.sepCEM (the CPU test) are run through
SEPCEM_SEED = 4200
SEPCEM = {"pop4": dict(pop_size=4, antithetic=True), "pop10": dict(pop_size=10, antithetic=True), "pop5": dict(pop_size=5, antithetic=False)}
SEPCEM_PARAMS, SEPCEM_GENERATIONS = 50, 3


def sepcem_script(cls, cfg, seed):
    """The loop's use of the class (CEM_GD3PG.py:405-439): ask(2 n) once, then per generation tell(all, fitness) and ask(n) into the first
    half; fitness from the seeded stream.  -> dict of everything returned / held, and the generator state afterwards"""
    np.random.seed(seed)
    n = cfg["pop_size"]
    mu0 = np.random.randn(SEPCEM_PARAMS)
    es = cls(SEPCEM_PARAMS, mu_init=mu0, sigma_init=1e-3, damp=1e-3, damp_limit=1e-5, pop_size=n, antithetic=cfg["antithetic"], parents=n // 2, elitism=False)
    out = {"weights": np.array(es.weights), "elite0": np.array(es.elite)}
    params = es.ask(2 * n)
    out["ask0"] = params.copy()
    for g in range(SEPCEM_GENERATIONS):
        fitness = list(np.random.randn(2 * n) * 100.0)
        es.tell(params, fitness)
        half = es.ask(n)
        params[:n] = half
        mu, cov = es.get_distrib_params()
        out["gen%d/ask" % g], out["gen%d/mu" % g], out["gen%d/cov" % g] = half.copy(), mu, cov
        out["gen%d/elite" % g], out["gen%d/elite_score" % g], out["gen%d/damp" % g] = np.array(es.elite), np.float64(es.elite_score), np.float64(es.damp)
    out["next_uniform"] = np.float64(np.random.rand())          # the generator state afterwards
    return out
