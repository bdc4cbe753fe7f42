"""MASAC (MAAC_file/MASAC.py:32-139,205-286; entropy_way_c = entropy_way_a = action_way = '1', adaptive alpha) restated in NumPy: the whole
learn() with injected row indices and N(0,1) draws, in float32 or float64, and the seeded inputs of its golden cases.  The golden
generator (tests/golden/make_masac_golden.py) runs the reference on exactly these inputs; the CPU test (tests/test_masac_oracle.py)
holds this oracle to its output and to torch autograd, the GPU test (tests/test_gpu_masac.py) holds the HIP engine to both.

Per updating agent i, in agent order: rows idx[i]; draws eps[i][s]: s = j the target actor j's, s = n + j the online actor j's, s = 2 n the
second draw of actor i (the entropy).  Three switches exist only to prove that the tests tell the reference's semantics from near misses:
`stale_actors` (the actor stage reads the other agents' online actors as they were before the call), `one_draw` (the entropy reuses
the draw n + i), `mean_twins` (the twins' mean instead of their minimum in the actor loss).
"""
import numpy as np

from oracle import nn
from tests.golden import synth

F32 = np.float32
CLIP = 0.5
ALPHA_LR = 1e-4
ACTOR_NAMES = ["l1", "l2", "mean_layer", "log_std_layer"]
CRITIC_NAMES = ["l1", "l2", "l3", "l1_2", "l2_2", "l3_2"]
Q1, Q2 = CRITIC_NAMES[:3], CRITIC_NAMES[3:]
LOG_SQRT_2PI = 0.5 * np.log(2 * np.pi)

# name -> agents (obs, act), hidden, batch.  Every case: 3 learn() calls, recorded after the 1st and the 3rd.
#   pair    no full 16-row chunk; agent 0's own action columns (14 .. 17 of the 22 of [obs | act]) straddle the 16-column tile seam
#   hetero  one full chunk plus one row; a 2-column actor head (agents 0 and 2); action offsets [0, 1, 3, 4]
#   spread3 the script's nets (simple_spread_v3, N = 3)
#   clamp   pair's shape, log_std_layer rescaled so that its outputs leave [-20, 2] on both sides
#   seq     hetero's shape, larger learning rates and alpha: what the three switches must move
CASES = {
    "pair": dict(dims=[(7, 4)] * 2, hidden=64, batch=5, seed=8100),
    "hetero": dict(dims=[(8, 1), (10, 2), (10, 1)], hidden=64, batch=17, seed=8200),
    "spread3": dict(dims=[(18, 5)] * 3, hidden=128, batch=64, seed=8300),
    "clamp": dict(dims=[(7, 4)] * 2, hidden=64, batch=5, seed=8400, ls_scale=120.0, alpha0=[0.001, 0.001]),
    "seq": dict(dims=[(8, 1), (10, 2), (10, 1)], hidden=64, batch=17, seed=8500, actor_lr=0.05, critic_lr=0.02, alpha0=[0.1, 0.5, 1.0], critic_scale=3.0),
}
# alpha0: None = the class's own 0.01; a list = per agent, set through the Alpha objects before the first call
COMMON = dict(n_table=300, n_learn=3, gamma=0.95, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, done_p=0.1, alpha0=None, ls_scale=1.0, critic_scale=1.0)
# per-agent reward scales: agent 0's rewards are small (its critic's pre-clip norm stays under 0.5), the others' are O(1) and larger
REW_SCALE = dict(pair=[0.02, 2.0], hetero=[0.02, 1.0, 3.0], spread3=[0.02, 1.0, 3.0], clamp=[0.02, 2.0], seq=[0.02, 1.0, 3.0])
RECORD_AFTER = (1, 3)
# The project's tolerances (tests/test_gpu_envelope_ddpg.py): losses rtol 1e-4 / atol 1e-6, norms rtol 1e-3, parameters rtol 5e-4 / atol 5e-6
# on >= 99 % of a tensor's elements, Adam's m 2e-3 of a tensor's largest |m|.  Measured on the CPU against the float64 oracle
# (tests/test_masac_oracle.py: test_float32_against_float64 for the float32 oracle, test_reference_against_float64 for the reference's
# float32 recording), both stay under 6 % of every one of them in pair, hetero, spread3 and seq: nothing is widened there.
# `clamp` is the exception, in two different ways:
#   * LOSSES, against anything: at log_std = -20, std = 2e-9 and u - mean = std eps is at or under half an ulp of the mean, so float32
#     keeps none or a rounded part of each such column's eps^2 / 2 of log pi, and which it keeps hangs on the mean's last bit.  That is
#     the number format's, in the float32 oracle (122.3 x the loss tolerance against float64), in torch's float32 (123.5 x) and in the
#     kernel alike: the loss tolerance of this case is 4 x 123.5 whatever the engine is compared with.
#   * norms, parameters, Adam's m and log_alpha's exp_avg, against the REFERENCE'S RECORDING only: torch's autograd forms
#     d log pi / d std from two terms of size eps^2 / std = 5e8 that cancel to their last bits; its float32 recording is 30.8 x (norms),
#     2.9 x (parameters), 2.6 x (Adam's m) and 21 x (alpha's exp_avg, rtol 1e-3) from the float64 oracle.  The closed form of the oracle
#     and of the kernel has no such terms: the float32 ORACLE is at 0.09 (norms), 0.06 (parameters) and 0.05 (alpha) of the tolerance.
#     So those are 4 x the recording's gap against the recording, and the project's own against the oracle.
WIDEN = dict(clamp=dict(loss=4 * 123.5))                                                            # against the oracle and the recording
WIDEN_RECORDING = dict(clamp=dict(norm=4 * 30.8, param=4 * 2.9, m=4 * 2.6, alpha_m=4 * 21.0))       # against the recording only


def tolerances(name, against="oracle"):
    """against: "oracle" (the NumPy restatement) or "reference" (the recording of the reference's float32 run in masac.npz)"""
    w = dict(WIDEN.get(name, {}))
    if against == "reference":
        w.update(WIDEN_RECORDING.get(name, {}))
    else:
        assert against == "oracle", against
    return dict(loss=(1e-4 * w.get("loss", 1), 1e-6 * w.get("loss", 1)), norm=1e-3 * w.get("norm", 1),
                param=(5e-4 * w.get("param", 1), 5e-6 * w.get("param", 1)), m=2e-3 * w.get("m", 1), alpha=1e-5, alpha_m=1e-3 * w.get("alpha_m", 1))


def case(name):
    c = dict(COMMON)
    c.update(CASES[name])
    c["rew_scale"] = REW_SCALE[name]
    return c


def actor_layers(c, j):
    H, (O, A) = c["hidden"], c["dims"][j]
    return [("l1", H, O), ("l2", H, H), ("mean_layer", A, H), ("log_std_layer", A, H)]


def critic_layers(c):
    H, T = c["hidden"], sum(o + a for o, a in c["dims"])
    return [("l1", H, T), ("l2", H, H), ("l3", 1, H), ("l1_2", H, T), ("l2_2", H, H), ("l3_2", 1, H)]


def table(seed, n, c):
    """per agent: obs, next_obs ~ N(0,1), act ~ U(-1,1), rew ~ N(0,1) x rew_scale, done ~ Bernoulli(done_p) (per agent, both values)"""
    g = np.random.default_rng(seed)
    tabs = []
    for j, (O, A) in enumerate(c["dims"]):
        s = F32(c["rew_scale"][j])
        tabs.append(dict(obs=g.standard_normal((n, O)).astype(F32), next_obs=g.standard_normal((n, O)).astype(F32),
                         act=g.uniform(-1, 1, (n, A)).astype(F32), rew=(g.standard_normal(n).astype(F32) * s).astype(F32),
                         done=g.random(n) < c["done_p"]))
    return tabs


def inputs(c, n_learn=None, seed=None, batch=None):
    """-> actor / critic parameters per agent, the table, idx[call][agent] rows, eps[call][agent][set] draws [B, A_set]"""
    s = c["seed"] if seed is None else seed
    calls = c["n_learn"] if n_learn is None else n_learn
    n, na, B = c["n_table"], len(c["dims"]), batch or c["batch"]
    actor = [synth.mlp_params(s + 10 * j, actor_layers(c, j)) for j in range(na)]
    for p in actor:      # (clamp: the log_std head's outputs leave [-20, 2]; 1.0 elsewhere)
        p["log_std_layer.weight"] = (p["log_std_layer.weight"] * F32(c["ls_scale"])).astype(F32)
        p["log_std_layer.bias"] = (p["log_std_layer.bias"] * F32(c["ls_scale"])).astype(F32)
    critic = [synth.mlp_params(s + 10 * j + 1, critic_layers(c)) for j in range(na)]
    for p in critic:     # (seq: critics three times as steep, so that the twins differ and the other agents' actions matter; 1.0 elsewhere)
        for kk in p:
            p[kk] = (p[kk] * F32(c["critic_scale"])).astype(F32)
    set_dim = lambda i, st: c["dims"][i if st == 2 * na else st % na][1]
    return dict(actor=actor, critic=critic, table=table(s + 5, n, c),
                idx=[np.stack([synth.indices(s + 1000 + 10 * k + j, n, B) for j in range(na)]) for k in range(calls)],
                eps=[[[synth.normal(s + 5000 + 1000 * k + 50 * i + st, (B, set_dim(i, st))) for st in range(2 * na + 1)] for i in range(na)] for k in range(calls)])


def pad_eps(eps_call, n, B, am):
    """eps[agent][set] of one call -> the engine's noise block [n][2 n + 1][B][act_max], zero padded"""
    out = np.zeros((n, 2 * n + 1, B, am), F32)
    for i in range(n):
        for st in range(2 * n + 1):
            e = eps_call[i][st]
            out[i, st, :, :e.shape[1]] = e
    return out


def softplus(x):
    return np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))


def actor_forward(p, x, eps):
    """Actor.forward (MASAC.py:41-68) with the draw injected -> action, log_pi [B, 1], cache"""
    dt = x.dtype.type
    h1 = np.maximum(nn.linear(x, p, "l1"), dt(0))
    h2 = np.maximum(nn.linear(h1, p, "l2"), dt(0))
    mean, raw = nn.linear(h2, p, "mean_layer"), nn.linear(h2, p, "log_std_layer")
    ls = np.clip(raw, dt(-20), dt(2))
    sd = np.exp(ls)
    u = mean + sd * eps
    logp = (-((u - mean) ** 2) / (dt(2) * sd * sd) - np.log(sd) - dt(LOG_SQRT_2PI)).sum(axis=1, keepdims=True)
    logp = logp - (dt(2) * (dt(np.log(2)) - u - softplus(dt(-2) * u))).sum(axis=1, keepdims=True)
    a = np.tanh(u)
    return a, logp, dict(x=x, h1=h1, h2=h2, mean=mean, raw=raw, sd=sd, u=u, a=a, eps=eps)


def actor_backward(p, k, d_mean, d_raw):
    """head deltas (d loss / d mean, d loss / d raw log_std) -> grads keyed like p"""
    g = {"mean_layer.weight": d_mean.T @ k["h2"], "mean_layer.bias": d_mean.sum(axis=0),
         "log_std_layer.weight": d_raw.T @ k["h2"], "log_std_layer.bias": d_raw.sum(axis=0)}
    d = (d_mean @ p["mean_layer.weight"] + d_raw @ p["log_std_layer.weight"]) * (k["h2"] > 0)
    g["l2.weight"], g["l2.bias"] = d.T @ k["h1"], d.sum(axis=0)
    d = (d @ p["l2.weight"]) * (k["h1"] > 0)
    g["l1.weight"], g["l1.bias"] = d.T @ k["x"], d.sum(axis=0)
    return {kk: g[kk] for kk in p}


def clip_grad_norm(grads, max_norm, dt):
    norms = np.array([np.sqrt(np.sum(g.astype(dt) ** 2, dtype=dt)) for g in grads.values()], dtype=dt)
    total = np.sqrt(np.sum(norms ** 2, dtype=dt))
    coef = min(dt(max_norm) / (total + dt(1e-6)), dt(1.0))
    for kk in grads:
        grads[kk] = grads[kk] * dt(coef)
    return float(total)


class Adam:
    """oracle.nn.Adam's arithmetic (torch.optim.Adam's defaults and operation order) with its constants in the run's dtype: nn.Adam rounds
    them to float32 whatever the parameters are, which a float64 run against torch in double would see at 1e-8"""

    def __init__(self, params, lr, dt):
        self.lr, self.dt, self.t = float(lr), dt, 0
        self.m = {k: np.zeros_like(v) for k, v in params.items()}
        self.v = {k: np.zeros_like(v) for k, v in params.items()}

    def step(self, params, grads):
        dt = self.dt
        self.t += 1
        bc1, bc2 = 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t
        for k in params:
            g, m, v = grads[k], self.m[k], self.v[k]
            m += (g - m) * dt(1.0 - 0.9)
            v *= dt(0.999)
            v += dt(1.0 - 0.999) * g * g
            params[k] -= dt(self.lr / bc1) * (m / (np.sqrt(v) / dt(np.sqrt(bc2)) + dt(1e-8)))


class MASAC:
    """One learner.  Per agent: an actor, a twin critic, a deep copy of each as target, Adam (torch defaults) behind a global-norm clip at
    0.5 for each, log_alpha with Adam at 1e-4."""

    def __init__(self, c, inp, dtype=F32, stale_actors=False, one_draw=False, mean_twins=False):
        self.dims, self.dt, self.n = c["dims"], dtype, len(c["dims"])
        self.stale_actors, self.one_draw, self.mean_twins = stale_actors, one_draw, mean_twins
        cp = lambda p: {kk: np.array(v, dtype=dtype) for kk, v in p.items()}
        self.actor, self.actor_t = [cp(p) for p in inp["actor"]], [cp(p) for p in inp["actor"]]
        self.critic, self.critic_t = [cp(p) for p in inp["critic"]], [cp(p) for p in inp["critic"]]
        self.q1, self.q2 = nn.MLP(Q1), nn.MLP(Q2)
        self.aopt = [Adam(p, c["actor_lr"], dtype) for p in self.actor]
        self.copt = [Adam(p, c["critic_lr"], dtype) for p in self.critic]
        # Alpha (MASAC.py:124-139): log_alpha is a float32 tensor whatever the nets are; alpha = exp(log_alpha)
        a0 = c["alpha0"] or [0.01] * self.n
        self.log_alpha = [{"log_alpha": np.array(np.log(a0[j]), dtype=dtype)} for j in range(self.n)]
        self.alopt = [Adam(p, ALPHA_LR, dtype) for p in self.log_alpha]
        t = inp["table"]
        cast = lambda x: np.asarray(x, dtype)
        self.obs, self.act = [cast(x["obs"]) for x in t], [cast(x["act"]) for x in t]
        self.nobs = [cast(x["next_obs"]) for x in t]
        self.rew, self.done = [cast(x["rew"]) for x in t], [cast(x["done"]) for x in t]
        self.OT = sum(o for o, _ in self.dims)
        self.acol = np.concatenate([[0], np.cumsum([a for _, a in self.dims])])

    def alpha(self, i):
        return np.exp(self.log_alpha[i]["log_alpha"])

    def set_alpha(self, i, alpha):
        self.log_alpha[i]["log_alpha"] = np.array(np.log(alpha), dtype=self.dt)

    def q(self, p, obs_all, act_all):
        """-> (q1, q2) [B, 1] each, the two caches"""
        x = np.concatenate(list(obs_all) + list(act_all), axis=1)
        a, ka = self.q1.forward(p, x)
        b, kb = self.q2.forward(p, x)
        return a, b, ka, kb

    def learn_with(self, idx, eps, gamma, tau):
        """idx [n, B]; eps[i][set] [B, A].  -> dict of per-agent lists: critic_loss, actor_loss, critic_norm, actor_norm, alpha (after
        the agent's step), and what the generator's conditions look at: head0_target / head0_actor (share of rows whose minimum is Q1),
        raw_log_std (actor i's, actor stage), actor_grad"""
        dt, n = self.dt, self.n
        out = dict(critic_loss=[], actor_loss=[], critic_norm=[], actor_norm=[], alpha=[], head0_target=[], head0_actor=[], raw_log_std=[])
        before = [{kk: v.copy() for kk, v in p.items()} for p in self.actor]
        for i in range(n):
            rows = np.asarray(idx[i], np.int64)
            B = rows.size
            e = [np.asarray(x, dt) for x in eps[i]]
            obs, act, nobs = [o[rows] for o in self.obs], [a[rows] for a in self.act], [o[rows] for o in self.nobs]
            alpha = self.alpha(i)
            # -- critic (MASAC.py:224-242)
            nxt = [actor_forward(self.actor_t[j], nobs[j], e[j]) for j in range(n)]
            qa, qb, _, _ = self.q(self.critic_t[i], nobs, [x[0] for x in nxt])
            out["head0_target"].append(float(np.mean(qa < qb)))
            T = self.rew[i][rows][:, None] + dt(gamma) * (dt(1) - self.done[i][rows][:, None]) * (np.minimum(qa, qb) - alpha * nxt[i][1])
            q1, q2, k1, k2 = self.q(self.critic[i], obs, act)
            d1, d2 = q1 - T, q2 - T
            out["critic_loss"].append(dt(np.mean(d1 * d1, dtype=dt) + np.mean(d2 * d2, dtype=dt)))
            _, g1 = self.q1.backward(self.critic[i], k1, d1 * dt(2.0 / B), need_dx=False)
            _, g2 = self.q2.backward(self.critic[i], k2, d2 * dt(2.0 / B), need_dx=False)
            g = {kk: (g1[kk] if kk in g1 else g2[kk]) for kk in self.critic[i]}
            out["critic_norm"].append(clip_grad_norm(g, CLIP, dt))
            self.copt[i].step(self.critic[i], g)
            # -- actor (MASAC.py:254-267)
            src = lambda j: before[j] if (self.stale_actors and j != i) else self.actor[j]
            new = [actor_forward(src(j), obs[j], e[n + j]) for j in range(n)]
            a_i, _, k = new[i]
            _, lp2, kent = actor_forward(self.actor[i], obs[i], e[n + i] if self.one_draw else e[2 * n])
            q1, q2, k1, k2 = self.q(self.critic[i], obs, [x[0] for x in new])
            out["head0_actor"].append(float(np.mean(q1 < q2)))
            out["raw_log_std"].append(k["raw"].copy())
            if self.mean_twins:
                qpi, w0 = (q1 + q2) * dt(0.5), np.full_like(q1, dt(0.5))
            else:       # torch.min(a, b)'s backward: the smaller one takes the gradient, a tie splits it in halves
                qpi, w0 = np.minimum(q1, q2), np.where(q1 < q2, dt(1), np.where(q1 == q2, dt(0.5), dt(0)))
            out["actor_loss"].append(dt(np.mean(-qpi + alpha * lp2, dtype=dt)))
            dx1, _ = self.q1.backward(self.critic[i], k1, -w0 / dt(B))
            dx2, _ = self.q2.backward(self.critic[i], k2, -(dt(1) - w0) / dt(B))
            c0 = self.OT + int(self.acol[i])
            da = (dx1 + dx2)[:, c0:c0 + self.dims[i][1]]
            opened = ((k["raw"] >= dt(-20)) & (k["raw"] <= dt(2))).astype(dt)
            du1 = da * (dt(1) - a_i * a_i)
            kk_ = alpha / dt(B)
            t2 = np.tanh(kent["u"])
            d_mean = du1 + kk_ * dt(2) * t2
            d_raw = (du1 * k["sd"] * k["eps"] + kk_ * (dt(2) * t2 * kent["sd"] * kent["eps"] - dt(1))) * opened
            ga = actor_backward(self.actor[i], k, d_mean, d_raw)
            out["actor_norm"].append(clip_grad_norm(ga, CLIP, dt))
            self.aopt[i].step(self.actor[i], ga)
            # -- alpha (MASAC.py:271-273): d/d log_alpha of mean(alpha (-log_pi + A)) with alpha = exp(log_alpha)
            gl = alpha * np.mean(-lp2 + dt(self.dims[i][1]), dtype=dt)
            self.alopt[i].step(self.log_alpha[i], {"log_alpha": np.asarray(gl, dt)})
            out["alpha"].append(dt(self.alpha(i)))
        for i in range(n):
            nn.soft_update(self.actor_t[i], self.actor[i], tau)
            nn.soft_update(self.critic_t[i], self.critic[i], tau)
        return out


def make(c, inp, dtype=F32, **switches):
    o = MASAC(c, inp, dtype, **switches)
    return o


def compact_digest(tensors, names):
    """name.weight / name.bias tensors of `names` in order -> (float64 [T, 2] sum and abs-sum, float32 [T, 16] strided sample): what the
    fixture keeps of a net (two arrays per net: at several thousand tensors the archive's per-entry overhead is what counts)"""
    stats, sample = [], []
    for nme in names:
        for suf in (".weight", ".bias"):
            flat = np.asarray(tensors[nme + suf]).reshape(-1).astype(np.float64)
            stats.append([flat.sum(), np.abs(flat).sum()])
            sm = flat[::max(1, flat.size // 16)][:16]
            sample.append(np.pad(sm, (0, 16 - sm.size)))
    return np.array(stats, np.float64), np.array(sample, F32)


def check_digest(tensors, names, stats, sample, rtol, atol, label):
    """hold `tensors` to a compact_digest record: every sampled element within (rtol, atol), sum and abs-sum within rtol x abs-sum +
    atol x size"""
    got_stats, got_sample = compact_digest(tensors, names)
    np.testing.assert_allclose(got_sample, sample, rtol=rtol, atol=atol, err_msg=label + " samples")
    sizes = np.array([np.asarray(tensors[nme + suf]).size for nme in names for suf in (".weight", ".bias")], np.float64)
    tol = rtol * stats[:, 1] + atol * sizes
    assert np.all(np.abs(got_stats[:, 0] - stats[:, 0]) <= tol), label + " sums"
    assert np.all(np.abs(got_stats[:, 1] - stats[:, 1]) <= tol), label + " abs-sums"
