"""ATT-MADDPG (MADDPG_file/MADDPG_simple_with_tricks.py:91-208 with trick['ATT'], ATT.py:81-103,181-229) restated in NumPy: the attention
critic's forward and backward, the whole learn(), and the seeded inputs of its golden cases.  The golden generator
(tests/golden/make_att_golden.py) runs the reference on exactly these inputs; the CPU test (tests/test_att_oracle.py) holds this oracle
to its output and to torch autograd, the GPU test (tests/test_gpu_att.py) holds the HIP engine to both.

Per row, for agent i's critic (H hidden, K = 4 heads):
    x_e = [o_0 | .. | o_{n-1} | a_i]    x_d = [a_j, j != i]
    e = E x_e    d = D x_d                                   (no activation)
    g = relu(EI e)    h_k = relu(HEAD_k g)    u = relu(DI d)
    s_k = <h_k, u>    p = softmax_k(s)    c = sum_k p_k h_k
    y = relu(FC1 c)   Q = FC2 y
`dtype=np.float64` runs the same arithmetic in float64.
"""
import numpy as np

from oracle import nn
from tests.golden import synth

F32 = np.float32
K = 4
CLIP = 0.5
ACTOR_NAMES = ["l1", "l2", "l3"]
# the reference's state_dict order of ATT_critic (ATT.py:202-213)
CRITIC_NAMES = (["attention_modules.fc_encoder_input"] + ["attention_modules.fc_encoder_heads.%d" % k for k in range(K)] +
                ["attention_modules.fc_decoder_input", "encoder_input_fc", "decoder_input_fc", "fc1", "fc2"])
EI, DI, E_, D_, FC1, FC2 = CRITIC_NAMES[0], CRITIC_NAMES[5], CRITIC_NAMES[6], CRITIC_NAMES[7], CRITIC_NAMES[8], CRITIC_NAMES[9]
HEADS = CRITIC_NAMES[1:5]
# the engine's seven layers (csrc/frl_desc.h: AttLayer): the four heads stacked into one layer
ENGINE_NAMES = ["ei", "heads", "di", "E", "D", "fc1", "fc2"]

# name -> agents (obs, act), hidden, batch, learn() calls; rew_scale: see make_att_golden.py (norms on both sides of the clip)
CASES = {
    "spread3": dict(dims=[(18, 5)] * 3, hidden=128, batch=64, n_learn=3, seed=7100),
    "hetero": dict(dims=[(8, 1), (10, 2), (10, 1)], hidden=64, batch=17, n_learn=3, seed=7200),
    "pair": dict(dims=[(7, 4)] * 2, hidden=128, batch=5, n_learn=2, seed=7300),
    "spread5": dict(dims=[(30, 5)] * 5, hidden=128, batch=50, n_learn=2, seed=7400),
}
COMMON = dict(n_table=300, gamma=0.95, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, done_p=0.1, rew_scale=None)
# per-agent reward scales: agent 0's rewards are small (its critic's pre-clip norm stays under 0.5), the others' are O(1) and larger
REW_SCALE = dict(spread3=[0.02, 1.0, 3.0], hetero=[0.02, 1.0, 3.0], pair=[0.02, 2.0], spread5=[0.02, 0.5, 1.0, 2.0, 3.0])
CLASS = dict(dims=[(6, 2), (5, 3), (6, 2)], hidden=128, batch=8, seed=7900, capacity=64, n_steps=40, learn_from=20, learn_every=5, n_learn=5)


def case(name):
    c = dict(COMMON)
    c.update(CLASS if name == "class" else CASES[name])
    if name in REW_SCALE:
        c["rew_scale"] = REW_SCALE[name]
    return c


def actor_layers(c, j):
    H, (O, A) = c["hidden"], c["dims"][j]
    return [("l1", H, O), ("l2", H, H), ("l3", A, H)]


def critic_layers(c, i):
    """[(name, out, in)] in the reference's state_dict order"""
    H = c["hidden"]
    OT, AT, Ai = sum(o for o, _ in c["dims"]), sum(a for _, a in c["dims"]), c["dims"][i][1]
    return ([(EI, H, H)] + [(h, H, H) for h in HEADS] + [(DI, H, H), (E_, H, OT + Ai), (D_, H, AT - Ai), (FC1, H, H), (FC2, 1, H)])


def to_engine(p):
    """reference-keyed critic parameters -> the engine's seven layers (name.weight / name.bias), the heads stacked along the output rows"""
    out = {}
    for en, rn in zip(ENGINE_NAMES, [EI, None, DI, E_, D_, FC1, FC2]):
        if rn is None:
            out[en + ".weight"] = np.concatenate([p[h + ".weight"] for h in HEADS], axis=0)
            out[en + ".bias"] = np.concatenate([p[h + ".bias"] for h in HEADS], axis=0)
        else:
            out[en + ".weight"], out[en + ".bias"] = p[rn + ".weight"], p[rn + ".bias"]
    return out


def table(seed, n, c):
    """per agent: obs, next_obs ~ N(0,1), act ~ U(-1,1), rew ~ N(0,1) x rew_scale, done ~ Bernoulli(done_p) (per agent, both values)"""
    g = np.random.default_rng(seed)
    tabs = []
    for j, (O, A) in enumerate(c["dims"]):
        s = F32(c["rew_scale"][j]) if c.get("rew_scale") else F32(1)
        tabs.append(dict(obs=g.standard_normal((n, O)).astype(F32), next_obs=g.standard_normal((n, O)).astype(F32),
                         act=g.uniform(-1, 1, (n, A)).astype(F32), rew=(g.standard_normal(n).astype(F32) * s).astype(F32),
                         done=g.random(n) < c["done_p"]))
    return tabs


def inputs(c, n_learn=None, seed=None, batch=None):
    s = c["seed"] if seed is None else seed
    calls = c["n_learn"] if n_learn is None else n_learn
    n, na, B = c.get("n_steps", c["n_table"]), len(c["dims"]), batch or c["batch"]
    return dict(actor=[synth.mlp_params(s + 10 * j, actor_layers(c, j)) for j in range(na)],
                critic=[synth.mlp_params(s + 10 * j + 1, critic_layers(c, j)) for j in range(na)],
                table=table(s + 5, n, c),
                idx=[np.stack([synth.indices(s + 1000 + 10 * k + j, n, B) for j in range(na)]) for k in range(calls)])


# ----------------------------------------------------------------------------------- the critic
def split_inputs(dims, i, obs_all, act_all):
    """[all obs], [all actions] (lists, agent order) -> x_e, x_d of agent i's critic"""
    xe = np.concatenate(list(obs_all) + [act_all[i]], axis=1)
    xd = np.concatenate([act_all[j] for j in range(len(dims)) if j != i], axis=1)
    return xe, xd


def critic_forward(p, xe, xd):
    """-> Q [B, 1], cache"""
    lin = nn.linear
    dt = xe.dtype
    e, d = lin(xe, p, E_), lin(xd, p, D_)
    g = np.maximum(lin(e, p, EI), dt.type(0))
    u = np.maximum(lin(d, p, DI), dt.type(0))
    h = np.stack([np.maximum(lin(g, p, hn), dt.type(0)) for hn in HEADS], axis=1)          # [B, K, H]
    s = np.einsum("bkh,bh->bk", h, u)
    ex = np.exp(s - s.max(axis=1, keepdims=True))
    pr = ex / ex.sum(axis=1, keepdims=True)
    c = np.einsum("bk,bkh->bh", pr, h)
    y = np.maximum(lin(c, p, FC1), dt.type(0))
    q = lin(y, p, FC2)
    return q, dict(xe=xe, xd=xd, e=e, d=d, g=g, u=u, h=h, s=s, p=pr, c=c, y=y)


def critic_backward(p, k, dq, need_dx=False):
    """dq [B, 1] -> (d loss / d x_e or None, grads keyed like p)"""
    gr = {}

    def back(name, dy, x):
        gr[name + ".weight"], gr[name + ".bias"] = dy.T @ x, dy.sum(axis=0)
        return dy @ p[name + ".weight"]
    dy = back(FC2, dq, k["y"]) * (k["y"] > 0)
    dc = back(FC1, dy, k["c"])
    h, u, pr = k["h"], k["u"], k["p"]
    dp = np.einsum("bh,bkh->bk", dc, h)
    ds = pr * (dp - np.sum(pr * dp, axis=1, keepdims=True))
    dh = (pr[:, :, None] * dc[:, None, :] + ds[:, :, None] * u[:, None, :]) * (h > 0)
    du = np.einsum("bk,bkh->bh", ds, h) * (u > 0)
    dg = sum(back(hn, dh[:, j], k["g"]) for j, hn in enumerate(HEADS)) * (k["g"] > 0)
    dd = back(DI, du, k["d"])
    de = back(EI, dg, k["e"])
    back(D_, dd, k["xd"])
    dxe = back(E_, de, k["xe"])
    return (dxe if need_dx else None), {kk: gr[kk] for kk in p}


def clip_grad_norm(grads, max_norm, dt):
    norms = np.array([np.sqrt(np.sum(g.astype(dt) ** 2, dtype=dt)) for g in grads.values()], dtype=dt)
    total = np.sqrt(np.sum(norms ** 2, dtype=dt))
    coef = min(dt(max_norm) / (total + dt(1e-6)), dt(1.0))
    for kk in grads:
        grads[kk] = grads[kk] * dt(coef)
    return float(total)


class AttMADDPG:
    """One learner: per agent an actor l1..l3 (tanh head) and an attention critic, a deep copy of each as target, Adam (torch defaults)
    behind a global-norm clip at 0.5 for each; learn() = per agent critic step then actor step through the stepped critic, then every
    target moves by tau."""

    def __init__(self, c, inp, dtype=F32):
        self.dims, self.dt, self.n = c["dims"], dtype, len(c["dims"])
        cp = lambda p: {kk: np.array(v, dtype=dtype) for kk, v in p.items()}
        self.actor, self.actor_t = [cp(p) for p in inp["actor"]], [cp(p) for p in inp["actor"]]
        self.critic, self.critic_t = [cp(p) for p in inp["critic"]], [cp(p) for p in inp["critic"]]
        self.anet = nn.MLP(ACTOR_NAMES, out_act="tanh")
        self.aopt = [nn.Adam(p, c["actor_lr"]) for p in self.actor]
        self.copt = [nn.Adam(p, c["critic_lr"]) for p in self.critic]
        t = inp["table"]
        cast = lambda x: np.asarray(x, dtype)
        self.obs, self.act = [cast(x["obs"]) for x in t], [cast(x["act"]) for x in t]
        self.nobs = [cast(x["next_obs"]) for x in t]
        self.rew, self.done = [cast(x["rew"]) for x in t], [cast(x["done"]) for x in t]

    def q(self, p, i, obs_all, act_all):
        xe, xd = split_inputs(self.dims, i, obs_all, act_all)
        return critic_forward(p, xe, xd)

    def learn_with(self, idx, gamma, tau, do_actor=True, agents=None):
        """idx [n, B]: agent i's rows.  -> dict of per-agent lists: critic_loss, actor_loss, critic_norm, actor_norm, q (the online
        critic's Q of the sampled rows before the step), q_target (critic_target's on the same stored rows)"""
        dt, n = self.dt, self.n
        out = dict(critic_loss=[], actor_loss=[], critic_norm=[], actor_norm=[], q=[], q_target=[])
        for i in (range(n) if agents is None else agents):
            rows = np.asarray(idx[i], np.int64)
            B = rows.size
            obs, act, nobs = [o[rows] for o in self.obs], [a[rows] for a in self.act], [o[rows] for o in self.nobs]
            nact = [self.anet.forward(self.actor_t[j], nobs[j])[0] for j in range(n)]
            qn, _ = self.q(self.critic_t[i], i, nobs, nact)
            T = self.rew[i][rows][:, None] + dt(gamma) * qn * (dt(1) - self.done[i][rows][:, None])
            Q, cache = self.q(self.critic[i], i, obs, act)
            out["q"].append(Q[:, 0].copy())
            out["q_target"].append(self.q(self.critic_t[i], i, obs, act)[0][:, 0].copy())
            diff = Q - T
            out["critic_loss"].append(dt(np.mean(diff * diff, dtype=dt)))
            _, g = critic_backward(self.critic[i], cache, diff * dt(2.0 / B))
            out["critic_norm"].append(clip_grad_norm(g, CLIP, dt))
            self.copt[i].step(self.critic[i], g)
            if not do_actor:
                continue
            a, aacts = self.anet.forward(self.actor[i], obs[i])
            act2 = list(act)
            act2[i] = a
            Q2, cache2 = self.q(self.critic[i], i, obs, act2)
            out["actor_loss"].append(dt(-np.mean(Q2, dtype=dt)))
            dxe, _ = critic_backward(self.critic[i], cache2, np.full((B, 1), dt(-1.0 / B), dt), need_dx=True)
            OT = sum(o for o, _ in self.dims)
            _, ga = self.anet.backward(self.actor[i], aacts, dxe[:, OT:], need_dx=False)
            ga = {kk: ga[kk] for kk in self.actor[i]}
            out["actor_norm"].append(clip_grad_norm(ga, CLIP, dt))
            self.aopt[i].step(self.actor[i], ga)
        if do_actor:
            for i in range(n):
                nn.soft_update(self.actor_t[i], self.actor[i], tau)
                nn.soft_update(self.critic_t[i], self.critic[i], tau)
        return out


def compact_digest(tensors, names):
    """name.weight / name.bias tensors of `names` in order -> (float64 [T, 2] sum and abs-sum, float32 [T, 16] strided sample): what
    the fixture keeps of a net (two arrays per net, not three entries per tensor: the archive's per-entry overhead is what counts)"""
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


def make(c, inp, dtype=F32):
    return AttMADDPG(c, inp, dtype)


def class_schedule(c):
    return [t for t in range(c["n_steps"]) if t + 1 >= c["learn_from"] and (t + 1 - c["learn_from"]) % c["learn_every"] == 0][:c["n_learn"]]
