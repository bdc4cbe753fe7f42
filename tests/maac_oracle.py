"""MAAC (MAAC_file/MAAC_discrete.py:44-75,106-131,208-280 with attention = True, adaptive_alpha = False; Attention.py:63-231 with
is_continue = False) restated in NumPy: the attention critic's forward and closed-form backward and the whole learn() with injected row
indices and Exp(1) draws, in float32 or float64, and the seeded inputs of its cases.  The CPU test (tests/test_maac_oracle.py) holds this
oracle to torch autograd + clip_grad_norm_ + torch.optim.Adam in double; tests/test_maac_golden.py holds it to the recording of the
imported reference class (tests/golden/maac.npz).  No engine runs MAAC yet (DESIGN.md "MAAC: what is pinned ahead of a port"): the
tolerances below are the ones a GPU test of a port will use.

Per updating agent i, in agent order: rows idx[i]; draws eps[i][s] ~ Exp(1), [B, A]: s = j the target actor j's, s = n + j the online
actor j's draw 1, s = 2 n the second draw of actor i.  A draw is argmax_k probs[k] / eps[k] (torch.multinomial's single-sample rule).

One `Attention` block is shared by every agent's ONLINE critic (a default argument evaluated once, Attention.py:118); each target critic
holds its own copy; each agent's Adam steps the shared block from its own moments.  Agent i's loss never reaches its own encoder_fc_sa,
encoder_fc_a, bias_fc1, bias_fc2: they stay as loaded and have no Adam state.

Five switches exist only to prove that the tests tell the reference's semantics from near misses: `own_attention` (no sharing: every
agent trains a copy of its own), `final_attention` (the actor stages read the block after ALL critics have stepped it), `one_draw`
(log_pi of draw 1), `stale_actors` (the actor stage reads the other agents' online actors as they were before the call), `detach_probs`
(probs detached in v).
"""
import numpy as np

from tests.golden import synth
from tests.masac_oracle import Adam, check_digest, clip_grad_norm, compact_digest  # noqa: F401  (re-exported)

F32 = np.float32
CLIP = 0.5
HEADS = 4
SLOPE = 0.01
ACTOR_NAMES = ["l1", "l2", "l3"]
ATT_KEYS = ["attention.query.weight", "attention.key.weight", "attention.value.0.weight", "attention.value.0.bias",
            "attention.fc_out.weight", "attention.fc_out.bias"]
OWN_LAYERS = ["encoder_fc_s", "encoder_fc_sa", "encoder_fc_a", "fc1", "fc2", "bias_fc1", "bias_fc2"]
CRITIC_KEYS = ATT_KEYS + [n + s for n in OWN_LAYERS for s in (".weight", ".bias")]          # the 20 state_dict keys, in order
FROZEN_LAYERS = ["encoder_fc_sa", "encoder_fc_a", "bias_fc1", "bias_fc2"]
FROZEN_KEYS = [n + s for n in FROZEN_LAYERS for s in (".weight", ".bias")]                   # 8 tensors nothing trains
TRAINED_KEYS = [k for k in CRITIC_KEYS if k not in FROZEN_KEYS]                              # 12 tensors agent i's optimiser moves

# name -> agents (obs, actions), hidden, batch.  Every case: 3 learn() calls, compared after the 1st and the 3rd.
#   pair     one other agent: the softmax over the others is 1 and its backward is zero; no full 16-row chunk
#   hetero   unequal observation and action widths; one full chunk plus one row
#   spread3  simple_spread_v3 with N = 3; four full chunks
#   spread5  the script's own shape (N = 5); a ragged last chunk
#   eight    the most agents an engine takes; hidden 64
#   wide17   an agent with 17 actions: the all_q head and the actor's head pass a 16-column tile
#   b1 / b15 / b33   hetero's nets at hidden 64 with batches where no chunk is full or the last one is short
CASES = {
    "pair": dict(dims=[(7, 4)] * 2, hidden=128, batch=5, seed=9100),
    "hetero": dict(dims=[(8, 3), (6, 2), (8, 5)], hidden=128, batch=17, seed=9200),
    "spread3": dict(dims=[(18, 5)] * 3, hidden=128, batch=64, seed=9300),
    "spread5": dict(dims=[(30, 5)] * 5, hidden=128, batch=50, seed=9400),
    "eight": dict(dims=[(5, 2)] * 8, hidden=64, batch=16, seed=9500),
    "wide17": dict(dims=[(6, 17), (9, 3), (4, 2)], hidden=64, batch=20, seed=9600),
    "b1": dict(dims=[(8, 3), (6, 2), (8, 5)], hidden=64, batch=1, seed=9700),
    "b15": dict(dims=[(8, 3), (6, 2), (8, 5)], hidden=64, batch=15, seed=9710),
    "b33": dict(dims=[(8, 3), (6, 2), (8, 5)], hidden=64, batch=33, seed=9720),
}
# att_scale: query / key weights are this much larger than nn.Linear's default range, so that the attention weights differ between the
# other agents; actor_lr / critic_lr above the script's 1e-3 so that three calls move what the switches are about
COMMON = dict(n_table=300, n_learn=3, gamma=0.95, tau=0.01, actor_lr=5e-3, critic_lr=5e-3, done_p=0.1, alpha=0.1, att_scale=4.0)
RECORD_AFTER = (1, 3)
# The project's tolerances (tests/test_gpu_envelope_ddpg.py): losses rtol 1e-4 / atol 1e-6, norms rtol 1e-3, parameters rtol 5e-4 / atol 5e-6
# on >= 99 % of a tensor's elements, Adam's m 2e-3 of a tensor's largest |m|.  Nothing is widened: tests/test_maac_oracle.py
# (test_float32_against_float64) measures the float32 oracle against the float64 one as a share of each and asserts it stays under 1/4.
TOL = dict(loss=(1e-4, 1e-6), norm=1e-3, param=(5e-4, 5e-6), m=2e-3)


def case(name):
    c = dict(COMMON)
    c.update(CASES[name])
    n = len(c["dims"])
    # per-agent reward scales: agent 0's rewards are small (its critic's pre-clip norm stays under 0.5), the others' O(1) and larger
    c["rew_scale"] = [0.02] + [1.0 + 2.0 * (j - 1) / max(1, n - 2) for j in range(1, n)]
    return c


def actor_layers(c, j):
    H, (O, A) = c["hidden"], c["dims"][j]
    return [("l1", H, O), ("l2", H, H), ("l3", A, H)]


def own_layers(c, j):
    H, (O, A) = c["hidden"], c["dims"][j]
    return [("encoder_fc_s", H, O), ("encoder_fc_sa", H, O + A), ("encoder_fc_a", H, A), ("fc1", H, 2 * H), ("fc2", A, H), ("bias_fc1", H, H), ("bias_fc2", 1, H)]


def critic_shapes(c, j):
    """[(key, shape)] of agent j's critic in state_dict order"""
    H = c["hidden"]
    out = [("attention.query.weight", (H, H)), ("attention.key.weight", (H, H)), ("attention.value.0.weight", (H, H)), ("attention.value.0.bias", (H,)),
           ("attention.fc_out.weight", (H, H)), ("attention.fc_out.bias", (H,))]
    for nme, o, i in own_layers(c, j):
        out += [(nme + ".weight", (o, i)), (nme + ".bias", (o,))]
    return out


def flat_critic(p):
    return np.concatenate([np.asarray(p[k], F32).reshape(-1) for k in CRITIC_KEYS])


def unflat_critic(flat, c, j):
    out, o = {}, 0
    for k, shp in critic_shapes(c, j):
        sz = int(np.prod(shp))
        out[k] = np.array(flat[o:o + sz], copy=True).reshape(shp)
        o += sz
    assert o == flat.size, (o, flat.size)
    return out


def table(seed, n, c):
    """per agent: obs, next_obs ~ N(0,1), act = one-hot of a uniform index, rew ~ N(0,1) x rew_scale, done ~ Bernoulli(done_p)"""
    g = np.random.default_rng(seed)
    tabs = []
    for j, (O, A) in enumerate(c["dims"]):
        s = F32(c["rew_scale"][j])
        k = g.integers(0, A, n)
        tabs.append(dict(obs=g.standard_normal((n, O)).astype(F32), next_obs=g.standard_normal((n, O)).astype(F32),
                         act=np.eye(A, dtype=F32)[k], rew=(g.standard_normal(n).astype(F32) * s).astype(F32), done=g.random(n) < c["done_p"]))
    return tabs


def inputs(c, n_learn=None, seed=None, batch=None):
    """-> actor parameters and the critic's own layers per agent, the ONE attention block, the table, idx[call][agent] rows,
    eps[call][agent][set] Exp(1) draws [B, A_set]"""
    s = c["seed"] if seed is None else seed
    calls = c["n_learn"] if n_learn is None else n_learn
    n, na, B, H = c["n_table"], len(c["dims"]), batch or c["batch"], c["hidden"]
    actor = [synth.mlp_params(s + 10 * j, actor_layers(c, j)) for j in range(na)]
    own = [synth.mlp_params(s + 10 * j + 1, own_layers(c, j)) for j in range(na)]
    a = synth.mlp_params(s + 7, [("query", H, H), ("key", H, H), ("value.0", H, H), ("fc_out", H, H)])
    att = {"attention.query.weight": (a["query.weight"] * F32(c["att_scale"])).astype(F32), "attention.key.weight": (a["key.weight"] * F32(c["att_scale"])).astype(F32),
           "attention.value.0.weight": a["value.0.weight"], "attention.value.0.bias": a["value.0.bias"],
           "attention.fc_out.weight": a["fc_out.weight"], "attention.fc_out.bias": a["fc_out.bias"]}
    set_dim = lambda i, st: c["dims"][i if st == 2 * na else st % na][1]
    expo = lambda sd, shape: np.random.default_rng(sd).standard_exponential(shape).astype(F32)
    return dict(actor=actor, own=own, att=att, table=table(s + 5, n, c),
                idx=[np.stack([synth.indices(s + 1000 + 10 * k + j, n, B) for j in range(na)]) for k in range(calls)],
                eps=[[[expo(s + 5000 + 1000 * k + 50 * i + st, (B, set_dim(i, st))) for st in range(2 * na + 1)] for i in range(na)] for k in range(calls)])


def critic_params(inp, j):
    """agent j's critic as loaded: the 20 tensors"""
    p = dict(inp["att"])
    p.update(inp["own"][j])
    return {k: p[k] for k in CRITIC_KEYS}


def pad_eps(eps_call, n, B, am):
    """eps[agent][set] of one call -> the engine's noise block [n][2 n + 1][B][act_max], padded with ones (a padded column is never read)"""
    out = np.ones((n, 2 * n + 1, B, am), F32)
    for i in range(n):
        for st in range(2 * n + 1):
            e = eps_call[i][st]
            out[i, st, :, :e.shape[1]] = e
    return out


def leaky(x):
    return np.where(x > 0, x, x.dtype.type(SLOPE) * x)


def dleaky(h):
    """derivative from the activation's OUTPUT"""
    return np.where(h > 0, h.dtype.type(1), h.dtype.type(SLOPE))


def lin(x, p, name):
    return x @ p[name + ".weight"].T + p[name + ".bias"]


def actor_forward(p, x, eps):
    """Actor_discrete.forward (MAAC_discrete.py:51-75) with the Exp(1) draw injected -> index [B], log_pi [B, 1], probs [B, A], one-hot [B, A], cache"""
    dt = x.dtype.type
    h1 = leaky(lin(x, p, "l1"))
    h2 = leaky(lin(h1, p, "l2"))
    z = lin(h2, p, "l3")
    zs = z - z.max(axis=1, keepdims=True)
    ez = np.exp(zs)
    ssum = ez.sum(axis=1, keepdims=True)
    probs = ez / ssum
    cat = probs / probs.sum(axis=1, keepdims=True)          # Categorical(probs) renormalises
    k = np.argmax(cat / np.asarray(eps, dt), axis=1)         # torch.multinomial, one sample: argmax(probs / q), q ~ Exp(1)
    logp = (zs - np.log(ssum))[np.arange(len(k)), k][:, None]
    onehot = np.eye(z.shape[1], dtype=x.dtype)[k]
    return k, logp, probs, onehot, dict(x=x, h1=h1, h2=h2)


def actor_backward(p, k, dz):
    g = {"l3.weight": dz.T @ k["h2"], "l3.bias": dz.sum(axis=0)}
    d = (dz @ p["l3.weight"]) * dleaky(k["h2"])
    g["l2.weight"], g["l2.bias"] = d.T @ k["h1"], d.sum(axis=0)
    d = (d @ p["l2.weight"]) * dleaky(k["h1"])
    g["l1.weight"], g["l1.bias"] = d.T @ k["x"], d.sum(axis=0)
    return {kk: g[kk] for kk in p}


def critic_forward(own, att, enc_sa, i, obs, act):
    """Attention_Critic.forward (Attention.py:163-231) of agent i: `own` its own layers, `att` the attention block it holds (keys with
    the attention. prefix), enc_sa[j] the parameters agent j's ONLINE critic holds (its encoder_fc_sa is read).  -> all_q [B, A_i], cache"""
    dt = obs[0].dtype.type
    n = len(obs)
    s = leaky(lin(obs[i], own, "encoder_fc_s"))
    q = s @ att["attention.query.weight"].T
    others = [j for j in range(n) if j != i]
    xs = [np.concatenate([obs[j], act[j]], axis=1) for j in others]
    e = [leaky(lin(xs[k], enc_sa[j], "encoder_fc_sa")) for k, j in enumerate(others)]
    K = [ek @ att["attention.key.weight"].T for ek in e]
    V = [leaky(ek @ att["attention.value.0.weight"].T + att["attention.value.0.bias"]) for ek in e]
    B, H = q.shape
    d = H // HEADS
    qh = q.reshape(B, HEADS, d)
    z = np.stack([(qh * Kk.reshape(B, HEADS, d)).sum(axis=2) for Kk in K], axis=1) / dt(np.sqrt(d))      # [B, nk, heads]
    zs = z - z.max(axis=1, keepdims=True)
    w = np.exp(zs)
    w = w / w.sum(axis=1, keepdims=True)
    attv = sum(w[:, k, :, None] * V[k].reshape(B, HEADS, d) for k in range(len(others))).reshape(B, H)
    other = attv @ att["attention.fc_out.weight"].T + att["attention.fc_out.bias"]
    x2 = np.concatenate([s, other], axis=1)
    y1 = leaky(lin(x2, own, "fc1"))
    all_q = lin(y1, own, "fc2")
    return all_q, dict(o=obs[i], s=s, q=q, xs=xs, e=e, K=K, V=V, w=w, attv=attv, x2=x2, y1=y1, d=d)


def critic_backward(own, att, k, d_allq):
    """d loss / d all_q -> the gradients of the 12 trained tensors (CRITIC_KEYS' names).  Nothing flows into e_j's encoder."""
    dt = d_allq.dtype.type
    B, H = k["q"].shape
    d = k["d"]
    g = {"fc2.weight": d_allq.T @ k["y1"], "fc2.bias": d_allq.sum(axis=0)}
    dy = (d_allq @ own["fc2.weight"]) * dleaky(k["y1"])
    g["fc1.weight"], g["fc1.bias"] = dy.T @ k["x2"], dy.sum(axis=0)
    dx2 = dy @ own["fc1.weight"]
    ds, dother = dx2[:, :H], dx2[:, H:]
    g["attention.fc_out.weight"], g["attention.fc_out.bias"] = dother.T @ k["attv"], dother.sum(axis=0)
    datt = (dother @ att["attention.fc_out.weight"]).reshape(B, HEADS, d)
    nk = len(k["V"])
    dw = np.stack([(datt * k["V"][j].reshape(B, HEADS, d)).sum(axis=2) for j in range(nk)], axis=1)      # [B, nk, heads]
    dz = k["w"] * (dw - (k["w"] * dw).sum(axis=1, keepdims=True)) / dt(np.sqrt(d))
    qh = k["q"].reshape(B, HEADS, d)
    dq = np.zeros_like(k["q"])
    gk, gv, gvb = 0, 0, 0
    for j in range(nk):
        dq = dq + (dz[:, j, :, None] * k["K"][j].reshape(B, HEADS, d)).reshape(B, H)
        dK = (dz[:, j, :, None] * qh).reshape(B, H)
        dV = (k["w"][:, j, :, None] * datt).reshape(B, H) * dleaky(k["V"][j])
        gk = gk + dK.T @ k["e"][j]
        gv = gv + dV.T @ k["e"][j]
        gvb = gvb + dV.sum(axis=0)
    g["attention.key.weight"], g["attention.value.0.weight"], g["attention.value.0.bias"] = gk, gv, gvb
    g["attention.query.weight"] = dq.T @ k["s"]
    ds = (ds + dq @ att["attention.query.weight"]) * dleaky(k["s"])
    g["encoder_fc_s.weight"], g["encoder_fc_s.bias"] = ds.T @ k["o"], ds.sum(axis=0)
    return {kk: g[kk] for kk in TRAINED_KEYS}


class MAAC:
    """One learner.  Per agent: an actor, a critic's own seven layers, deep copies of both and of the attention block as targets, Adam
    (torch defaults) behind a global-norm clip at 0.5 for the actor and for the critic's 12 trained tensors; alpha is a constant."""

    def __init__(self, c, inp, dtype=F32, own_attention=False, final_attention=False, one_draw=False, stale_actors=False, detach_probs=False):
        self.dims, self.dt, self.n = c["dims"], dtype, len(c["dims"])
        self.own_attention, self.final_attention, self.one_draw = own_attention, final_attention, one_draw
        self.stale_actors, self.detach_probs = stale_actors, detach_probs
        cp = lambda p: {kk: np.array(v, dtype=dtype) for kk, v in p.items()}
        n = self.n
        self.actor, self.actor_t = [cp(p) for p in inp["actor"]], [cp(p) for p in inp["actor"]]
        self.own, self.own_t = [cp(p) for p in inp["own"]], [cp(p) for p in inp["own"]]
        shared = cp(inp["att"])
        self.att = [cp(inp["att"]) for _ in range(n)] if own_attention else [shared] * n      # (the same dict n times: ONE block)
        self.att_t = [cp(inp["att"]) for _ in range(n)]
        self.alpha = [dtype(c["alpha"])] * n
        self.aopt = [Adam(p, c["actor_lr"], dtype) for p in self.actor]
        self.copt = [Adam(self.trained(i), c["critic_lr"], dtype) for i in range(n)]
        t = inp["table"]
        cast = lambda x: np.asarray(x, dtype)
        self.obs, self.act = [cast(x["obs"]) for x in t], [cast(x["act"]) for x in t]
        self.nobs = [cast(x["next_obs"]) for x in t]
        self.rew, self.done = [cast(x["rew"]) for x in t], [cast(x["done"]) for x in t]

    def trained(self, i):
        """the 12 tensors agent i's optimiser steps: views of the own layers and of the (shared) attention block, updated in place"""
        p = dict(self.att[i])
        p.update(self.own[i])
        return {k: p[k] for k in TRAINED_KEYS}

    def critic(self, i, target=False):
        """agent i's critic as its state_dict: 20 tensors"""
        p = dict(self.att_t[i] if target else self.att[i])
        p.update(self.own_t[i] if target else self.own[i])
        return {k: p[k] for k in CRITIC_KEYS}

    def all_q(self, i, obs, act, target=False):
        return critic_forward(self.own_t[i] if target else self.own[i], self.att_t[i] if target else self.att[i], self.own, i, obs, act)

    def _critic_step(self, i, rows, e, gamma, out):
        dt, n = self.dt, self.n
        B = rows.size
        obs, act, nobs = [o[rows] for o in self.obs], [a[rows] for a in self.act], [o[rows] for o in self.nobs]
        nxt = [actor_forward(self.actor_t[j], nobs[j], e[j]) for j in range(n)]
        aq, _ = self.all_q(i, nobs, [x[3] for x in nxt], target=True)
        qn = aq[np.arange(B), nxt[i][0]][:, None]
        T = self.rew[i][rows][:, None] + dt(gamma) * (dt(1) - self.done[i][rows][:, None]) * (qn - self.alpha[i] * nxt[i][1])
        aq, k = self.all_q(i, obs, act)
        pick = np.argmax(act[i], axis=1)
        dlt = aq[np.arange(B), pick][:, None] - T
        out["critic_loss"].append(dt(np.mean(dlt * dlt, dtype=dt)))
        d_allq = np.zeros_like(aq)
        d_allq[np.arange(B), pick] = (dlt * dt(2.0 / B))[:, 0]
        g = critic_backward(self.own[i], self.att[i], k, d_allq)
        out["critic_norm"].append(clip_grad_norm(g, CLIP, dt))
        self.copt[i].step(self.trained(i), g)
        out["att_spread"].append(float(np.mean((k["w"].max(axis=1) - k["w"].min(axis=1)).max(axis=1) >= 0.05)) if n > 2 else 1.0)

    def _actor_step(self, i, rows, e, before, out):
        dt, n = self.dt, self.n
        B = rows.size
        obs = [o[rows] for o in self.obs]
        src = lambda j: before[j] if (self.stale_actors and j != i) else self.actor[j]
        new = [actor_forward(src(j), obs[j], e[n + j]) for j in range(n)]
        a1 = new[i][0]
        a2, lp, probs, _, k = actor_forward(self.actor[i], obs[i], e[n + i] if self.one_draw else e[2 * n])
        aq, _ = self.all_q(i, obs, [x[3] for x in new])
        qpi = aq[np.arange(B), a1][:, None]
        v = (aq * probs).sum(axis=1, keepdims=True)
        alpha = self.alpha[i]
        out["actor_loss"].append(dt(np.mean(lp * (v - qpi + alpha * lp), dtype=dt)))
        out["draws_differ"].append(float(np.mean(a1 != a2)))
        onehot2 = np.eye(aq.shape[1], dtype=dt)[a2]
        dz = (v - qpi + dt(2) * alpha * lp) * (onehot2 - probs)
        if not self.detach_probs:
            dz = dz + lp * probs * (aq - v)
        ga = actor_backward(self.actor[i], k, dz / dt(B))
        out["actor_norm"].append(clip_grad_norm(ga, CLIP, dt))
        self.aopt[i].step(self.actor[i], ga)

    def learn_with(self, idx, eps, gamma, tau):
        """idx [n, B]; eps[i][set] [B, A].  -> dict of per-agent lists: critic_loss, actor_loss, critic_norm, actor_norm, and what the
        conditions look at: att_spread (share of rows whose attention weights differ by >= 0.05 between two other agents in some head),
        draws_differ (share of rows with draw 1 != draw 2)"""
        dt, n = self.dt, self.n
        out = dict(critic_loss=[], actor_loss=[], critic_norm=[], actor_norm=[], att_spread=[], draws_differ=[])
        before = [{kk: v.copy() for kk, v in p.items()} for p in self.actor]
        rows = [np.asarray(idx[i], np.int64) for i in range(n)]
        ee = [[np.asarray(x, dt) for x in eps[i]] for i in range(n)]
        if self.final_attention:
            for i in range(n):
                self._critic_step(i, rows[i], ee[i], gamma, out)
            for i in range(n):
                self._actor_step(i, rows[i], ee[i], before, out)
        else:
            for i in range(n):
                self._critic_step(i, rows[i], ee[i], gamma, out)
                self._actor_step(i, rows[i], ee[i], before, out)
        tk, tt = dt(1.0 - tau), dt(tau)
        for i in range(n):
            for tgt, srcp in ((self.actor_t[i], self.actor[i]), (self.own_t[i], self.own[i]), (self.att_t[i], self.att[i])):
                for kk in tgt:
                    tgt[kk] = tgt[kk] * tk + srcp[kk] * tt
        return out


def make(c, inp, dtype=F32, **switches):
    return MAAC(c, inp, dtype, **switches)


def digest_keys(tensors, keys):
    """the tensors of `keys` in order -> (float64 [T, 2] sum and abs-sum, float32 [T, 16] strided sample): what the fixture keeps of a net"""
    stats, sample = [], []
    for k in keys:
        flat = np.asarray(tensors[k]).reshape(-1).astype(np.float64)
        stats.append([flat.sum(), np.abs(flat).sum()])
        sm = flat[::max(1, flat.size // 16)][:16]
        sample.append(np.pad(sm, (0, 16 - sm.size)))
    return np.array(stats, np.float64), np.array(sample, F32)


def check_keys(tensors, keys, stats, sample, rtol, atol, label):
    """hold `tensors` to a digest_keys record: every sampled element within (rtol, atol), sum and abs-sum within rtol x abs-sum + atol x size"""
    got_stats, got_sample = digest_keys(tensors, keys)
    np.testing.assert_allclose(got_sample, sample, rtol=rtol, atol=atol, err_msg=label + " samples")
    sizes = np.array([np.asarray(tensors[k]).size for k in keys], np.float64)
    tol = rtol * stats[:, 1] + atol * sizes
    assert np.all(np.abs(got_stats[:, 0] - stats[:, 0]) <= tol), label + " sums"
    assert np.all(np.abs(got_stats[:, 1] - stats[:, 1]) <= tol), label + " abs-sums"


def gaps(name, dtype_a=F32, **sw):
    """largest |a - b| / tolerance over the compared quantities after all of the case's calls: a = float32 oracle (or a switched float64
    one), b = the float64 oracle"""
    c = case(name)
    inp = inputs(c)
    a, b = make(c, inp, dtype_a, **sw), make(c, inp, np.float64)
    gap = dict(loss=0.0, norm=0.0, param=0.0, m=0.0)
    for call in range(c["n_learn"]):
        ra, rb = a.learn_with(inp["idx"][call], inp["eps"][call], c["gamma"], c["tau"]), b.learn_with(inp["idx"][call], inp["eps"][call], c["gamma"], c["tau"])
        for key in ("critic_loss", "actor_loss"):
            x, y = np.array(ra[key], np.float64), np.array(rb[key], np.float64)
            gap["loss"] = max(gap["loss"], float(np.max(np.abs(x - y) / (TOL["loss"][1] + TOL["loss"][0] * np.abs(y)))))
        for key in ("critic_norm", "actor_norm"):
            x, y = np.array(ra[key], np.float64), np.array(rb[key], np.float64)
            gap["norm"] = max(gap["norm"], float(np.max(np.abs(x - y) / (TOL["norm"] * np.abs(y)))))
    for j in range(len(c["dims"])):
        for pa, pb in ((a.actor[j], b.actor[j]), (a.critic(j), b.critic(j)), (a.critic(j, True), b.critic(j, True))):
            for k in pb:
                d = np.abs(pa[k].astype(np.float64) - pb[k]) / (TOL["param"][1] + TOL["param"][0] * np.abs(pb[k]))
                gap["param"] = max(gap["param"], float(np.quantile(d, 0.99)))          # (_assert_net lets 1 % of a tensor's elements out)
        for ma, mb in ((a.aopt[j].m, b.aopt[j].m), (a.copt[j].m, b.copt[j].m)):
            for k in mb:
                scale = float(np.abs(mb[k]).max())
                if scale == 0.0:          # (pair: one other agent, the softmax is 1 and the key's and the query's gradients are exactly zero)
                    assert not ma[k].any()
                    continue
                gap["m"] = max(gap["m"], float(np.quantile(np.abs(ma[k].astype(np.float64) - mb[k]), 0.99) / (TOL["m"] * scale)))
    return gap


def switch_gap(name, switch):
    """how far the switched float64 oracle lands from the true one on `name`, in tolerances"""
    return max(gaps(name, np.float64, **{switch: True}).values())
