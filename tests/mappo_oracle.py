"""NumPy restatement of MAPPO_file/MAPPO.py:357-482 and IPPO.py:252-322 (`learn`) and of the nets' normalised forward
(MAPPO.py:123-218 = IPPO.py:57-153), in float32 where torch is.  Test infrastructure: the seeded cases below are what
tests/golden/make_mappo_golden.py runs the imported reference on, what tests/test_mappo_oracle.py checks this file against, and what
tests/test_gpu_mappo.py runs the kernels on.

Kept as the reference has it (DESIGN.md "MAPPO / IPPO"): MAPPO's actor loss is the mean over ratios [m, 1] x adv[index] [m, n], its
critic regresses V repeated n times on all n target columns, its adv_norm runs over the whole matrix; ValueClip clamps the TARGET and
takes the max of two mean losses (computed literally here: the step is the unclipped loss's); MAPPO's one Adam over actor + critic
(lr = actor_lr, eps 1e-5, no clip) is two Adams with those settings.
"""
import math

import numpy as np

from oracle import nn
from oracle.nn import F32, Adam
from oracle.ppo import F32_EPS, HALF_LOG_2PI, LOG_SQRT_2PI, gae

LN_EPS = 1e-5
ACTOR_C = ["l1", "l2", "mean_layer"]
ACTOR_D = ["l1", "l2", "l3"]
CRITIC = ["l1", "l2", "l3"]
DIMS = ((5, 3), (4, 2), (5, 3))          # (obs, act) per agent: unequal, so that a wrong per-agent offset shows
TRICKS_ON = dict(adv_norm=True, adam_eps=True, ValueClip=True, huber_loss=True, LayerNorm=True, feature_norm=True)
TRICKS_OFF = dict(adv_norm=False, adam_eps=False, ValueClip=False, huber_loss=False, LayerNorm=False, feature_norm=False)
HYPER = dict(gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3)


def _case(kind, cont, tricks, **kw):
    c = dict(kind=kind, cont=cont, trick=dict(TRICKS_ON if tricks else TRICKS_OFF), dims=DIMS, hidden=32, horizon=40, minibatch=16,
             k_epochs=2, huber_delta=10.0, reward_scale=1.0, reward_same=False, dead_agent=None, seed=0)
    c.update(HYPER)
    c.update(kw)
    return c


CASES = {}
for _k in ("mappo", "ippo"):
    for _c in (True, False):
        for _t in (False, True):
            CASES["%s_%s_%s" % (_k, "c" if _c else "d", "tricks" if _t else "plain")] = _case(_k, _c, _t, seed=len(CASES) + 11)
# both Huber branches: delta 0.5 against the case's rewards, scaled so that the errors straddle it (the golden maker checks >= 10 % of the first step's errors on each side)
CASES["ippo_c_huber"] = _case("ippo", True, False, trick=dict(TRICKS_OFF, huber_loss=True), huber_delta=0.5, reward_scale=0.25, reward_same=True, seed=31)
CASES["mappo_d_huber"] = _case("mappo", False, False, trick=dict(TRICKS_OFF, huber_loss=True), huber_delta=0.5, reward_scale=0.25, reward_same=True, seed=32)
# ValueClip with >= 25 % of the first step's rows clamped (checked by the maker); `_off` is the same case without the trick
CASES["mappo_c_vclip"] = _case("mappo", True, False, trick=dict(TRICKS_OFF, ValueClip=True), seed=33)
CASES["mappo_c_vclip_off"] = _case("mappo", True, False, seed=33)
CASES["ippo_c_vclip"] = _case("ippo", True, False, trick=dict(TRICKS_OFF, ValueClip=True, huber_loss=True), huber_delta=0.5, reward_scale=0.25, reward_same=True, seed=34)
# a dead hidden layer: l1.bias = -10 on one agent's actor and critic, so the LayerNorm row has zero variance
CASES["mappo_c_dead"] = _case("mappo", True, True, dead_agent=1, seed=35)
CASES["ippo_d_dead"] = _case("ippo", False, True, dead_agent=1, seed=36)
# one minibatch longer than the engine's row chunk (64 rows at these widths): 70 rows in one step
CASES["mappo_c_chunk"] = _case("mappo", True, True, horizon=70, minibatch=70, k_epochs=1, seed=37)
CASES["ippo_d_chunk"] = _case("ippo", False, False, horizon=70, minibatch=70, k_epochs=1, seed=38)
# the scripts' widths: 3 x (18, 5), hidden 128; a MAPPO critic's first layer is 54 wide
CASES["mappo_c_wide"] = _case("mappo", True, True, dims=((18, 5),) * 3, hidden=128, horizon=64, minibatch=64, k_epochs=1, seed=39)
CASES["ippo_d_wide"] = _case("ippo", False, True, dims=((18, 5),) * 3, hidden=128, horizon=64, minibatch=64, k_epochs=1, seed=40)
# one agent, no tricks: an IPPO engine against the existing PPO engine (tests/test_gpu_mappo.py)
CASES["ippo_c_single"] = _case("ippo", True, False, dims=((5, 3),), seed=41)
CASES["ippo_d_single"] = _case("ippo", False, False, dims=((5, 3),), seed=42)


# cases whose final parameters the golden holds in full (the others: digests; a committed file stays under 1 MiB)
FULL_CASES = tuple(k for k in CASES if k.endswith(("_plain", "_tricks", "_huber", "_vclip", "_dead")))


def case(name):
    return dict(CASES[name], name=name)


def actor_names(c):
    return ACTOR_C if c["cont"] else ACTOR_D


def critic_in(c, i):
    return sum(o for o, _ in c["dims"]) if c["kind"] == "mappo" else c["dims"][i][0]


def flat(c, tag, p):
    """a net's tensors as one vector, in state_dict order (what frl_params_get returns)"""
    names = actor_names(c) if tag == "actor" else CRITIC
    parts = []
    for n in names:
        parts += [np.asarray(p[n + ".weight"], F32).reshape(-1), np.asarray(p[n + ".bias"], F32).reshape(-1)]
    if tag == "actor" and c["cont"]:
        parts.append(np.asarray(p["log_std"], F32).reshape(-1))
    return np.concatenate(parts)


def digest(x, n_sample=32):
    """[sum, abs-sum, a strided sample] of a vector, float64"""
    x = np.asarray(x, np.float64).reshape(-1)
    return np.concatenate([[x.sum(), np.abs(x).sum()], x[::max(1, x.size // n_sample)][:n_sample]])


def _linear(rng, out_dim, in_dim, scale=1.0):
    b = scale / math.sqrt(in_dim)
    return rng.uniform(-b, b, (out_dim, in_dim)).astype(F32), rng.uniform(-b, b, out_dim).astype(F32)


def net_params(rng, names, dims, log_std=None):
    p = {}
    for n, (o, i) in zip(names, dims):
        p[n + ".weight"], p[n + ".bias"] = _linear(rng, o, i)
    if log_std is not None:
        p["log_std"] = log_std.astype(F32)
    return p


def inputs(c, seed=None):
    """Seeded parameters and a horizon of rows per agent (PCG64: the same on every machine)."""
    rng = np.random.Generator(np.random.PCG64(c["seed"] if seed is None else seed))
    H, T, n = c["hidden"], c["horizon"], len(c["dims"])
    actors, critics, rows = [], [], []
    for i, (O, A) in enumerate(c["dims"]):
        ls = rng.uniform(-0.7, 0.2, (1, A)) if c["cont"] else None
        actors.append(net_params(rng, actor_names(c), [(H, O), (H, H), (A, H)], ls))
        critics.append(net_params(rng, CRITIC, [(H, critic_in(c, i)), (H, H), (1, H)]))
        if c["dead_agent"] == i:
            actors[i]["l1.bias"][:] = -10
            critics[i]["l1.bias"][:] = -10
    for i, (O, A) in enumerate(c["dims"]):
        obs = rng.normal(0, 1, (T, O)).astype(F32)
        nobs = (obs + rng.normal(0, 0.3, (T, O))).astype(F32)
        if c["cont"]:
            act = rng.normal(0, 0.8, (T, A)).astype(F32)
            logp = rng.normal(-1.0, 0.3, (T, A)).astype(F32)
        else:
            act = rng.integers(0, A, (T, 1)).astype(F32)
            logp = np.log(rng.uniform(0.15, 0.6, (T, 1))).astype(F32)
        j = 0 if c["reward_same"] else i                                                             # (one distribution, different draws)
        rew = (rng.normal(0.3 * (j + 1), 1.0 + 0.5 * j, (T, 1)) * c["reward_scale"]).astype(F32)      # different rewards per agent
        done = np.zeros((T, 1), F32)
        if i == 1 or n == 1:
            done[[7, T - 9]] = 1                                                                     # `done` on two rows of one agent only
        adv_done = np.zeros((T, 1), F32)
        adv_done[9::10] = 1                                                                          # every 10th row
        rows.append(dict(obs=obs, act=act, rew=rew, next_obs=nobs, done=done, logp=logp, adv_done=adv_done))
    return dict(actors=actors, critics=critics, rows=rows)


def perms(c, seed=None):
    """[n_agents][k_epochs][horizon]: what np.random.permutation returns after np.random.seed(case seed + 1000), in learn()'s order"""
    st = np.random.RandomState((c["seed"] if seed is None else seed) + 1000)
    return np.stack([np.stack([st.permutation(c["horizon"]) for _ in range(c["k_epochs"])]) for _ in c["dims"]])


# ------------------------------------------------------------------------------------------------ nets
def layer_norm(x):
    """F.layer_norm over the row: no affine part, biased variance, eps 1e-5 -> (y, rstd)"""
    x = np.asarray(x, F32)
    mean = x.mean(axis=1, keepdims=True, dtype=F32)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True, dtype=F32)
    rstd = (F32(1) / np.sqrt(var + F32(LN_EPS))).astype(F32)
    return ((x - mean) * rstd).astype(F32), rstd


def layer_norm_bwd(dy, xhat, rstd):
    m1 = dy.mean(axis=1, keepdims=True, dtype=F32)
    m2 = (dy * xhat).mean(axis=1, keepdims=True, dtype=F32)
    return (rstd * ((dy - m1) - xhat * m2)).astype(F32)


def forward(p, names, x, trick):
    """-> (head output before any output activation, cache for backward)"""
    x = np.asarray(x, F32)
    if trick["feature_norm"]:
        x = layer_norm(x)[0]
    cache, h = [], x
    for n in names[:2]:
        a = np.maximum(h @ p[n + ".weight"].T + p[n + ".bias"], F32(0)).astype(F32)
        xh, rstd = layer_norm(a) if trick["LayerNorm"] else (a, None)
        cache.append((h, a, xh, rstd))
        h = xh
    out = (h @ p[names[2] + ".weight"].T + p[names[2] + ".bias"]).astype(F32)
    return out, (cache, h)


def backward(p, names, fwd_cache, dout):
    cache, h_last = fwd_cache
    g = {names[2] + ".weight": (dout.T @ h_last).astype(F32), names[2] + ".bias": dout.sum(axis=0).astype(F32)}
    d = (dout @ p[names[2] + ".weight"]).astype(F32)
    for n, (h_in, a, xh, rstd) in zip(reversed(names[:2]), reversed(cache)):
        if rstd is not None:
            d = layer_norm_bwd(d, xh, rstd)
        d = (d * (a > 0)).astype(F32)
        g[n + ".weight"] = (d.T @ h_in).astype(F32)
        g[n + ".bias"] = d.sum(axis=0).astype(F32)
        d = (d @ p[n + ".weight"]).astype(F32)
    return g


def value(p, x, trick):
    return forward(p, CRITIC, x, trick)[0]


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F32)


def act_forward(c, p, obs):
    """what frl_act returns before a mode's sampling: tanh mean (continuous) or the logits (discrete)"""
    z = forward(p, actor_names(c), obs, c["trick"])[0]
    return np.tanh(z).astype(F32) if c["cont"] else z


def huber_loss(e, d):
    d = F32(d)
    small = np.abs(e) <= d
    return np.where(small, e * e * F32(0.5), d * (np.abs(e) - d * F32(0.5))).astype(F32), np.where(small, e, d * np.sign(e)).astype(F32)


# ------------------------------------------------------------------------------------------------ learn
class Oracle:
    def __init__(self, c, inp):
        self.c, self.trick, self.n = c, c["trick"], len(c["dims"])
        self.actors = [nn.copy_params(p) for p in inp["actors"]]
        self.critics = [nn.copy_params(p) for p in inp["critics"]]
        self.rows = inp["rows"]
        if c["kind"] == "mappo":           # one Adam over both lists: lr = actor_lr, eps 1e-5, whatever trick['adam_eps'] says (MAPPO.py:229-230)
            eps, clr, self.clip_norm = 1e-5, c["actor_lr"], 0.0
        else:
            eps, clr, self.clip_norm = (1e-5 if self.trick["adam_eps"] else 1e-8), c["critic_lr"], 0.5
        self.adam_eps, self.critic_lr = eps, clr
        self.aopt = [Adam(p, c["actor_lr"], eps=eps) for p in self.actors]
        self.copt = [Adam(p, clr, eps=eps) for p in self.critics]
        self.first = {}                    # diagnostics of every agent's first critic step (the golden maker's conditions)

    def critic_obs(self, i, key="obs", ix=slice(None)):
        if self.c["kind"] == "mappo":
            return np.concatenate([r[key][ix] for r in self.rows], axis=1)
        return self.rows[i][key][ix]

    def gae(self):
        c, T, n = self.c, self.c["horizon"], self.n
        adv, vs_all = np.zeros((T, n), F32), np.zeros((T, n), F32)
        for i, r in enumerate(self.rows):
            vs = value(self.critics[i], self.critic_obs(i), self.trick)
            vs_ = value(self.critics[i], self.critic_obs(i, "next_obs"), self.trick)
            td = r["rew"] + F32(c["gamma"]) * (F32(1) - r["done"]) * vs_ - vs
            adv[:, i] = gae(td.reshape(-1), r["adv_done"].reshape(-1), c["gamma"], c["lmbda"])
            vs_all[:, i] = vs.reshape(-1)
        v_target = (adv + vs_all).astype(F32)
        self.adv_raw, self.v_target = adv.copy(), v_target
        if self.trick["adv_norm"]:
            def norm(a):
                mean = a.mean(dtype=F32)
                std = np.sqrt(np.sum((a - mean) ** 2, dtype=F32) / F32(a.size - 1))
                return ((a - mean) / (std + F32(1e-8))).astype(F32)
            adv = norm(adv) if c["kind"] == "mappo" else np.stack([norm(adv[:, i]) for i in range(n)], axis=1)
        self.adv = adv

    def learn(self, perm):
        """perm [n][K][T] -> trace [n][K * n_mb][2]"""
        c, T, mb = self.c, self.c["horizon"], self.c["minibatch"]
        self.gae()
        trace = []
        for i in range(self.n):
            cols = slice(None) if c["kind"] == "mappo" else slice(i, i + 1)
            tr = []
            for k in range(c["k_epochs"]):
                for s in range(0, T, mb):
                    ix = np.asarray(perm[i][k][s:s + mb])
                    tr.append((self.actor_step(i, ix, self.adv[ix][:, cols]), self.critic_step(i, ix, self.v_target[ix][:, cols])))
            trace.append(tr)
        return np.array(trace, F32)

    def actor_step(self, i, ix, A):
        c, r, p = self.c, self.rows[i], self.actors[i]
        names = actor_names(c)
        m, ent_coef, clip = len(ix), c["ent_coef"], c["clip"]
        z, cache = forward(p, names, r["obs"][ix], self.trick)
        if c["cont"]:
            mean = np.tanh(z).astype(F32)
            raw = p["log_std"]
            log_std = np.clip(np.broadcast_to(raw, mean.shape), -20, 2).astype(F32)
            var = np.exp(log_std) ** 2
            a = r["act"][ix]
            lp = (-((a - mean) ** 2) / (F32(2) * var) - log_std - F32(LOG_SQRT_2PI)).sum(axis=1, keepdims=True)
            ent = (F32(0.5 + HALF_LOG_2PI) + log_std).sum(axis=1, keepdims=True)
        else:
            pr = softmax(z)
            logit = np.log(np.clip(pr / pr.sum(axis=1, keepdims=True, dtype=F32), F32_EPS, 1 - F32_EPS)).astype(F32)
            a = r["act"][ix].astype(np.int64).reshape(-1)
            lp = logit[np.arange(m), a].reshape(-1, 1)
            ent = -(logit * pr).sum(axis=1, keepdims=True)
        ratio = np.exp(lp - r["logp"][ix].sum(axis=1, keepdims=True)).astype(F32)
        surr1 = ratio * A
        surr2 = np.clip(ratio, 1 - clip, 1 + clip).astype(F32) * A
        loss = F32(-np.mean(np.minimum(surr1, surr2), dtype=F32) - F32(ent_coef) * np.mean(ent, dtype=F32))
        dlp = (np.where(surr1 <= surr2, A, F32(0)).sum(axis=1, keepdims=True) * F32(-1.0 / A.size) * ratio).astype(F32)
        if c["cont"]:
            dz = (dlp * (a - mean) / var * (F32(1) - mean * mean)).astype(F32)
            g = backward(p, names, cache, dz)
            inside = ((raw >= -20) & (raw <= 2)).astype(F32)
            g["log_std"] = ((dlp * ((a - mean) ** 2 / var - F32(1)) - F32(ent_coef / m)).sum(axis=0, keepdims=True) * inside).astype(F32)
        else:
            onehot = np.zeros_like(pr)
            onehot[np.arange(m), a] = 1
            g = backward(p, names, cache, (dlp * (onehot - pr) + F32(ent_coef / m) * pr * (logit + ent)).astype(F32))
        g = {k: g[k] for k in p}
        if self.clip_norm > 0:
            nn.clip_grad_norm(g, self.clip_norm)
        self.aopt[i].step(p, g)
        return loss

    def critic_step(self, i, ix, Y):
        c, p = self.c, self.critics[i]
        v, cache = forward(p, CRITIC, self.critic_obs(i, "obs", ix), self.trick)
        V = np.repeat(v, Y.shape[1], axis=1)

        def loss_of(y):
            e = (y - V).astype(F32)
            if self.trick["huber_loss"]:
                per, de = huber_loss(e, c["huber_delta"])
            else:
                per, de = e * e, F32(2) * e
            return F32(np.mean(per, dtype=F32)), de
        loss, de = loss_of(Y)
        if ("critic", i) not in self.first:
            e = np.abs(Y - V)
            self.first[("critic", i)] = dict(frac_small=float((e <= c["huber_delta"]).mean()), frac_clamped=float((e > c["clip"]).mean()))
        if self.trick["ValueClip"]:
            # literally (MAPPO.py:422-431, IPPO.py:302-311): the clamped loss never exceeds the original, and where no row is clamped the
            # two have equal gradients, so torch.max steps like, and reports, the original
            loss_clip, _ = loss_of(np.clip(Y, V - F32(c["clip"]), V + F32(c["clip"])).astype(F32))
            assert loss_clip <= loss
            loss = max(loss, loss_clip)
        dv = (-de.sum(axis=1, keepdims=True) * F32(1.0 / Y.size)).astype(F32)
        g = backward(p, CRITIC, cache, dv)
        g = {k: g[k] for k in p}
        if self.clip_norm > 0:
            nn.clip_grad_norm(g, self.clip_norm)
        self.copt[i].step(p, g)
        return loss


def run(c, inp=None, perm=None):
    inp = inputs(c) if inp is None else inp
    o = Oracle(c, inp)
    o.trace = o.learn(perms(c) if perm is None else perm)
    return o


# ------------------------------------------------------------------------------------------------ comparisons
# Parameter tolerances: tests/test_gpu_envelope.py's rules, unchanged (quoted in tests/test_gpu_envelope_ddpg.py:68-71): >= 99 % of a
# net's elements within (rtol 5e-4, atol 5e-6), none further than Adam can move an element in `steps` steps (2 lr steps); the first
# moment within 2e-3 of its largest on >= 99 % of a net, within 5e-2 everywhere (2e-2 for nets under 2048 elements).
def assert_net(got, want, lr, steps, label, rtol=5e-4, atol=5e-6):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert np.isfinite(got).all(), label + ": not finite"
    d = np.abs(got - want)
    bad = d > atol + rtol * np.abs(want)
    assert bad.mean() <= 0.01, "%s: %d of %d elements outside (max |diff| %.3g)" % (label, bad.sum(), bad.size, d.max())
    assert d.max() <= 2 * lr * steps, "%s: max |diff| %.3g" % (label, d.max())


def assert_m(got, want, label):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    scale = float(np.abs(want).max())
    d = np.abs(got - want)
    if d.size < 2048:
        assert d.max() <= 2e-2 * scale, "adam m %s: %.3g of max |m| %.3g" % (label, d.max(), scale)
        return
    assert np.quantile(d, 0.99) <= 2e-3 * scale, "adam m %s: 99th percentile" % label
    assert d.max() <= 5e-2 * scale, "adam m %s: max %.3g of %.3g" % (label, d.max(), scale)


def assert_digest(got_flat, want_digest, label, rtol=5e-4, atol=5e-6):
    """a vector against a digest of the reference's: the sample by the element rule's bounds, the sums within them summed"""
    d = digest(got_flat)
    np.testing.assert_allclose(d[2:], want_digest[2:], rtol=20 * rtol, atol=20 * atol, err_msg=label + " sample")
    tol = rtol * want_digest[1] + atol * np.asarray(got_flat).size
    assert abs(d[0] - want_digest[0]) <= tol and abs(d[1] - want_digest[1]) <= tol, "%s sums %r vs %r" % (label, d[:2], want_digest[:2])
