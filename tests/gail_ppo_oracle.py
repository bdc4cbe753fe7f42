"""GAIL's policy side (GAIL_file/PPO2.py:20-307, `PPO.PPO_learn`) restated in NumPy float64, and the seeded inputs of its cases.
tests/golden/make_gail_ppo_golden.py runs the reference on exactly these inputs; tests/test_gail_ppo_oracle.py holds this oracle to
its output and tests/test_gpu_gail_ppo.py holds the HIP engine to both.

Nets: actor s -> H -> H -> a, critic s -> H -> H -> 1, hidden activation LeakyReLU(0.01) or ReLU.  Continuous: mean = tanh(head),
std = exp(clamp(log_std, lo, hi)), Normal; discrete: Categorical(logits = head).  One PPO_learn:
    V and the OLD log-prob (summed over dimensions) over the whole horizon with the pre-update nets;
    td_t = r_t + gamma V_{t+1} - V_t with V_{t+1} the next row's value also behind a `done` row (mask_1 == 1) and last_value behind the
    last row;  A_t = td_t + c (1 - done_t) A_{t+1};  returns = A + V;  A <- (A - mean) / (unbiased std + 1e-8);
    K x ceil(T / mb) steps on torch.randperm minibatches: actor loss -mean(min(ratio A, clip(ratio) A)) - ent_weight mean(entropy),
    critic loss value_loss_coef mse(V, returns); clip_grad_norm_(., 0.5) on each net alone; ONE Adam (two lrs, one step count).
gamma and c enter as the float32 values torch multiplies float32 tensors with: float32(gamma), float32(gamma * lam).

What the conditioning rules of tests/ppo_edge_cases.py need is logged per step: the ratios, which rows sit on the clamped branch, the raw
log_std, and the smallest |pre-activation| of any hidden unit of either net.
"""
import functools
import math

import numpy as np

from tests.golden import synth

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
SLOPES = {"LeakyReLU": 0.01, "ReLU": 0.0}
NAMES = ["backbone.0", "backbone.1", "backbone.2"]
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
# what every case shares (PPO2's shipped values but the learning rates: 3e-3 / 1e-3 move the ratios off 1 within a few steps, and tell the
# two param groups apart)
HYPER = dict(gamma=0.99, lam=0.95, clip=0.2, ent_weight=0.01, value_loss_coef=0.5, p_lr=3e-3, v_lr=1e-3, clip_norm=0.5)
PARAM_RTOL, PARAM_ATOL = 2e-3, 2e-5      # tests/test_gpu_ppo_edges.py: PARAM_TOL
TWIN_SPREAD = 0.25
KINK = 1e-6
N_PROBE = 16


def case(name, s, a, H, T, mb, K, seed, act="LeakyReLU", discrete=False, calls=1, log_std=None, rng=(-10.0, 2.0), last_value=0.0, done=None, head_scale=1.0):
    """log_std: raw values set over the zeros of the reference's init; done: rows with done = 1 (None: about one row in eleven);
    head_scale: multiplies the actor's head layer (see the clamp case)."""
    return dict(head_scale=head_scale, name=name, s=s, a=a, H=H, T=T, mb=mb, K=K, seed=seed, act=act, discrete=discrete, calls=calls, log_std=log_std, rng=rng,
                last_value=last_value, done=done)


CASES = [
    case("leaky-3-1", 3, 1, 32, 40, 16, 2, 0, calls=2, last_value=0.7, done=(17, 39)),      # the script's dims; tail minibatch 8
    case("relu-17-6", 17, 6, 64, 70, 24, 2, 1, act="ReLU", last_value=-0.3),                   # two first-layer k-blocks, 6-column head, tail 22
    case("leaky-8-17", 8, 17, 128, 33, 33, 1, 2, last_value=0.2),                              # head past one tile, one minibatch = horizon
    case("cat-4-2", 4, 2, 32, 33, 7, 2, 3, discrete=True, last_value=0.4),                     # Categorical logits; tail 5
    case("cat-4-5", 4, 5, 32, 33, 7, 2, 4, discrete=True, last_value=0.4),
    # raw log_std ON both bounds (the closed range passes the gradient) and PAST them (gated: bit-unchanged, Adam moments 0)
    # A std of e^-10 = 4.5e-5 makes d logp / d mean = (a - mean) / var as large as 2e4 per unit of eps: a float32 forward of a mean of order 1
    # (rounding 6e-8) would carry a relative error of 1e-3 into every row's gradient, and no seed conditions that.  The head layer is scaled
    # by 1e-3, so that means and stored actions are of order 1e-3 and their float32 roundings of order 1e-10.
    case("clamp", 8, 4, 32, 40, 16, 2, 5, log_std=(2.0, 2.5, -10.0, -10.5), head_scale=1e-3),
    # one net under two ranges with raw log_std -7 and 1: inside [-10, 2], clamped to (-5, 0.5) by [-5, 0.5]
    case("range-wide", 8, 2, 32, 40, 16, 1, 6, log_std=(-7.0, 1.0), rng=(-10.0, 2.0)),
    case("range-narrow", 8, 2, 32, 40, 16, 1, 6, log_std=(-7.0, 1.0), rng=(-5.0, 0.5)),
    case("t2", 3, 1, 32, 2, 2, 1, 7, last_value=0.5, done=()),                                 # the smallest horizon
]
POPULATION = [case("pop%d" % p, 3, 1, 32, 40, 16, 2, sd, last_value=lv) for p, (sd, lv) in enumerate(((8, 0.1), (9, -0.6), (10, 0.9)))]
BY_NAME = {c["name"]: c for c in CASES + POPULATION}
# raw log_std values a case puts ON or PAST a bound on purpose (the 1e-3 rule of assert_conditions exempts exactly these)
ON_PURPOSE = {"clamp": (0, 1, 2, 3), "range-narrow": (0, 1)}


def n_mb(c):
    return (c["T"] + c["mb"] - 1) // c["mb"]


def n_steps(c):
    return c["K"] * n_mb(c)


def layers(c, out):
    return [(NAMES[0], c["H"], c["s"]), (NAMES[1], c["H"], c["H"]), (NAMES[2], out, c["H"])]


def config(c):
    """The reference's config dict (GAIL_file/config.py) for a case."""
    return dict(seed=c["seed"], use_gpu=False, s_dim=c["s"], a_dim=c["a"], discrete=c["discrete"], algo="PPO", log_dir="logs", id="case",
                env_reproducible=True, collect_eval_data=False,
                PPO=dict(policy_mlp_dim=c["H"], activation=c["act"], dropout=0.0, layernorm=False, log_std_min=c["rng"][0], log_std_max=c["rng"][1],
                         p_lr=HYPER["p_lr"], v_lr=HYPER["v_lr"], horizon=c["T"], gamma=HYPER["gamma"], lam=HYPER["lam"], clip_epsilon=HYPER["clip"],
                         K_epochs=c["K"], value_loss_coef=HYPER["value_loss_coef"], ent_weight=HYPER["ent_weight"], mini_batch_size=c["mb"],
                         eval_interval=10, eval_episodes=1))


# the loop case: one GAIL.train on the in-repo PendulumShort-v1 (40-step episodes) — 2 episodes at horizon 64 are ONE iteration of
# trian_D + compute_reward + PPO_learn with an episode end at row 39, then 16 more steps under the updated policy
TRAIN = dict(seed=7, s_dim=3, a_dim=1, hidden=32, horizon=64, mb=16, K=2, episodes=2, n_expert=200, env="PendulumShort-v1")


def train_config(log_dir="logs"):
    t = TRAIN
    return dict(id=t["env"], log_dir=log_dir, algo="GAIL", seed=t["seed"], env_reproducible=True, collect_eval_data=False, num_workers=0, use_gpu=False,
                s_dim=t["s_dim"], a_dim=t["a_dim"], discrete=False,
                PPO=dict(policy_mlp_dim=t["hidden"], activation="LeakyReLU", dropout=0.0, layernorm=False, log_std_min=-10, log_std_max=2, p_lr=1e-4, v_lr=3e-4,
                         horizon=t["horizon"], gamma=0.99, lam=0.95, clip_epsilon=0.2, K_epochs=t["K"], value_loss_coef=1, ent_weight=0.01,
                         mini_batch_size=t["mb"], eval_interval=10, eval_episodes=1),
                D=dict(d_mlp_dim=t["hidden"], activation="LeakyReLU", dropout=0.0, layernorm=False, d_lr=4e-4, gp_coef=10.0))


def train_expert():
    """The seeded synthetic expert set: 200 unscaled (state, action) rows, every column with its own offset and range."""
    g = np.random.default_rng(69000 + TRAIN["seed"])
    n = TRAIN["n_expert"]
    return (g.standard_normal((n, 3)) * np.array([0.7, 0.7, 3.0]) + np.array([0.1, -0.2, 0.5])), g.uniform(-2.0, 2.0, (n, 1))


# ------------------------------------------------------------------------------------------------ the nets
def act_f(x, slope):
    return np.where(x > 0, x, slope * x)


def mlp_forward(p, x, slope):
    """-> (head, cache); cache keeps what the backward and the kink rule need."""
    z1 = x @ p[NAMES[0] + ".weight"].T + p[NAMES[0] + ".bias"]
    h1 = act_f(z1, slope)
    z2 = h1 @ p[NAMES[1] + ".weight"].T + p[NAMES[1] + ".bias"]
    h2 = act_f(z2, slope)
    return h2 @ p[NAMES[2] + ".weight"].T + p[NAMES[2] + ".bias"], (x, z1, h1, z2, h2)


def mlp_backward(p, cache, dz, slope):
    x, z1, h1, z2, h2 = cache
    g = {NAMES[2] + ".weight": dz.T @ h2, NAMES[2] + ".bias": dz.sum(0)}
    d2 = (dz @ p[NAMES[2] + ".weight"]) * np.where(z2 > 0, 1.0, slope)
    g[NAMES[1] + ".weight"], g[NAMES[1] + ".bias"] = d2.T @ h1, d2.sum(0)
    d1 = (d2 @ p[NAMES[1] + ".weight"]) * np.where(z1 > 0, 1.0, slope)
    g[NAMES[0] + ".weight"], g[NAMES[0] + ".bias"] = d1.T @ x, d1.sum(0)
    return g


def log_softmax(z):
    z = z - z.max(axis=1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


class Oracle:
    def __init__(self, c, params, dtype=np.float64):
        self.c, self.dt = c, dtype
        self.slope = SLOPES[c["act"]]
        self.actor = {k: np.array(v, dtype) for k, v in params["actor"].items()}
        self.critic = {k: np.array(v, dtype) for k, v in params["critic"].items()}
        self.m = {n: {k: np.zeros_like(v) for k, v in net.items()} for n, net in (("actor", self.actor), ("critic", self.critic))}
        self.v = {n: {k: np.zeros_like(v) for k, v in net.items()} for n, net in (("actor", self.actor), ("critic", self.critic))}
        self.step = 0
        self.ratio_log, self.preact_log, self.actor_losses, self.critic_losses = [], [], [], []

    # ---- forward pieces (PolicyModel.pi / value)
    def log_std(self):
        return np.clip(self.actor["log_std"], self.c["rng"][0], self.c["rng"][1])

    def head(self, s):
        return mlp_forward(self.actor, np.asarray(s, self.dt), self.slope)

    def pi_mean(self, s):
        z = self.head(s)[0]
        return np.argmax(z, axis=1) if self.c["discrete"] else np.tanh(z)

    def value(self, s):
        return mlp_forward(self.critic, np.asarray(s, self.dt), self.slope)[0][:, 0]

    def logp(self, s, a):
        z = self.head(s)[0]
        if self.c["discrete"]:
            return np.take_along_axis(log_softmax(z), np.asarray(a).reshape(-1, 1).astype(np.int64), axis=1)[:, 0]
        ls = self.log_std()
        return (-(np.asarray(a, self.dt) - np.tanh(z)) ** 2 / (2 * np.exp(2 * ls)) - ls - HALF_LOG_2PI).sum(axis=1)

    # ---- PPO.GAE with masks_1 == 1; bootstrap_done=True: the OTHER recurrence, r + gamma (1 - done) V' - V (what PPO_file does)
    def gae(self, rewards, values, done, last_value, bootstrap_done=False):
        g, cc = float(F32(HYPER["gamma"])), float(F32(HYPER["gamma"] * HYPER["lam"]))
        T = len(rewards)
        nxt = np.append(values[1:], last_value)
        adv, last = np.zeros(T, self.dt), 0.0
        for t in reversed(range(T)):
            boot = nxt[t] * ((1.0 - done[t]) if bootstrap_done else 1.0)
            last = rewards[t] + g * boot - values[t] + cc * (1.0 - done[t]) * last
            adv[t] = last
        return adv, adv + values, (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)

    def _adam(self, name, net, grads, lr):
        total = math.sqrt(sum(float((g * g).sum()) for g in grads.values()))
        coef = min(1.0, HYPER["clip_norm"] / (total + 1e-6))
        b1, b2, t = 0.9, 0.999, self.step
        for k in net:
            g = grads[k].reshape(net[k].shape) * coef
            self.m[name][k] = b1 * self.m[name][k] + (1 - b1) * g
            self.v[name][k] = b2 * self.v[name][k] + (1 - b2) * g * g
            net[k] = net[k] - (lr / (1 - b1 ** t)) * self.m[name][k] / (np.sqrt(self.v[name][k]) / math.sqrt(1 - b2 ** t) + 1e-8)

    def learn(self, table, perms, last_value, rewards=None, bootstrap_done=False):
        """One PPO_learn.  table: states [T, s], actions [T, a] ([T, 1] indices when discrete), rewards [T], done [T]; perms [K, T]."""
        c, dt = self.c, self.dt
        S, A = np.asarray(table["states"], dt), np.asarray(table["actions"], dt)
        rew = np.asarray(table["rewards"] if rewards is None else rewards, dt)
        done = np.asarray(table["done"], dt)
        T, mb = c["T"], c["mb"]
        vs, lp_old = self.value(S), self.logp(S, A)
        adv_raw, returns, adv = self.gae(rew, vs, done, float(last_value), bootstrap_done)
        lo, hi = c["rng"]
        for k in range(c["K"]):
            for s0 in range(0, T, mb):
                idx = np.asarray(perms[k][s0:s0 + mb], np.int64)
                m = len(idx)
                x, a, Ar = S[idx], A[idx], adv[idx]
                z, cache = mlp_forward(self.actor, x, self.slope)
                if c["discrete"]:
                    lg = log_softmax(z)
                    pr = np.exp(lg)
                    ai = a.reshape(-1).astype(np.int64)
                    lp = lg[np.arange(m), ai]
                    ent = -(pr * lg).sum(axis=1)
                    ent_mean, raw = ent.mean(), None
                else:
                    raw = self.actor["log_std"].reshape(-1).copy()
                    ls = np.clip(raw, lo, hi)
                    mean, var = np.tanh(z), np.exp(2 * ls)
                    lp = (-(a - mean) ** 2 / (2 * var) - ls - HALF_LOG_2PI).sum(axis=1)
                    ent_mean = (0.5 + HALF_LOG_2PI + ls).sum()
                ratio = np.exp(lp - lp_old[idx])
                s1, s2 = ratio * Ar, np.clip(ratio, 1 - HYPER["clip"], 1 + HYPER["clip"]) * Ar
                self.actor_losses.append(float(-np.minimum(s1, s2).mean() - HYPER["ent_weight"] * ent_mean))
                open_ = s1 <= s2                                   # (a tie splits torch.min's gradient between two equal branches: the same sum)
                coef = np.where(open_, Ar, 0.0) * (-1.0 / m) * ratio
                if c["discrete"]:
                    onehot = np.zeros_like(pr)
                    onehot[np.arange(m), ai] = 1.0
                    dz = coef[:, None] * (onehot - pr) + (HYPER["ent_weight"] / m) * pr * (lg + ent[:, None])
                    ga = mlp_backward(self.actor, cache, dz, self.slope)
                else:
                    dm = a - mean
                    dz = coef[:, None] * dm / var * (1 - mean * mean)
                    ga = mlp_backward(self.actor, cache, dz, self.slope)
                    gls = (coef[:, None] * (dm * dm / var - 1.0)).sum(axis=0) - HYPER["ent_weight"]
                    ga["log_std"] = np.where((raw >= lo) & (raw <= hi), gls, 0.0)      # torch.clamp: the closed range passes
                v, vcache = mlp_forward(self.critic, x, self.slope)
                diff = v[:, 0] - returns[idx]
                self.critic_losses.append(float(HYPER["value_loss_coef"] * (diff * diff).mean()))
                gc = mlp_backward(self.critic, vcache, (HYPER["value_loss_coef"] * 2.0 * diff / m)[:, None], self.slope)
                self.ratio_log.append((ratio, ~open_, raw))
                self.preact_log.append(min(float(np.abs(t).min()) for t in (cache[1], cache[3], vcache[1], vcache[3])))
                self.step += 1
                self._adam("actor", self.actor, ga, HYPER["p_lr"])
                self._adam("critic", self.critic, gc, HYPER["v_lr"])
        return dict(adv=adv_raw, adv_norm=adv, returns=returns, logp_old=lp_old, vs=vs)


# ------------------------------------------------------------------------------------------------ inputs
def _inputs(name):
    c = BY_NAME[name]
    s = 61000 + 100 * c["seed"]
    T = c["T"]
    params = dict(actor=synth.mlp_params(s, layers(c, c["a"])), critic=synth.mlp_params(s + 1, layers(c, 1)))
    g = np.random.default_rng(s + 2)
    for k in (NAMES[2] + ".weight", NAMES[2] + ".bias"):
        params["actor"][k] = (params["actor"][k] * F32(c["head_scale"])).astype(F32)
    if not c["discrete"]:
        ls = np.zeros((1, c["a"]), F32)
        if c["log_std"] is not None:
            ls[0, :] = c["log_std"]
        params["actor"]["log_std"] = ls
    states = g.uniform(-1, 1, (T, c["s"])).astype(F32)
    orc = Oracle(c, params)
    z = orc.head(states)[0]
    if c["discrete"]:            # Categorical(logits).sample() by inversion on PCG64 uniforms
        cdf = np.cumsum(np.exp(log_softmax(z)), axis=1)
        actions = np.minimum((g.random((T, 1)) > cdf).sum(axis=1), c["a"] - 1).reshape(T, 1).astype(F32)
    else:                        # pi(s): mean + std eps under the case's range
        actions = (np.tanh(z) + np.exp(orc.log_std()) * g.standard_normal((T, c["a"]))).astype(F32)
    rewards = g.standard_normal(T).astype(F32)
    done = np.zeros(T, F32)
    if c["done"] is None:
        done[g.random(T) < 1 / 11] = 1.0
    else:
        done[list(c["done"])] = 1.0
    perms = [np.stack([synth.permutation(s + 10 + 10 * call + k, T) for k in range(c["K"])]) for call in range(c["calls"])]
    probe = g.uniform(-1, 1, (N_PROBE, c["s"])).astype(F32)
    return dict(params=params, table=dict(states=states, actions=actions, rewards=rewards, done=done), perms=perms, probe=probe)


_cached_inputs = functools.lru_cache(maxsize=None)(_inputs)


def inputs(c):
    """dict(params, table, perms [calls][K, T], probe).  Cached: do not write into it."""
    return _cached_inputs(c["name"])


def run(c, params=None, perms=None, rewards=None, bootstrap_done=False):
    """The case's `calls` PPO_learn calls on its table -> the oracle (nets, moments, logs) and every call's GAE outputs."""
    inp = inputs(c)
    orc = Oracle(c, params or inp["params"])
    outs = [orc.learn(inp["table"], (perms or inp["perms"])[call], c["last_value"], rewards=rewards, bootstrap_done=bootstrap_done)
            for call in range(c["calls"])]
    return orc, outs


def _twin_spread(c, orc):
    """The oracle's own conditioning (tests/ppo_edge_cases.py): the largest change of any final parameter, in units of the parameter
    tolerance, when the initial parameters move by one float32 rounding (three draws); here the per-step losses are held to the same rule."""
    worst = 0.0
    for draw in range(3):
        r = np.random.default_rng(68000 + 10 * c["seed"] + draw)
        moved = {n: {k: (v * (1 + EPS32 * r.standard_normal(v.shape))).astype(F32) for k, v in inputs(c)["params"][n].items()} for n in ("actor", "critic")}
        if c["log_std"] is not None:      # (a raw log_std put ON a bound stays there: one rounding up would close torch.clamp's gate)
            moved["actor"]["log_std"] = inputs(c)["params"]["actor"]["log_std"]
        twin = run(c, moved)[0]
        for ref, got in ((orc.actor, twin.actor), (orc.critic, twin.critic)):
            worst = max([worst] + [float((np.abs(got[k] - ref[k]) / (PARAM_ATOL + PARAM_RTOL * np.abs(ref[k]))).max()) for k in ref])
        # ... and the loss traces likewise, in units of their tolerances (ACTOR_TOL / CRITIC_TOL of tests/test_gpu_ppo_edges.py)
        al, tl = np.array(orc.actor_losses), np.array(twin.actor_losses)
        cl, tc = np.array(orc.critic_losses), np.array(twin.critic_losses)
        worst = max(worst, float((np.abs(tl - al) / (5e-6 + 2e-4 * np.abs(al))).max()), float((np.abs(tc - cl) / (2e-4 * np.abs(cl))).max()))
    return worst


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    c = BY_NAME[name]
    orc, outs = run(c)
    return dict(orc=orc, outs=outs, twin_spread=_twin_spread(c, orc), actor_losses=np.array(orc.actor_losses), critic_losses=np.array(orc.critic_losses))


def oracle_run(c):
    return _oracle_run(c["name"])


def assert_conditions(c):
    """The conditioning rules of tests/ppo_edge_cases.py on this oracle's numbers alone."""
    r, name = oracle_run(c), c["name"]
    orc = r["orc"]
    assert len(orc.ratio_log) == c["calls"] * n_steps(c) == len(r["actor_losses"]) == len(r["critic_losses"]), name
    assert np.isfinite(r["actor_losses"]).all() and np.isfinite(r["critic_losses"]).all(), name
    lo, hi = c["rng"]
    free = [j for j in range(c["a"]) if j not in ON_PURPOSE.get(name, ())]
    for i, (ratio, clamped, raw) in enumerate(orc.ratio_log):
        edge = np.minimum(np.abs(ratio - (1 - HYPER["clip"])), np.abs(ratio - (1 + HYPER["clip"]))).min()
        assert edge > 1e-4, "%s step %d: a ratio within %.1e of a clip edge: choose another seed" % (name, i, edge)
        if c["log_std"] is None:      # (a case that sets log_std near -10 has std e^-10: its ratios underflow to 0 after the first step, by design)
            assert 0.1 <= ratio.min() and ratio.max() <= 10, "%s step %d: ratios in [%g, %g]" % (name, i, ratio.min(), ratio.max())
        if raw is not None and free:
            assert np.minimum(np.abs(raw[free] - lo), np.abs(raw[free] - hi)).min() > 1e-3, "%s step %d: log_std at its clamp" % (name, i)
    assert min(orc.preact_log) > KINK, "%s: a hidden pre-activation at %.1e: choose another seed" % (name, min(orc.preact_log))
    assert r["twin_spread"] < TWIN_SPREAD, "%s: an element moves by %.2f of the tolerance under a rounding of the parameters" % (name, r["twin_spread"])
