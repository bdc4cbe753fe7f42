"""Inputs and references shared by tests/test_ppo_edge_cases.py (CPU) and tests/test_gpu_ppo_edges.py (GPU): the PPO update
(kernels_ppo2.hip on chip, kernels_ppo.hip streaming) and the GAE scans at their minibatch, horizon and head-width edges.

Inputs start from tests/golden/cases.py's builders.  For the Gaussian and Categorical cases the stored actions and log-probs
are the oracle's own at the initial parameters (oracle.ppo.PPO.select_action / select_action_discrete) plus a perturbation
of the log-probs, N(0, (0.3 / sqrt(A))^2) per dimension (one draw of sd 0.3 for a discrete action): the log-ratio of a row
then has sd 0.3 whatever the head's width, every row carries gradient, and with clip 0.2 about a quarter of the rows sit
on the clamped side of the `min`.  The Beta case keeps ppo_beta_inputs' table as it is.

Three steps of the update are discontinuous: the clamp of the ratio at 1 -+ clip (where surr1 == surr2 the gradient jumps),
the clamp of log_std at -20 and 2, and ReLU's kink: a hidden unit whose pre-activation is 0 to rounding on one row is live
in one implementation and dead in the other, and with it that row's share of a whole row of the next layer's gradient
(seen once: 3.7e-9 at unit 93 of the actor's second layer moved nine elements of l2.weight by up to lr / 10, on both
kernels alike).  `assert_conditions` checks on the oracle's numbers alone that every row of every minibatch of every step
keeps its ratio further than 1e-4 from either edge and inside [0.1, 10], that the first minibatch has 10 % .. 50 % of its
rows on the clamped branch, that every raw log_std stays further than 1e-3 from -20 and 2, and that every pre-activation
of a ReLU layer in every actor and critic step is further than 1e-6 from 0 (the two implementations' pre-activations
differ by a few float32 eps of values of order 1).  A unit that is live by a hair on the only row that feeds an element
is the same trouble one size down: its activation, and so that element's whole gradient history, carries a large
RELATIVE rounding error, and Adam's step does not depend on the gradient's size (seen once: one element of the critic's
l2.weight 1.2 tolerances off the oracle).  No threshold on pre-activations catches that at a usable rate, so the last
condition asks the oracle itself: rerun from parameters moved by one float32 rounding (three draws), no final parameter
may move by more than a quarter of the parameter tolerance (`_twin_spread`; that element moved by 0.9 and 1.2 tolerances,
the cases below move by 0.001 .. 0.16).  The seeds below were chosen so that all of this holds, and no row or
element is left out of any comparison.

GAE references: the float64 sequential recurrence A_t = d_t + c (1 - adv_done_t) A_{t+1} and the same on |d_t| (S_t, the
scale of the error bound), BufferForPPO2.compute_returns_and_advantage's formula in float64, and a NumPy float32 emulation
of gae_scan's order of operations (per-thread fold, six shuffle levels, four wave totals, replay) that shows on the CPU
that a correct scan meets the bound  |A - A_f64| <= 3 (2 L + 12) eps32 S_t,  L = ceil(T / 256): the longest dependency chain
is L folds + 6 shuffle levels + 4 wave totals + L replays, every one an affine composition of at most three roundings (the
multiply by c (1 - adv_done), the multiply and the add; fewer where the compiler contracts them), and every intermediate
is bounded by the recurrence on |d|.  c is the float32 product of the float32 gamma and lambda, as the kernel receives it."""
import functools
import math

import numpy as np

from tests.golden import cases as gcases

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
GAMMA, LMBDA, CLIP, ENT, LR = 0.99, 0.95, 0.2, 0.01, 1e-3
# The GAE tests take td from the ORACLE's value forward; the kernel's differs from it by the rounding of a 3-layer forward,
# measured at up to 2.8 eps32 (|r| + gamma |V(s')| + |V(s)|) on an MI355X, whatever |td| is.  Where adv_done cuts every step
# S_t = |td_t|, so the bound allows 3 (2 L + 12) eps32 |td_t| >= 42 eps32 |td_t|: it can be met only where |td| is no tiny
# remainder of that sum.  The tables keep |td_t| >= TD_FLOOR of it on every row (rewards of rows below twice the floor are
# moved by +-1), which leaves the value forward 42 * 0.25 = 10.5 eps32 of the sum; asserted from the oracle alone.
TD_FLOOR = 0.25
PARAM_RTOL, PARAM_ATOL = 2e-3, 2e-5    # test_ppo_learn's parameter tolerance
TWIN_SPREAD = 0.25                     # see _twin_spread
KINK = 1e-6                            # a hidden pre-activation this close to 0 may fall on either side of ReLU's kink
KWG, WAVE = 256, 64                    # gae_scan's workgroup and wave


def case(name, kind, O, A, T, mb, K, seed, tanh=False, adam_eps=False, adv_norm=False, logits=False, hidden=128, c_adamw=False, log_std=None):
    """log_std: (column, raw value) pairs set over the golden builder's interior draw, before the stored actions are drawn."""
    return dict(name=name, kind=kind, O=O, A=A, T=T, mb=mb, K=K, seed=seed, tanh=tanh, adam_eps=adam_eps, adv_norm=adv_norm,
                logits=logits, hidden=hidden, c_adamw=c_adamw, log_std=log_std)


# (a) hidden 128, both kernels.  name, kind, obs, act (classes), horizon, minibatch, epochs, seed
ONCHIP = [
    case("relu-8-2-100-24", "gauss", 8, 2, 100, 24, 2, 0),          # minibatches 24 24 24 24 4: a partly filled wave, empty waves, 1/m changes
    case("relu-16-1-70-64", "gauss", 16, 1, 70, 64, 2, 1),          # k_pad exactly 16, one head column, 6-row tail
    case("relu-17-16-150-70", "gauss", 17, 16, 150, 70, 2, 0),      # two k-blocks, full head tile, second chunk of 6 rows, 10-row tail
    case("relu-32-5-130-129", "gauss", 32, 5, 130, 129, 2, 0),      # k_pad exactly 32, head ends in lane group 1, chunks 64 + 64 + 1, 1-row tail
    case("tanh-8-2-100-24", "gauss", 8, 2, 100, 24, 2, 0, tanh=True, adam_eps=True, adv_norm=True),
    case("tanh-17-5-100-24", "gauss", 17, 5, 100, 24, 2, 0, tanh=True, adam_eps=True, adv_norm=True),
    case("cat-4-2-100-24", "cat", 4, 2, 100, 24, 2, 2, adv_norm=True),
    case("cat-4-5-100-24", "cat", 4, 5, 100, 24, 2, 2, adv_norm=True),
    case("cat-4-16-100-24", "cat", 4, 16, 100, 24, 2, 1, adv_norm=True),
    case("logits-4-5-100-24", "cat", 4, 5, 100, 24, 2, 2, adv_norm=True, logits=True),
    # the first shape with one raw log_std past the clamp (2.5: std = e^2, no gradient; 0.5 from the bound, so the condition on log_std
    # below holds as it stands) and the other interior: the gated column stays bit-unchanged and its Adam moments 0 (tests/test_gpu_ppo_edges.py)
    case("relu-8-2-100-24-clamp", "gauss", 8, 2, 100, 24, 2, 0, log_std=((0, 2.5),)),
]
# (b) shapes only the streaming kernel serves
STREAMING_ONLY = [
    case("relu-33-5-100-24", "gauss", 33, 5, 100, 24, 2, 2),
    case("relu-8-17-96-40", "gauss", 8, 17, 96, 40, 2, 1),           # head past one tile
    case("relu-11-3-100-24-h64", "gauss", 11, 3, 100, 24, 2, 1, hidden=64),
    case("relu-11-3-100-24-h256", "gauss", 11, 3, 100, 24, 2, 3, hidden=256),
    case("beta-8-2-100-24", "beta", 8, 2, 100, 24, 2, 0, adv_norm=True),
    case("cadamw-8-2-100-24", "gauss", 8, 2, 100, 24, 2, 0, c_adamw=True),
]
# (d) three learners at (a)'s first shape, each with its own table, parameters and permutations
POPULATION = [case("pop%d-8-2-100-24" % p, "gauss", 8, 2, 100, 24, 2, s) for p, s in enumerate((1, 2, 4))]
ALL_CASES = ONCHIP + STREAMING_ONLY + POPULATION
# (c) adv_norm through the first actor loss: mb = T, K = 1
ADV_NORM = [case("advnorm-8-2-2", "gauss", 8, 2, 2, 2, 1, 0, adv_norm=True), case("advnorm-8-2-300", "gauss", 8, 2, 300, 300, 1, 0, adv_norm=True)]
GAE_HORIZONS = [2, 63, 257, 300, 1000]
GAE_O, GAE_A, GAE_SEED, GAE_LAST_VALUE = 8, 2, 40, 0.37


def n_steps(c):
    return c["K"] * ((c["T"] + c["mb"] - 1) // c["mb"])


def trick(c):
    return dict(adv_norm=c["adv_norm"], tanh=c["tanh"], adam_eps=c["adam_eps"])


def new_oracle(c, params, horizon=None, rollout_values=False):
    from oracle import ppo as oppo
    return oppo.PPO(params["actor"], params["critic"], c["O"], c["A"], LR, LR, horizon or c["T"], trick(c), discrete=c["kind"] == "cat",
                    beta=c["kind"] == "beta", optimizer="c_adamw" if c["c_adamw"] else "adam", cat_logits=c["logits"],
                    rollout_values=rollout_values)


def fill(orc, tab, values=None):
    disc = orc.discrete
    for i in range(len(tab["rew"])):
        extra = () if values is None else (float(values[i]),)
        orc.add(tab["obs"][i], tab["act"][i][0] if disc else tab["act"][i], float(tab["rew"][i]), tab["next_obs"][i], bool(tab["done"][i]),
                tab["logp"][i], bool(tab["adv_done"][i]), *extra)


def _inputs(name, kind, O, A, T, K, seed, hidden, tanh, logits, log_std=None):
    g = dict(obs_dim=O, act_dim=A, n_actions=A, horizon=T, k_epochs=K, hidden=hidden, table_seed=52000 + 10 * seed, param_seed=53000 + 10 * seed,
             perm_seed=54000 + 10 * seed)
    inp = {"gauss": gcases.ppo_inputs, "cat": gcases.ppo_discrete_inputs, "beta": gcases.ppo_beta_inputs}[kind](g)
    tab = inp["table"]
    for col, v in log_std or ():
        inp["params"]["actor"]["log_std"][0, col] = F32(v)
    c = case(name, kind, O, A, T, T, K, seed, tanh=tanh, logits=logits, hidden=hidden)
    orc = new_oracle(c, inp["params"])
    r = np.random.default_rng(55000 + 10 * seed)
    act, logp = tab["act"].copy(), tab["logp"].copy()
    if kind == "gauss":
        eps = r.standard_normal((T, A)).astype(F32)
        for i in range(T):
            act[i], logp[i] = orc.select_action(tab["obs"][i], eps[i])
        logp = logp + (0.3 / math.sqrt(A)) * r.standard_normal((T, A))
    elif kind == "cat":
        q = r.exponential(size=(T, A)).astype(F32)
        for i in range(T):
            act[i, 0], logp[i, 0] = orc.select_action_discrete(tab["obs"][i], q[i])
        logp = logp + 0.3 * r.standard_normal((T, 1))
    tab["act"], tab["logp"] = act.astype(F32), logp.astype(F32)
    return inp


def inputs(c):
    """dict(table, params, perms) of a case: the golden builders' table, parameters and permutations, stored actions and
    log-probs from the oracle's policy (module docstring).  Cached: do not write into it."""
    return _cached_inputs(c["name"], c["kind"], c["O"], c["A"], c["T"], c["K"], c["seed"], c["hidden"], c["tanh"], c["logits"], c["log_std"])


_cached_inputs = functools.lru_cache(maxsize=None)(_inputs)


def _learn(c, params):
    inp = inputs(c)
    orc = new_oracle(c, params)
    fill(orc, inp["table"])
    orc.ratio_log, orc.preact_log = [], []
    orc.learn_with(inp["perms"], c["mb"], GAMMA, LMBDA, CLIP, c["K"], ENT)
    return orc


def _twin_spread(c, orc):
    """The oracle's own conditioning: the largest change of any final parameter, in units of the parameter tolerance, when the
    initial parameters move by one float32 rounding (relative N(0, eps32^2), three draws)."""
    if c["c_adamw"]:                  # the cautious mask flips elements on such a change: that case has its own rule
        return 0.0
    worst = 0.0
    for draw in range(3):
        r = np.random.default_rng(58000 + 10 * c["seed"] + draw)
        moved = {n: {k: (v * (1 + EPS32 * r.standard_normal(v.shape))).astype(F32) for k, v in inputs(c)["params"][n].items()} for n in ("actor", "critic")}
        twin = _learn(c, moved)
        for ref, got in ((orc.actor, twin.actor), (orc.critic, twin.critic)):
            worst = max([worst] + [float((np.abs(got[k] - ref[k]) / (PARAM_ATOL + PARAM_RTOL * np.abs(ref[k]))).max()) for k in ref])
    return worst


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    c = BY_NAME[name]
    orc = _learn(c, inputs(c)["params"])
    return dict(twin_spread=_twin_spread(c, orc), actor_losses=np.array(orc.actor_losses, F32), critic_losses=np.array(orc.critic_losses, F32), actor=orc.actor, critic=orc.critic,
                adv=orc.adv_raw.reshape(-1), v_target=orc.v_target.reshape(-1), log=orc.ratio_log, preact=orc.preact_log)


def oracle_run(c):
    """oracle.ppo.PPO.learn_with on the case: loss traces, final parameters, raw advantages, value targets, the ratio log."""
    return _oracle_run(c["name"])


def assert_conditions(c, run=None):
    """The conditions on the inputs (module docstring), from the oracle alone."""
    run = run or oracle_run(c)
    log, name = run["log"], c["name"]
    assert len(log) == n_steps(c) == len(run["actor_losses"]) == len(run["critic_losses"]), name
    assert np.isfinite(run["actor_losses"]).all() and np.isfinite(run["critic_losses"]).all(), name
    for i, (ratio, clamped, ls) in enumerate(log):
        edge = np.minimum(np.abs(ratio - (1 - CLIP)), np.abs(ratio - (1 + CLIP))).min()
        assert edge > 1e-4, "%s step %d: a ratio within %.1e of a clip edge: choose another seed" % (name, i, edge)
        assert 0.1 <= ratio.min() and ratio.max() <= 10, "%s step %d: ratios in [%g, %g]" % (name, i, ratio.min(), ratio.max())
        if ls is not None:
            assert np.minimum(np.abs(ls + 20), np.abs(ls - 2)).min() > 1e-3, "%s step %d: log_std at its clamp" % (name, i)
    if "log_std" in run["actor"]:
        ls = run["actor"]["log_std"]
        assert np.minimum(np.abs(ls + 20), np.abs(ls - 2)).min() > 1e-3, name
    if not c["tanh"] or c["kind"] == "cat":
        assert len(run["preact"]) >= 4 * n_steps(c) and min(run["preact"]) > KINK, "%s: a ReLU pre-activation at %.1e: choose another seed" % (name, min(run["preact"]))
    assert run["twin_spread"] < TWIN_SPREAD, "%s: an element moves by %.2f of the tolerance under a rounding of the parameters: choose another seed" % (name, run["twin_spread"])
    frac = log[0][1].mean()
    assert 0.1 <= frac <= 0.5, "%s: %.0f %% of the first minibatch on the clamped branch: choose another seed" % (name, 100 * frac)


BY_NAME = {c["name"]: c for c in ALL_CASES + ADV_NORM}
assert len(BY_NAME) == len(ALL_CASES) + len(ADV_NORM)


# ------------------------------------------------------------------------------------------------ GAE
def gae_c32():
    return F32(F32(GAMMA) * F32(LMBDA))


def gae_f64(delta, adv_done, c):
    """(A, S): the sequential recurrence on float64 copies of delta and adv_done, and the same recurrence on |delta|."""
    d, ad, c = np.asarray(delta, np.float64), np.asarray(adv_done, np.float64), float(c)
    A, S = np.zeros(len(d)), np.zeros(len(d))
    a = s = 0.0
    for t in reversed(range(len(d))):
        g = c * (1.0 - ad[t])
        a, s = d[t] + g * a, abs(d[t]) + g * s
        A[t], S[t] = a, s
    return A, S


def gae_bound(T, S):
    L = (T + KWG - 1) // KWG
    return 3 * (2 * L + 12) * EPS32 * S


def sb3_f64(rew, done, adv_done, values, last_value, gamma, lmbda):
    """BufferForPPO2.compute_returns_and_advantage (stable-baselines3's form) on float64 copies -> (advantages, returns)."""
    rew, done, ad, v = (np.asarray(x, np.float64).reshape(-1) for x in (rew, done, adv_done, values))
    adv, last = np.zeros(len(rew)), 0.0
    for t in reversed(range(len(rew))):
        nv = float(last_value) if t == len(rew) - 1 else v[t + 1]
        delta = rew[t] + gamma * nv * (1.0 - done[t]) - v[t]
        last = delta + gamma * lmbda * (1.0 - ad[t]) * last
        adv[t] = last
    return adv, adv + v


def gae_scan_f32(delta, adv_done, c):
    """gae_scan (kernels_ppo.hip) in NumPy float32, in the kernel's order: thread t folds rows [t L, t L + L) into an affine
    map, an inclusive suffix scan over the 64 lanes of each wave in six shuffle levels, the four wave totals chained from
    the right, then each thread replays its rows from the value entering its segment.  (Separate multiply and add.)"""
    d, ad, c = np.asarray(delta, F32), np.asarray(adv_done, F32), F32(c)
    T = len(d)
    L = (T + KWG - 1) // KWG
    g = c * (F32(1) - ad)
    seg = [(min(t * L, T), min(min(t * L, T) + L, T)) for t in range(KWG)]
    fa, fb = np.ones(KWG, F32), np.zeros(KWG, F32)
    for t, (s0, s1) in enumerate(seg):
        for i in reversed(range(s0, s1)):
            fa[t], fb[t] = g[i] * fa[t], d[i] + g[i] * fb[t]
    sa, sb = fa.reshape(-1, WAVE).copy(), fb.reshape(-1, WAVE).copy()
    off = 1
    while off < WAVE:
        oa, ob = sa[:, off:].copy(), sb[:, off:].copy()
        sa[:, :-off], sb[:, :-off] = sa[:, :-off] * oa, sa[:, :-off] * ob + sb[:, :-off]      # compose(s, o) = s(o(x))
        off *= 2
    n_waves = KWG // WAVE
    right = np.zeros(n_waves, F32)
    for w in range(n_waves):
        for ww in range(n_waves - 1, w, -1):
            right[w] = sa[ww, 0] * right[w] + sb[ww, 0]
    mine = sa * right[:, None] + sb
    x = np.concatenate([mine[:, 1:], right[:, None]], axis=1).reshape(-1)
    adv = np.zeros(T, F32)
    for t, (s0, s1) in enumerate(seg):
        v = x[t]
        for i in reversed(range(s0, s1)):
            v = d[i] + g[i] * v
            adv[i] = v
    return adv


def adv_done_patterns(T):
    """name -> adv_done [T] (bool): none, all, last row only and, from T = 257 up, the rows either side of segment seams
    (L t - 1, L t) and of wave seams (64 L w - 1, 64 L w)."""
    L = (T + KWG - 1) // KWG
    out = {"none": np.zeros(T, bool), "all": np.ones(T, bool), "last": np.arange(T) == T - 1}
    if T >= 257:
        seams = [L * t for t in (1, 2, 7, 63, 65, 100, 127, 128)] + [WAVE * L * w for w in (1, 2, 3)]
        rows = sorted({r for s in seams for r in (s - 1, s) if 0 <= r < T})
        assert len(rows) >= 12
        out["seams"] = np.isin(np.arange(T), rows)
    return out


@functools.lru_cache(maxsize=None)
def gae_inputs(T):
    """One table and parameter set per horizon (O = 8, A = 2) with `done` set on about one row in twelve, on rows 0 and T // 2 and
    not on the last row, so that it differs from every adv_done pattern on some rows (truncation), and the oracle's float32 V(s), td and stored values."""
    c = case("gae-%d" % T, "gauss", GAE_O, GAE_A, T, T, 1, GAE_SEED)
    inp = _inputs(c["name"], "gauss", GAE_O, GAE_A, T, 1, GAE_SEED, 128, False, False)
    tab = inp["table"]
    r = np.random.default_rng(56000 + T)
    tab["done"] = r.random(T) < 1 / 12
    tab["done"][[0, T // 2]], tab["done"][T - 1] = True, False
    tab["value"] = (0.8 * r.standard_normal(T)).astype(F32)
    orc = new_oracle(c, inp["params"])
    obs, nobs = tab["obs"].astype(F32), tab["next_obs"].astype(F32)
    vs = orc.v.forward(orc.critic, obs)[0].reshape(-1)
    vs_ = orc.v.forward(orc.critic, nobs)[0].reshape(-1)
    nd = F32(1.0) - tab["done"].astype(F32)
    rew = tab["rew"].astype(F32).reshape(-1).copy()
    for _ in range(8):                # rewards moved off the cancellation, see TD_FLOOR
        td = rew + F32(GAMMA) * nd * vs_ - vs
        scale = np.abs(rew) + F32(GAMMA) * nd * np.abs(vs_) + np.abs(vs)
        low = np.abs(td) < 2 * TD_FLOOR * scale
        if not low.any():
            break
        rew[low] += np.where(td[low] < 0, F32(-1), F32(1))
    tab["rew"] = rew
    return dict(case=c, inp=inp, vs=vs.astype(F32), td=td.astype(F32), scale=scale.astype(np.float64))


def assert_gae_conditions(T):
    g = gae_inputs(T)
    assert (np.abs(g["td"]) >= TD_FLOOR * g["scale"]).all(), T
    assert g["inp"]["table"]["rew"].dtype == F32 and np.isfinite(g["td"]).all()
