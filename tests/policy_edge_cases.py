"""Inputs and the float64 reference shared by tests/test_policy_edge_cases.py (CPU) and tests/test_gpu_policy_edges.py (GPU): the
continuous-policy arithmetic of device/policy.hpp — the log_std clamp to [-20, 2], the clamp's gradient gate, the tanh-Gaussian
log-prob, TD3's target-policy smoothing — at its clamp and clip edges, on every kernel family that runs it.

Inputs start from tests/golden/cases.py:ac_inputs (table, parameters, index sets, noise) and are overridden as follows.
  * SAC log_std layouts (LAYOUTS; every value is exact in float32): `upper` [2.0, 2.5, ...], `lower` [-20.0, -21.0, ...], `mixed`
    [-20, -21, -0.3, 2.0, 2.5, 0.1, ...], `seam` (20 actions: 2.5, -20.0, 2.0, -21.0, 2.5 at columns 0, 3, 15, 16, 19, either side of
    the 16-column head tile's seam), `tdiff` (the target actor's log_std is interior where the online one is clamped and clamped
    where the online one is interior), `interior`.  A column at exactly 2.0 or -20.0 is on the closed bound: clamped to itself, gradient
    passes.  A column at 2.5 or -21.0 is clamped and its gradient is gated off: it must never move, nor its Adam moments.
  * alpha starts at 0.2 with alpha_lr 1e-3 and target_entropy -act, so that the entropy terms carry weight in the TD target and in
    the actor loss (at the parity tests' 0.01 an error in the log-prob enters at 1 % of its size).
  * both noise sets are ZERO on every column whose clamped log_std (online or target copy) is -20: at sd = 2e-9, u - mean falls under
    half an ulp of the mean and float32 keeps an arbitrary part of eps^2 / 2 (tests/masac_oracle.py records the same finding).
    With zero noise u == mean exactly, the log-prob term is 20 - log sqrt(2 pi) and the log_std gradient before the norm clip is
    exactly -alpha where the gate is open and 0 where it is closed.
  * `satmean`: mean_layer.weight of both actor copies times SAT_GAIN, so that a share of the rows has |u| > 10 on either sign: there
    softplus(-2u) takes its threshold branch (-2u > 20) and tanh(u) == -+1 in float32.
  * TD3: policy_noise 0.5, noise_clip 0.2, policy_noise_scale 0.5, max_action 2.0 — noise = clip(0.25 z, -+0.2) clips 42 % of the
    draws, and the order of scaling and clipping matters — and the target actor's head weight times TD3_GAIN, so that
    tanh(.) max_action + noise leaves [-max_action, max_action] on both sides.
  * the target copies of every net are the online ones plus N(0, 0.01^2): a pass that reads the wrong copy shows.
  * every index set holds at least two rows with done == 1 (the first two rows of every set are made terminal in the table).

`assert_conditions` qualifies a case from this module's float64 reference and the project's float32 oracle (oracle/algos.py)
alone, before any engine exists: the float32 oracle stays within ORACLE_SHARE = 0.25 of every tolerance of the GPU test against
float64 (ppo_edge_cases.TWIN_SPREAD's margin: three quarters of each tolerance are left to the kernels' summation order); no ReLU
pre-activation of any forward of any call is within KINK = 1e-6 of 0; the clip populations (TD3: >= 25 % of the noise entries at
-+noise_clip and 10 % .. 50 % of the target-action entries at -+max_action, both signs present with at least 5 % each; satmean:
>= 10 % of the entries with |u| > 10 on each sign, in both passes of every call); every column that starts exactly on a bound has
moved by 0.5 .. 1.5 lr after the first call, and no log_std lies within 1e-5 of a bound afterwards.  No row, element or case is
left out of a comparison: where a case missed a condition its seed or gain was changed (recorded in the case list).

Measured on the CPU, float32 oracle against the float64 reference as a fraction of each tolerance, worst over the calls and over
every case of a group (MEASURED below holds the same figures; tests/test_policy_edge_cases.py keeps them true):
    log_std layouts (upper, lower, mixed, seam, tdiff, interior)   losses 0.004   alpha 0.014   parameters 0.156
    satmean                                                        losses 0.004   alpha 0.015   parameters 0.041
    TD3                                                            losses 0.004   (no alpha)    parameters 0.152
    forward checks (act_checks): at most 0.01 of the sample's tolerance, 0.11 of the tanh heads'
"""
import functools
import math

import numpy as np

from tests.golden import cases as gcases
from tests.golden import synth

F32, F64 = np.float32, np.float64
GAMMA, TAU, LR = 0.99, 0.005, 1e-3
ALPHA0, ALPHA_LR = 0.2, 1e-3
TD3_KW = dict(policy_noise=0.5, noise_clip=0.2, policy_noise_scale=0.5, max_action=2.0)
POLICY_FREQ = 2
SAC_CALLS, TD3_CALLS = 3, 4
N_TABLE, BATCH_MAX = 300, 64
SAT_GAIN = 200.0        # satmean: |mean| of sd ~ 15, a quarter of the entries past 10 on either side (40 and 100 left under 10 % there)
TD3_GAIN = 30.0         # TD3: the target actor's head at |pre-activation| ~ 3 (8 .. 20 left under 5 % of the target actions on the lower clip)
# the project's tolerances (tests/test_gpu_parity.py), unchanged
LOSS_RTOL, ACTOR_LOSS_ATOL, ALPHA_RTOL = 1e-4, 2e-6, 1e-5
P_RTOL, P_ATOL = 5e-4, 5e-6
ORACLE_SHARE = 0.25
KINK = 1e-6              # ppo_edge_cases.KINK, same reasoning
LS_MIN, LS_MAX = -20.0, 2.0
LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)
LOG2 = math.log(2.0)

# worst float32-oracle-against-float64 fraction of the tolerance per group of cases: (losses, alpha, parameters)
MEASURED = {
    "sac-clamp": (0.01, 0.02, 0.16),       # upper / lower / mixed / seam / tdiff / interior; the largest: sac-head2h256-seam-b64's parameters
    "sac-satmean": (0.01, 0.02, 0.05),
    "td3": (0.01, 0.00, 0.16),             # the largest: td3-h256-b17's parameters
}
# ... and with the noise NOT zeroed on the lower-edge columns (sac-narrow-lower-b64 otherwise as it is): 0.3 of the loss tolerance after
# the first call and past the parameter tolerance (test_unzeroed_noise_on_the_lower_edge_is_the_number_formats asserts > 1 there)

# obs, act, hidden and the kernel families that serve the shape: family -> FRL_CRITIC_V2 ("0", "1" or None = unset, one learner)
SHAPES = {
    "narrow": dict(O=11, A=3, H=128, families=dict(rowchunk="0", chained="1", solo=None)),
    "wide": dict(O=17, A=6, H=128, families=dict(rowchunk="0", ksliced="1", solow=None)),
    "h256": dict(O=11, A=3, H=256, families=dict(rowchunk="0", xstationary="1")),
    "head2": dict(O=12, A=20, H=128, families=dict(rowchunk="0", ksliced="1", solow=None)),
    "head2h256": dict(O=12, A=20, H=256, families=dict(rowchunk="0", xstationary="1")),
}
# what frl_learn_path reports for a chained family: (True, dynamic LDS bytes, rows per workgroup) (frl_desc.h / engine_plan.hpp: solo_lds_floats,
# solow_lds_floats, wide_lds_floats, wide16_lds_floats_host; the register-chained kernels and the two wide families walk the whole batch)
SOLO_LDS = 117376
SOLOW_LDS = 4 * (64 * 256 + 2 * 8 * 256 + 128 + 128 + 32 + 32 + 4 * 8 * 256 + 26 * 256 + 3 * 256 + 256 + 4 * 2 * 256 + 16 * 32 + 16 * 48 + 128)
WIDE_LDS = 4 * (8 * 8 * 256 + 2 * 8 * 256 + 2 * 8192 + 128 + 128 + 32 + 32 + 64)
WIDE16_LDS = 4 * (16384 + 2 * 16 * 256 + 3 * 16 * 256 + 256 + 256 + 32 + 32 + 192)


def path_is(family, path, batch):
    """Does frl_learn_path's answer name `family`?"""
    chained, lds, rows = path
    if family == "rowchunk":
        return not chained
    if family == "solo":
        return path == (True, SOLO_LDS, 16)
    if family == "solow":
        return path == (True, SOLOW_LDS, 16)
    if family == "ksliced":
        return path == (True, WIDE_LDS, batch)
    if family == "xstationary":
        return path == (True, WIDE16_LDS, batch)
    assert family == "chained", family
    return chained and rows == batch and lds not in (SOLO_LDS, SOLOW_LDS, WIDE_LDS, WIDE16_LDS)


# column -> raw log_std; the other columns keep ac_inputs' uniform(-0.5, 0.3) draw
LAYOUTS = {
    "interior": {},
    "upper": {0: 2.0, 1: 2.5},
    "lower": {0: -20.0, 1: -21.0},
    "mixed": {0: -20.0, 1: -21.0, 2: -0.3, 3: 2.0, 4: 2.5, 5: 0.1},
    "seam": {0: 2.5, 3: -20.0, 15: 2.0, 16: -21.0, 19: 2.5},
    "tdiff": {0: 2.5, 2: -21.0, 4: 2.0, 5: -20.0},          # (columns past the head's width are dropped)
}
TARGET_LAYOUTS = {"tdiff": {1: 2.5, 3: -21.0}}             # the target copy's own columns; every other target column is a fresh interior draw


def case(name, algo, shape, batch, seed, layout=None, act_seed=0):
    s = SHAPES[shape]
    return dict(name=name, algo=algo, shape=shape, O=s["O"], A=s["A"], H=s["H"], batch=batch, seed=seed, layout=layout, act_seed=act_seed,
                n_calls=SAC_CALLS if algo == "sac" else TD3_CALLS)


# name, algorithm, shape, batch, seed, log_std layout, seed of the forward checks' inputs (both seeds chosen so that assert_conditions holds)
SAC_CASES = [
    case("sac-narrow-upper-b17", "sac", "narrow", 17, 0, "upper"),
    case("sac-narrow-lower-b64", "sac", "narrow", 64, 0, "lower"),
    case("sac-narrow-tdiff-b64", "sac", "narrow", 64, 5, "tdiff"),
    case("sac-narrow-satmean-b17", "sac", "narrow", 17, 2, "satmean", act_seed=4),
    case("sac-wide-mixed-b17", "sac", "wide", 17, 0, "mixed"),
    case("sac-wide-tdiff-b64", "sac", "wide", 64, 0, "tdiff"),
    case("sac-wide-satmean-b64", "sac", "wide", 64, 0, "satmean", act_seed=135),
    case("sac-h256-upper-b64", "sac", "h256", 64, 25, "upper"),
    case("sac-h256-lower-b17", "sac", "h256", 17, 1, "lower"),
    case("sac-head2-seam-b17", "sac", "head2", 17, 0, "seam"),
    case("sac-head2h256-seam-b64", "sac", "head2h256", 64, 12, "seam"),
]
TD3_CASES = [
    case("td3-narrow-b17", "td3", "narrow", 17, 2, act_seed=72),
    case("td3-narrow-b64", "td3", "narrow", 64, 1, act_seed=30),
    case("td3-wide-b64", "td3", "wide", 64, 5, act_seed=4),
    case("td3-h256-b17", "td3", "h256", 17, 1, act_seed=83),
]
# three learners of one engine at the narrow shape, each with its own layout, parameters, table, index sets and noise
POPULATION = [
    case("pop0-narrow-upper-b17", "sac", "narrow", 17, 1, "upper"),
    case("pop1-narrow-lower-b17", "sac", "narrow", 17, 3, "lower"),
    case("pop2-narrow-interior-b17", "sac", "narrow", 17, 4, "interior"),
]
POPULATION_FAMILIES = ("rowchunk", "chained")
ALL_CASES = SAC_CASES + TD3_CASES + POPULATION
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)
PAIRS = [(c, f) for c in SAC_CASES + TD3_CASES for f in SHAPES[c["shape"]]["families"]]
SAC_PAIRS = [(c, f) for c, f in PAIRS if c["algo"] == "sac"]

ACTOR_NAMES = {"sac": ["l1", "l2", "mean_layer"], "td3": ["l1", "l2", "l3"]}
CRITIC_NAMES = ["l1", "l2", "l3", "l4", "l5", "l6"]


# ------------------------------------------------------------------------------------------------ inputs
def _moved(params, seed, skip=()):
    """A target copy: every tensor plus N(0, 0.01^2), float32."""
    g = np.random.default_rng(seed)
    return {k: (v if k in skip else (v + F32(0.01) * g.standard_normal(v.shape).astype(F32)).astype(F32)) for k, v in params.items()}


def _spec(name, zero_noise=True):
    c = BY_NAME[name]
    O, A, H, B, s, sac = c["O"], c["A"], c["H"], c["batch"], c["seed"], c["algo"] == "sac"
    g = dict(obs_dim=O, act_dim=A, n_table=N_TABLE, batch=B, n_learn=c["n_calls"], table_seed=61000 + 10 * s, param_seed=62000 + 10 * s,
             idx_seed=63000 + 10 * s, noise_seed=64000 + 100 * s)
    inp = gcases.ac_inputs(g, twin=True, gaussian=sac)
    actor, critic = inp["params"]["actor"], inp["params"]["critic"]
    if H != gcases.H:                 # ac_inputs builds the reference's hidden 128: the same draws at this width
        head = "mean_layer" if sac else "l3"
        body = synth.mlp_params(g["param_seed"], gcases.actor_layers(O, A, head=head, hidden=H))
        actor = dict(([("log_std", actor["log_std"])] if sac else []) + list(body.items()))
        critic = synth.mlp_params(g["param_seed"] + 1, gcases.critic_layers(O + A, twin=True, hidden=H))
    actor_t, critic_t = _moved(actor, 65000 + 10 * s, skip=("log_std",)), _moved(critic, 65001 + 10 * s)
    noise = [[n.copy() for n in call] for call in inp["noise"]]
    if sac:
        lay = c["layout"]
        ls = actor["log_std"].copy()
        for col, v in LAYOUTS.get(lay, {}).items():
            if col < A:
                ls[0, col] = F32(v)
        ls_t = ls.copy()
        if lay in TARGET_LAYOUTS:
            ls_t = np.random.default_rng(g["param_seed"] + 8).uniform(-0.5, 0.3, (1, A)).astype(F32)
            for col, v in TARGET_LAYOUTS[lay].items():
                if col < A:
                    ls_t[0, col] = F32(v)
        actor["log_std"], actor_t["log_std"] = ls, ls_t
        if lay == "satmean":
            for p in (actor, actor_t):
                p["mean_layer.weight"] = (p["mean_layer.weight"] * F32(SAT_GAIN)).astype(F32)
        zero = (np.clip(ls, LS_MIN, LS_MAX) == LS_MIN) | (np.clip(ls_t, LS_MIN, LS_MAX) == LS_MIN)
        for call in noise:
            for n in call:
                if zero_noise:
                    n[:, zero.reshape(-1)] = 0
    else:
        actor_t["l3.weight"] = (actor_t["l3.weight"] * F32(TD3_GAIN)).astype(F32)
    tab = {k: v.copy() for k, v in inp["table"].items()}
    for idx in inp["idx"]:
        tab["done"][idx[:2]] = True
    assert all(tab["done"][idx].sum() >= 2 for idx in inp["idx"])
    hyper = dict(gamma=GAMMA, tau=TAU, actor_lr=LR, critic_lr=LR)
    hyper.update(dict(alpha0=ALPHA0, alpha_lr=ALPHA_LR, target_entropy=-float(A)) if sac else dict(TD3_KW, policy_freq=POLICY_FREQ))
    return dict(algo=c["algo"], O=O, A=A, table=tab, idx=inp["idx"], noise=noise, actor=actor, critic=critic, actor_t=actor_t, critic_t=critic_t,
                hyper=hyper)


@functools.lru_cache(maxsize=None)
def spec(name):
    """The inputs of a case: table, index sets, noise, the four parameter sets, hyper-parameters.  Cached: do not write into it."""
    return _spec(name)


@functools.lru_cache(maxsize=None)
def golden_spec(kind):
    """The project's interior parity case tests.golden.cases.CASES[kind] ("sac" or "td3") in this module's input format."""
    g = gcases.CASES[kind]
    inp = gcases.ac_inputs(g, twin=True, gaussian=kind == "sac")
    hyper = dict(gamma=g["gamma"], tau=g["tau"], actor_lr=g["actor_lr"], critic_lr=g["critic_lr"])
    if kind == "sac":
        hyper.update(alpha0=0.01, alpha_lr=1e-4, target_entropy=-float(g["act_dim"]))
    else:
        hyper.update({k: g[k] for k in ("policy_noise", "noise_clip", "policy_noise_scale", "max_action", "policy_freq")})
    a, c = inp["params"]["actor"], inp["params"]["critic"]
    return dict(algo=kind, O=g["obs_dim"], A=g["act_dim"], table=inp["table"], idx=inp["idx"], noise=inp["noise"], actor=a, critic=c, actor_t=a, critic_t=c,
                hyper=hyper)


# ------------------------------------------------------------------------------------------------ the float64 reference
def _f64(p):
    return {k: np.array(v, dtype=F64) for k, v in p.items()}


def _forward(p, names, x, kink, out_tanh=False):
    """Linear layers with ReLU between them (oracle.nn.MLP.forward); the smallest |pre-activation| of every hidden layer goes to `kink`."""
    acts, h = [x], x
    for i, n in enumerate(names):
        z = h @ p[n + ".weight"].T + p[n + ".bias"]
        if i < len(names) - 1:
            kink.append(float(np.abs(z).min()))
            h = np.maximum(z, 0.0)
        else:
            h = np.tanh(z) if out_tanh else z
        acts.append(h)
    return h, acts


def _backward(p, names, acts, dy, out_tanh=False, need_dx=False):
    g, d = {}, dy
    for i in reversed(range(len(names))):
        n, h = names[i], acts[i + 1]
        if i < len(names) - 1:
            d = d * (h > 0)
        elif out_tanh:
            d = d * (1.0 - h * h)
        g[n + ".weight"], g[n + ".bias"] = d.T @ acts[i], d.sum(axis=0)
        if i > 0 or need_dx:
            d = d @ p[n + ".weight"]
    return (d if need_dx else None), g


class _Adam:
    """torch.optim.Adam's defaults as oracle.nn.Adam states them."""

    def __init__(self, params, lr):
        self.lr, self.t = lr, 0
        self.m = {k: np.zeros_like(v) for k, v in params.items()}
        self.v = {k: np.zeros_like(v) for k, v in params.items()}

    def step(self, params, grads):
        self.t += 1
        bc1, bc2 = 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t
        for k in params:
            g = grads[k]
            self.m[k] = self.m[k] + (g - self.m[k]) * 0.1
            self.v[k] = 0.999 * self.v[k] + 0.001 * g * g
            params[k] = params[k] - (self.lr / bc1) * (self.m[k] / (np.sqrt(self.v[k]) / math.sqrt(bc2) + 1e-8))


def _clip_grad_norm(grads, max_norm=0.5):
    total = math.sqrt(sum(float((g * g).sum()) for g in grads.values()))
    coef = min(max_norm / (total + 1e-6), 1.0)
    return {k: g * coef for k, g in grads.items()}


def _soft_update(target, source, tau):
    for k in target:
        target[k] = target[k] * (1.0 - tau) + source[k] * tau


def _softplus(x):
    return np.logaddexp(0.0, x)


# Near misses of device/policy.hpp that the GPU test must tell from the reference.  Reference(sp, mutation) computes each of them in float64;
# tests/test_policy_edge_cases.py shows that every one leaves the tolerances (or breaks the bit-level gate assertions) on the cases it bears on.
MUTATIONS = ("gate-strict",               # log_std_grad_open with > / < instead of >= / <=
             "gate-removed",              # the gate missing at a call site
             "target-unclamped",          # clamp_log_std dropped from the target pass
             "clip-before-scale",         # td3_smooth clipping before it scales by policy_noise_scale
             "softplus-threshold-zero")   # softplus_t's threshold branch returning 0


class Reference:
    """One SAC or TD3 learner in float64: oracle.algos.SAC.learn_with / TD3.learn_with (GaussianActor.forward / backward, _critic_step,
    clip_grad_norm 0.5, Adam, soft update) restated on float64 copies of the float32 inputs."""

    Q1, Q2 = CRITIC_NAMES[:3], CRITIC_NAMES[3:]

    def __init__(self, sp, mutation=None):
        assert mutation in (None,) + MUTATIONS, mutation
        self.mutation = mutation
        self.sp, self.h, self.sac = sp, sp["hyper"], sp["algo"] == "sac"
        self.names = ACTOR_NAMES[sp["algo"]]
        self.actor, self.critic, self.actor_t, self.critic_t = (_f64(sp[k]) for k in ("actor", "critic", "actor_t", "critic_t"))
        self.actor_opt, self.critic_opt = _Adam(self.actor, self.h["actor_lr"]), _Adam(self.critic, self.h["critic_lr"])
        if self.sac:
            self.log_alpha = {"log_alpha": np.array(math.log(self.h["alpha0"]))}
            self.alpha = self.h["alpha0"]
            self.alpha_opt = _Adam(self.log_alpha, self.h["alpha_lr"])
        tab = sp["table"]
        self.tab = dict(obs=tab["obs"].astype(F64), act=tab["act"].astype(F64), rew=tab["rew"].astype(F64).reshape(-1, 1),
                        next_obs=tab["next_obs"].astype(F64), done=tab["done"].astype(F64).reshape(-1, 1))
        self.total_it = 0
        self.kink, self.log = [], []

    # GaussianActor.forward
    def pi(self, p, obs, eps, target=False):
        mean, acts = _forward(p, self.names, obs, self.kink)
        log_std = np.broadcast_to(p["log_std"], mean.shape)
        if not (target and self.mutation == "target-unclamped"):
            log_std = np.clip(log_std, LS_MIN, LS_MAX)
        std = np.exp(log_std)
        u = mean + std * eps
        lp = -((u - mean) ** 2) / (2.0 * std * std) - log_std - LOG_SQRT_2PI
        sp_ = _softplus(-2.0 * u)
        if self.mutation == "softplus-threshold-zero":
            sp_ = np.where(-2.0 * u > 20.0, 0.0, sp_)
        log_pi = lp.sum(axis=1, keepdims=True) - (2.0 * (LOG2 - u - sp_)).sum(axis=1, keepdims=True)
        a = np.tanh(u)
        return a, log_pi, dict(acts=acts, std=std, u=u, eps=eps, a=a)

    def _critic_step(self, oa, y):
        g, loss = {}, 0.0
        for names in (self.Q1, self.Q2):
            q, acts = _forward(self.critic, names, oa, self.kink)
            diff = q - y
            loss += float(np.mean(diff * diff))
            g.update(_backward(self.critic, names, acts, diff * (2.0 / diff.size))[1])
        self.critic_opt.step(self.critic, _clip_grad_norm({k: g[k] for k in self.critic}))
        return loss

    def _rows(self, idx):
        return tuple(self.tab[k][idx] for k in ("obs", "act", "rew", "next_obs", "done"))

    def learn_sac(self, idx, eps_next, eps_new):
        h = self.h
        obs, act, rew, nobs, done = self._rows(idx)
        B = obs.shape[0]
        a_next, logpi_next, ct = self.pi(self.actor_t, nobs, eps_next.astype(F64), target=True)
        oa_next = np.concatenate([nobs, a_next], axis=1)
        next_q = np.minimum(_forward(self.critic_t, self.Q1, oa_next, self.kink)[0], _forward(self.critic_t, self.Q2, oa_next, self.kink)[0])
        y = rew + h["gamma"] * (1.0 - done) * (next_q + self.alpha * (-logpi_next))
        closs = self._critic_step(np.concatenate([obs, act], axis=1), y)
        a_new, logpi, cache = self.pi(self.actor, obs, eps_new.astype(F64))
        oa_new = np.concatenate([obs, a_new], axis=1)
        q1, acts1 = _forward(self.critic, self.Q1, oa_new, self.kink)
        q2, acts2 = _forward(self.critic, self.Q2, oa_new, self.kink)
        entropy = -logpi
        aloss = float(np.mean(-(q1 + q2) / 2.0 - self.alpha * entropy))
        dq = np.full_like(q1, -0.5 / B)
        da = (_backward(self.critic, self.Q1, acts1, dq, need_dx=True)[0] + _backward(self.critic, self.Q2, acts2, dq, need_dx=True)[0])[:, obs.shape[1]:]
        dlogpi = np.full_like(logpi, self.alpha / B)
        # GaussianActor.backward
        a, u, std, eps = cache["a"], cache["u"], cache["std"], cache["eps"]
        du = da * (1.0 - a * a) + dlogpi * (2.0 * np.tanh(u))
        g = _backward(self.actor, self.names, cache["acts"], du)[1]
        raw = self.actor["log_std"]
        gate = {"gate-strict": (raw > LS_MIN) & (raw < LS_MAX), "gate-removed": np.ones_like(raw, bool)}.get(self.mutation, (raw >= LS_MIN) & (raw <= LS_MAX))
        g["log_std"] = (du * std * eps - dlogpi).sum(axis=0, keepdims=True) * gate
        self.actor_opt.step(self.actor, _clip_grad_norm({k: g[k] for k in self.actor}))
        _soft_update(self.critic_t, self.critic, h["tau"])
        _soft_update(self.actor_t, self.actor, h["tau"])
        mean_term = float(np.mean(entropy - h["target_entropy"]))
        alpha_loss = self.alpha * mean_term
        self.alpha_opt.step(self.log_alpha, {"log_alpha": np.array(self.alpha * mean_term)})
        self.alpha = math.exp(float(self.log_alpha["log_alpha"]))
        self.log.append(dict(u_target=ct["u"], u_online=u))
        return closs, aloss, alpha_loss, self.alpha

    def learn_td3(self, idx, noise):
        h = self.h
        self.total_it += 1
        obs, act, rew, nobs, done = self._rows(idx)
        ma = h["max_action"]
        v = _forward(self.actor_t, self.names, nobs, self.kink, out_tanh=True)[0]
        n = np.clip(h["policy_noise_scale"] * (noise.astype(F64) * h["policy_noise"]), -h["noise_clip"], h["noise_clip"])
        if self.mutation == "clip-before-scale":
            n = h["policy_noise_scale"] * np.clip(noise.astype(F64) * h["policy_noise"], -h["noise_clip"], h["noise_clip"])
        a_next = np.clip(v * ma + n, -ma, ma) / ma
        oa_next = np.concatenate([nobs, a_next], axis=1)
        next_q = np.minimum(_forward(self.critic_t, self.Q1, oa_next, self.kink)[0], _forward(self.critic_t, self.Q2, oa_next, self.kink)[0])
        y = rew + h["gamma"] * next_q * (1.0 - done)
        closs = self._critic_step(np.concatenate([obs, act], axis=1), y)
        self.log.append(dict(noise=n, a_next=a_next))
        aloss = None
        if self.total_it % h["policy_freq"] == 0:
            a_new, pacts = _forward(self.actor, self.names, obs, self.kink, out_tanh=True)
            q, qacts = _forward(self.critic, self.Q1, np.concatenate([obs, a_new], axis=1), self.kink)
            aloss = float(-np.mean(q))
            da = _backward(self.critic, self.Q1, qacts, np.full_like(q, -1.0 / q.shape[0]), need_dx=True)[0][:, obs.shape[1]:]
            g = _backward(self.actor, self.names, pacts, da, out_tanh=True)[1]
            self.actor_opt.step(self.actor, _clip_grad_norm({k: g[k] for k in self.actor}))
            _soft_update(self.critic_t, self.critic, h["tau"])
            _soft_update(self.actor_t, self.actor, h["tau"])
        return closs, aloss


def _snapshot(actor, critic, actor_t, critic_t, actor_opt):
    cp = lambda p: {k: np.array(v, copy=True) for k, v in p.items()}
    return dict(actor=cp(actor), critic=cp(critic), actor_t=cp(actor_t), critic_t=cp(critic_t), actor_m=cp(actor_opt.m), actor_v=cp(actor_opt.v))


def _result(sp, stats, snaps, steps, extra):
    """stats: per call (critic loss, actor loss or None, [alpha loss, alpha])"""
    out = dict(critic_loss=np.array([s[0] for s in stats]), actor_loss=np.array([s[1] for s in stats if s[1] is not None]),
               calls=snaps, steps=steps, **extra)
    if sp["algo"] == "sac":
        out.update(alpha_loss=np.array([s[2] for s in stats]), alpha=np.array([s[3] for s in stats]))
    return out


def run_reference(sp, mutation=None):
    """The float64 reference on a spec: loss traces, alpha, every parameter set and the actor's Adam moments after every call, the
    Adam step counts, the smallest ReLU |pre-activation| seen and the per-call log (u of both passes; TD3's clipped noise and target action)."""
    r = Reference(sp, mutation)
    stats, snaps = [], []
    for k, idx in enumerate(sp["idx"]):
        stats.append(r.learn_sac(idx, sp["noise"][k][0], sp["noise"][k][1]) if r.sac else r.learn_td3(idx, sp["noise"][k][0]))
        snaps.append(_snapshot(r.actor, r.critic, r.actor_t, r.critic_t, r.actor_opt))
    return _result(sp, stats, snaps, (r.actor_opt.t, r.critic_opt.t), dict(kink=min(r.kink), log=r.log))


def run_oracle(sp):
    """The project's float32 oracle (oracle.algos.SAC / TD3) on the same spec, same result format."""
    from oracle import algos, nn
    h, tab = sp["hyper"], sp["table"]
    if sp["algo"] == "sac":
        o = algos.SAC(sp["actor"], sp["critic"], sp["O"], sp["A"], h["actor_lr"], h["critic_lr"], len(tab["rew"]), alpha0=h["alpha0"], alpha_lr=h["alpha_lr"])
        assert o.target_entropy == h["target_entropy"]
    else:
        o = algos.TD3(sp["actor"], sp["critic"], sp["O"], sp["A"], h["actor_lr"], h["critic_lr"], len(tab["rew"]))
    o.actor_t, o.critic_t = nn.copy_params(sp["actor_t"]), nn.copy_params(sp["critic_t"])
    for i in range(len(tab["rew"])):
        o.add(tab["obs"][i], tab["act"][i], float(tab["rew"][i]), tab["next_obs"][i], bool(tab["done"][i]))
    stats, snaps = [], []
    for k, idx in enumerate(sp["idx"]):
        if sp["algo"] == "sac":
            cl, al, ll = o.learn_with(idx, sp["noise"][k][0], sp["noise"][k][1], h["gamma"], h["tau"])
            stats.append((float(cl), float(al), float(ll), float(o.alpha)))
        else:
            cl, al = o.learn_with(idx, sp["noise"][k][0], h["gamma"], h["tau"], h["policy_noise"], h["noise_clip"], h["max_action"], h["policy_freq"],
                                  h["policy_noise_scale"])
            stats.append((float(cl), None if al is None else float(al)))
        snaps.append(_snapshot(o.actor, o.critic, o.actor_t, o.critic_t, o.actor_opt))
    return _result(sp, stats, snaps, (o.actor_opt.t, o.critic_opt.t), {})


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """run_reference of a case, once per process.  Cached: do not write into it."""
    return run_reference(spec(name))


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    return run_oracle(spec(name))


# ------------------------------------------------------------------------------------------------ comparisons
def share(got, want, rtol, atol=0.0):
    """max |got - want| / (atol + rtol |want|): the part of the tolerance used; <= 1 is what assert_allclose(got, want, rtol, atol) asks."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not got.size:
        return 0.0
    bound = atol + rtol * np.abs(want)
    err = np.abs(got - want)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)).max())


def shares(got, want, every_call=True):
    """(losses, alpha, parameters): the largest share of its tolerance any loss, alpha and parameter of `got` uses against `want`."""
    loss = max(share(got["critic_loss"], want["critic_loss"], LOSS_RTOL), share(got["actor_loss"], want["actor_loss"], LOSS_RTOL, ACTOR_LOSS_ATOL))
    alpha = 0.0
    if "alpha" in want:
        loss = max(loss, share(got["alpha_loss"], want["alpha_loss"], LOSS_RTOL))
        alpha = share(got["alpha"], want["alpha"], ALPHA_RTOL)
    param = 0.0
    for k in (range(len(want["calls"])) if every_call else [len(want["calls"]) - 1]):
        for net in ("actor", "critic", "actor_t", "critic_t"):
            param = max([param] + [share(got["calls"][k][net][n], w, P_RTOL, P_ATOL) for n, w in want["calls"][k][net].items()])
    return loss, alpha, param


def gate_columns(name):
    """(closed, on_bound): bool masks over the online log_std's columns — raw value outside [-20, 2]; exactly -20 or 2."""
    raw = spec(name)["actor"]["log_std"].reshape(-1)
    return (raw < LS_MIN) | (raw > LS_MAX), (raw == F32(LS_MIN)) | (raw == F32(LS_MAX))


def assert_conditions(c):
    """The conditions on a case's inputs (module docstring), from the float64 reference and the float32 oracle alone."""
    name, sp = c["name"], spec(c["name"])
    ref, orc = reference_run(name), oracle_run(name)
    n = c["n_calls"]
    assert len(sp["idx"]) == n == len(ref["calls"]) == len(orc["calls"]) and len(sp["idx"][0]) == c["batch"] <= BATCH_MAX, name
    assert ref["steps"] == orc["steps"] == ((n, n) if c["algo"] == "sac" else (n // POLICY_FREQ, n)), (name, ref["steps"], orc["steps"])
    for idx in sp["idx"]:
        assert sp["table"]["done"][idx].sum() >= 2 and len(set(idx.tolist())) == len(idx), name
    used = shares(orc, ref)
    assert max(used) <= ORACLE_SHARE, "%s: the float32 oracle uses %.2f / %.2f / %.2f of the loss / alpha / parameter tolerance against float64: choose another seed or gain" % ((name,) + used)
    assert ref["kink"] > KINK, "%s: a ReLU pre-activation at %.1e: choose another seed" % (name, ref["kink"])
    obs = act_inputs(name)[0]
    for label, eps, target, tol in act_checks(c):
        used_act = share(act_oracle(name, obs, eps, target), act_reference(name, obs, eps, target), **tol)
        assert used_act <= ORACLE_SHARE, "%s act %s: the float32 oracle uses %.2f of the tolerance" % (name, label, used_act)
    if c["algo"] == "td3":
        h = sp["hyper"]
        for k, lg in enumerate(ref["log"]):
            hi, lo = (lg["noise"] == h["noise_clip"]).mean(), (lg["noise"] == -h["noise_clip"]).mean()
            assert hi + lo >= 0.25 and min(hi, lo) >= 0.05, "%s call %d: %.0f %% / %.0f %% of the noise at +- noise_clip" % (name, k, 100 * hi, 100 * lo)
            hi, lo = (lg["a_next"] == 1.0).mean(), (lg["a_next"] == -1.0).mean()
            assert 0.10 <= hi + lo <= 0.50 and min(hi, lo) >= 0.05, "%s call %d: %.0f %% / %.0f %% of the target actions at +- max_action" % (name, k, 100 * hi, 100 * lo)
        return
    closed, on_bound = gate_columns(name)
    lay = c["layout"]
    assert closed.sum() == sum(1 for col, v in LAYOUTS.get(lay, {}).items() if col < c["A"] and not LS_MIN <= v <= LS_MAX), name
    assert on_bound.sum() == sum(1 for col, v in LAYOUTS.get(lay, {}).items() if col < c["A"] and v in (LS_MIN, LS_MAX)), name
    raw = sp["actor"]["log_std"].astype(F64)
    for k, call in enumerate(ref["calls"]):
        ls = call["actor"]["log_std"]          # (the online copy: the gate is the discontinuity; the target copy is only clamped, which is continuous)
        assert np.minimum(np.abs(ls - LS_MIN), np.abs(ls - LS_MAX)).min() > 1e-5, "%s call %d: an online log_std within 1e-5 of a bound" % (name, k)
        np.testing.assert_array_equal(call["actor"]["log_std"].reshape(-1)[closed], raw.reshape(-1)[closed])       # the reference's own gate
    step = np.abs(ref["calls"][0]["actor"]["log_std"] - raw).reshape(-1)[on_bound]
    assert ((step >= 0.5 * LR) & (step <= 1.5 * LR)).all(), "%s: columns on a bound moved by %r in the first call" % (name, step)
    zero = (np.clip(raw, LS_MIN, LS_MAX) == LS_MIN) | (np.clip(sp["actor_t"]["log_std"].astype(F64), LS_MIN, LS_MAX) == LS_MIN)
    for call in sp["noise"]:
        for nz in call:
            assert not nz[:, zero.reshape(-1)].any() and np.abs(nz[:, ~zero.reshape(-1)]).min() > 0, name
    if lay == "satmean":
        for k, lg in enumerate(ref["log"]):
            for which in ("u_target", "u_online"):
                hi, lo = (lg[which] > 10).mean(), (lg[which] < -10).mean()
                assert min(hi, lo) >= 0.10, "%s call %d %s: %.0f %% / %.0f %% of the entries past +- 10" % (name, k, which, 100 * hi, 100 * lo)
                assert (np.abs(np.tanh(lg[which][np.abs(lg[which]) > 10]).astype(F32)) == 1).all(), name


ACT_ROWS = 17                                      # one 16-row tile and one row
ACT_SAMPLE_TOL = dict(rtol=5e-4, atol=5e-5)        # test_sac_learn's select_action tolerance
ACT_TANH_TOL = dict(rtol=1e-5, atol=1e-6)          # test_ddpg_learn's / test_sac_learn's evaluate_action tolerance


def act_inputs(name):
    """(obs [17, O], eps [17, A]) of the forward checks, from the case's act_seed (eps is not zeroed anywhere: at sd = 2e-9 the sample is
    the mean to rounding, which tanh's tolerance absorbs).  The seed is chosen like the case's own: a head scaled by SAT_GAIN or
    TD3_GAIN carries the float32 rounding of its pre-activation times the gain, and tanh's tolerance of 1e-6 + 1e-5 |x| has to hold
    four times over on every entry that is not saturated."""
    c = BY_NAME[name]
    return synth.normal(66000 + 10 * c["act_seed"], (ACT_ROWS, c["O"])), synth.normal(66001 + 10 * c["act_seed"], (ACT_ROWS, c["A"]))


def act_oracle(name, obs, eps=None, target=False):
    """act_reference in the float32 oracle's arithmetic."""
    from oracle import algos, nn
    sp = spec(name)
    p = sp["actor_t" if target else "actor"]
    if sp["algo"] == "sac":
        return algos.GaussianActor().forward(p, nn.f32(obs), None if eps is None else nn.f32(eps))[0]
    return nn.MLP(ACTOR_NAMES["td3"], out_act="tanh").forward(p, nn.f32(obs))[0]


def act_checks(c):
    """The forward checks of a case: (label, eps or None, target copy, tolerance).  SAC: the stochastic sample of the online actor and
    tanh(mean); TD3: the online head and the target head (the one the gain saturates)."""
    obs, eps = act_inputs(c["name"])
    if c["algo"] == "sac":
        return [("sample", eps, False, ACT_SAMPLE_TOL), ("tanh-mean", None, False, ACT_TANH_TOL)]
    return [("tanh-online", None, False, ACT_TANH_TOL), ("tanh-target", None, True, ACT_TANH_TOL)]


def act_reference(name, obs, eps=None, target=False):
    """tanh(mean + exp(clamp(log_std)) eps) (SAC, eps given) or tanh(head) of the initial online / target actor, in float64."""
    sp = spec(name)
    p = _f64(sp["actor_t" if target else "actor"])
    head = _forward(p, ACTOR_NAMES[sp["algo"]], np.asarray(obs, F64), [])[0]
    if eps is not None:
        head = head + np.exp(np.clip(p["log_std"], LS_MIN, LS_MAX)) * np.asarray(eps, F64)
    return np.tanh(head)
