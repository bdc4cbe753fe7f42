"""NumPy restatement of MAPPO_file/MAPPO_for_mask_action.py: `learn` (:299-387), CategoricalMasked (:191-215) and the masked sample
of `select_action` (:256-259), in float32 where torch is.  Nets, LayerNorm, GAE, the critic step, digests and the comparison rules
are tests/mappo_oracle.py's.  Test infrastructure: the seeded cases and the toy environment below are what
tests/golden/make_mappo_mask_golden.py runs the imported reference on, what tests/test_mappo_mask_oracle.py checks this file against
and what tests/test_gpu_mappo_mask.py runs the kernels on.

Kept as the reference has it (DESIGN.md "MAPPO_for_mask_action"): learn() reads the whole capacity in ONE minibatch per epoch whatever
was added (rows never written are zeros with an all-closed mask; rows of earlier episodes stay); logits' = where(mask, logits, -1e8)
normalised as l = logits' - (max + log sum exp(logits' - max)), which makes every l of an all-closed row exactly 0; the log-prob is
not clamped; entropy and gradient are zero in a closed action; two Adams per agent behind clip_grad_norm_(..., 0.5).
"""
import numpy as np

from oracle import nn
from oracle.nn import F32, Adam
from tests import mappo_oracle as mo

CLOSED = F32(-1e8)
DIMS = ((5, 4), (4, 3), (5, 6))          # (obs, actions) per agent: unequal, so that a wrong block offset shows


def _case(cont, tricks, **kw):
    # horizon 40 in one minibatch: several row chunks with a short last one
    c = dict(kind="mappo", cont=cont, trick=dict(mo.TRICKS_ON if tricks else mo.TRICKS_OFF), dims=DIMS, hidden=32, horizon=40, minibatch=40,
             k_epochs=2, huber_delta=10.0, reward_scale=1.0, reward_same=False, dead_agent=None, seed=0, fill=None, second=0, edges=False)
    c.update(mo.HYPER)
    c.update(kw)
    c["minibatch"] = c["horizon"]
    return c


CASES = {
    "plain": _case(False, False, seed=61),
    # Huber delta 0.5 against rewards scaled so that the first critic step's errors straddle it (the maker checks >= 10 % on each side)
    "tricks": _case(False, True, huber_delta=0.5, reward_scale=0.25, reward_same=True, seed=62),
    # 13 rows never written: zeros, all-closed masks.  adv_norm is on so that those rows carry advantages of the others' size (raw,
    # they are a discounted V(0) (gamma - 1) and move the loss by under 1e-3): the normalisation order then decides the loss
    "partial": _case(False, False, trick=dict(mo.TRICKS_OFF, adv_norm=True), fill=27, seed=63),
    "stale": _case(False, True, second=18, seed=64),               # learn, 18 new rows over the old ones, learn again
    "edges": _case(False, False, edges=True, seed=65),             # rows with exactly one open action, rows with all open
    "wide": _case(False, True, dims=((18, 11),) * 3, hidden=128, horizon=64, k_epochs=1, seed=66),
    "cont": _case(True, True, seed=67),                            # masks stored and never read
}
FULL_CASES = ("plain", "tricks", "partial", "stale", "edges", "cont")


def case(name):
    return dict(CASES[name], name=name)


def masks(c, rows, seed):
    """[n][T][A] bool.  Outside `edges` 70 % of the rows have between 2 and A-1 open actions, the rest one or all; in `edges` half have
    exactly one and half have all.  The stored action is always open (discrete cases)."""
    rng = np.random.Generator(np.random.PCG64(seed + 7000))
    out = []
    for (O, A), r in zip(c["dims"], rows):
        T = r["obs"].shape[0]
        m = np.zeros((T, A), bool)
        for t in range(T):
            u = rng.random()
            if c["edges"]:
                k = 1 if t % 2 == 0 else A
            else:
                k = int(rng.integers(2, A)) if u < 0.7 else (1 if u < 0.85 else A)
            order = rng.permutation(A)
            if not c["cont"]:
                a = int(r["act"][t, 0])
                order = np.concatenate([[a], order[order != a]])
            m[t, order[:k]] = True
        out.append(m)
    return out


def inputs(c, seed=None):
    """mappo_oracle.inputs plus a `mask` [T][A] per agent"""
    seed = c["seed"] if seed is None else seed
    inp = mo.inputs(c, seed=seed)
    for r, m in zip(inp["rows"], masks(c, inp["rows"], seed)):
        r["mask"] = m
    return inp


def calls(c):
    """learn() calls of a case"""
    return 2 if c["second"] else 1


def perms(c):
    """[calls][n_agents][k_epochs][horizon]: np.random.permutation after np.random.seed(case seed + 1000), in learn()'s order"""
    st = np.random.RandomState(c["seed"] + 1000)
    return np.stack([np.stack([np.stack([st.permutation(c["horizon"]) for _ in range(c["k_epochs"])]) for _ in c["dims"]]) for _ in range(calls(c))])


def ring(c, inp):
    """what the buffers hold at the first learn(): the first `fill` rows as added, zeros behind them"""
    fill = c["horizon"] if c["fill"] is None else c["fill"]
    rows = []
    for r in inp["rows"]:
        z = {k: np.zeros_like(v) for k, v in r.items()}
        for k in r:
            z[k][:fill] = r[k][:fill]
        rows.append(z)
    return rows


def second_rows(c):
    """the `second` rows added after the first learn() (they land on rows 0 .. second-1: clear() reset the cursor)"""
    inp = inputs(c, seed=c["seed"] + 500)
    return [{k: v[:c["second"]] for k, v in r.items()} for r in inp["rows"]]


# ------------------------------------------------------------------------------------------------ CategoricalMasked
def masked_logits(z, mask, torch_order=True):
    """the normalised logits of Categorical(logits = where(mask, z, -1e8)); torch_order=False: (z' - max) - log sum, the order that an
    all-closed row tells apart (-log A instead of 0)"""
    zz = np.where(mask, z, CLOSED).astype(F32)
    mx = zz.max(axis=1, keepdims=True)
    ls = np.log(np.exp(zz - mx).sum(axis=1, keepdims=True, dtype=F32)).astype(F32)
    if torch_order:
        return (zz - (mx + ls).astype(F32)).astype(F32)
    return ((zz - mx).astype(F32) - ls).astype(F32)


def masked_dist(z, mask, torch_order=True):
    """-> (l, p, entropy [m, 1])"""
    l = masked_logits(z, mask, torch_order)
    p = mo.softmax(l)
    ent = -np.where(mask, l * p, F32(0)).sum(axis=1, keepdims=True, dtype=F32)
    return l, p, ent.astype(F32)


def sample(logits, mask, q):
    """CategoricalMasked(logits, masks).sample() with torch's Exp(1) draws q: -> (action, log-prob, relative margin of the winner)"""
    l, p, _ = masked_dist(np.asarray(logits, F32), np.asarray(mask, bool))
    v = p / np.asarray(q, F32)
    a = np.argmax(v, axis=1)
    top = np.sort(v, axis=1)[:, -2:]
    return a, l[np.arange(len(a)), a], (top[:, 1] - top[:, 0]) / top[:, 1]


# ------------------------------------------------------------------------------------------------ learn
class Oracle(mo.Oracle):
    def __init__(self, c, inp):
        super().__init__(c, inp)
        self.rows = ring(c, inp)
        # two Adams per agent, eps 1e-5 with trick['adam_eps'], both lrs read, clip_grad_norm_ 0.5 (:165-182)
        self.adam_eps = 1e-5 if self.trick["adam_eps"] else 1e-8
        self.critic_lr, self.clip_norm = c["critic_lr"], 0.5
        self.aopt = [Adam(p, c["actor_lr"], eps=self.adam_eps) for p in self.actors]
        self.copt = [Adam(p, c["critic_lr"], eps=self.adam_eps) for p in self.critics]
        self.torch_order = True
        self.first_actor_loss = None

    def add(self, new_rows):
        for r, nr in zip(self.rows, new_rows):
            for k, v in nr.items():
                r[k][:len(v)] = v

    def actor_step(self, i, ix, A):
        c, r, p = self.c, self.rows[i], self.actors[i]
        if c["cont"]:
            return super().actor_step(i, ix, A)
        m, ent_coef, clip = len(ix), c["ent_coef"], c["clip"]
        z, cache = mo.forward(p, mo.ACTOR_D, r["obs"][ix], self.trick)
        mask = r["mask"][ix].astype(bool)
        l, pr, ent = masked_dist(z, mask, self.torch_order)
        a = r["act"][ix].astype(np.int64).reshape(-1)
        lp = l[np.arange(m), a].reshape(-1, 1)
        ratio = np.exp(lp - r["logp"][ix].sum(axis=1, keepdims=True)).astype(F32)
        surr1 = ratio * A
        surr2 = np.clip(ratio, 1 - clip, 1 + clip).astype(F32) * A
        loss = F32(-np.mean(np.minimum(surr1, surr2), dtype=F32) - F32(ent_coef) * np.mean(ent, dtype=F32))
        if self.first_actor_loss is None:
            self.first_actor_loss = float(loss)
        dlp = (np.where(surr1 <= surr2, A, F32(0)).sum(axis=1, keepdims=True) * F32(-1.0 / A.size) * ratio).astype(F32)
        onehot = np.zeros_like(pr)
        onehot[np.arange(m), a] = 1
        dz = np.where(mask, dlp * (onehot - pr) + F32(ent_coef / m) * pr * (l + ent), F32(0)).astype(F32)
        g = mo.backward(p, mo.ACTOR_D, cache, dz)
        g = {k: g[k] for k in p}
        nn.clip_grad_norm(g, self.clip_norm)
        self.aopt[i].step(p, g)
        return loss


def run(c, inp=None, perm=None, torch_order=True, calls_max=None):
    """-> the oracle after the case's learn() calls; o.trace [n][calls * K][2], o.adv_raw / o.v_target of the LAST call"""
    inp = inputs(c) if inp is None else inp
    perm = perms(c) if perm is None else perm
    o = Oracle(c, inp)
    o.torch_order = torch_order
    traces = [o.learn(perm[0])]
    if c["second"] and (calls_max is None or calls_max > 1):
        o.add(second_rows(c))
        traces.append(o.learn(perm[1]))
    o.trace = np.concatenate(traces, axis=1)
    return o


# ------------------------------------------------------------------------------------------------ the episode run
# A seeded toy environment for the CLASS (the script's loop needs smacv2): four episodes of 13, 9, 16 and 5 steps at horizon 16 with a
# learn() after each: a partly filled ring, a stale tail, an exactly full ring, a short episode.  Observations are a function of the
# step alone (an action cannot steer the run), masks of (step, agent) with the last action always open, rewards a table lookup on the
# action.
LOOP = _case(False, True, horizon=16, seed=71)
LOOP_EPISODES = (13, 9, 16, 5)
LOOP_HYPER = dict(gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, k_epochs=2, huber_delta=10.0)


class ToyEnv:
    def __init__(self, c=LOOP, seed=None):
        rng = np.random.Generator(np.random.PCG64((c["seed"] if seed is None else seed) + 9000))
        steps = sum(LOOP_EPISODES) + 1
        self.agents = ["agent_%d" % i for i in range(len(c["dims"]))]
        self.obs = [rng.normal(0, 1, (steps, O)).astype(F32) for O, _ in c["dims"]]
        self.mask = []
        for _, A in c["dims"]:
            m = rng.random((steps, A)) < 0.5
            m[:, A - 1] = True
            self.mask.append(m)
        self.reward = [rng.normal(0, 1, A).astype(F32) for _, A in c["dims"]]
        self.t = 0

    def observe(self):
        return ({a: self.obs[i][self.t] for i, a in enumerate(self.agents)}, {a: self.mask[i][self.t] for i, a in enumerate(self.agents)})

    def step(self, action, last):
        rew = {a: float(self.reward[i][int(action[a])]) for i, a in enumerate(self.agents)}
        self.t += 1
        nobs = {a: self.obs[i][self.t] for i, a in enumerate(self.agents)}
        done = {a: bool(last) for a in self.agents}
        return nobs, rew, done


def run_loop(algo, env, on_step=None):
    """drives an object with the reference class's surface through the four episodes; -> (actions [steps][n], log-probs [steps][n])"""
    acts, lps = [], []
    for ep_len in LOOP_EPISODES:
        for s in range(ep_len):
            obs, avail = env.observe()
            if on_step is not None:
                on_step(obs, avail)
            action, logp = algo.select_action(obs, avail)
            nobs, rew, done = env.step(action, s == ep_len - 1)
            algo.add(obs, action, rew, nobs, done, logp, done, avail)
            acts.append([int(np.asarray(action[a]).reshape(-1)[0]) for a in env.agents])
            lps.append([float(np.asarray(logp[a]).reshape(-1)[0]) for a in env.agents])
        algo.learn(LOOP["horizon"], LOOP_HYPER["gamma"], LOOP_HYPER["lmbda"], LOOP_HYPER["clip"], LOOP_HYPER["k_epochs"], LOOP_HYPER["ent_coef"],
                   LOOP_HYPER["huber_delta"])
    return np.array(acts, np.int64), np.array(lps, np.float64)
