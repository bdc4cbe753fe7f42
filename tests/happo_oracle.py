"""NumPy restatement of MAPPO_file/HAPPO.py:339-458 (`learn`), float32 where torch is, on tests/mappo_oracle.py's forward, backward and
Adam.  Test infrastructure: the seeded cases below are what tests/golden/make_happo_golden.py runs the imported reference on, what
tests/test_happo_oracle.py checks this file against, and what tests/test_gpu_happo.py runs the kernels on.

HAPPO is MAPPO's advantage half (every critic on the concatenated observation, adv_norm over the whole matrix, the surrogate's mean
over ratios [m, 1] x adv[index] [m, n], the critic on all n target columns, a ValueClip that changes nothing) with IPPO's two clipped
Adams per agent, and its own second half: the agents are visited in `order`; the k-th visited agent's surrogate rows are multiplied
by factor_k [T, 1], the product over the earlier visited agents of exp(new - old), their summed log-probabilities over the whole
horizon after and before their steps.  Deviation from the reference (DESIGN.md "HAPPO"): the discrete branch's `new` is taken over all
rows in time order, as the continuous branch's is, where HAPPO.py:449-450 indexes the loop's last minibatch.
"""
import numpy as np

from oracle import nn
from oracle.nn import F32, Adam
from oracle.ppo import F32_EPS, HALF_LOG_2PI, LOG_SQRT_2PI
from tests import mappo_oracle as mo

RC = 64          # the engine's row chunk at these widths (tests/test_gpu_happo.py asserts it)


def _case(cont, tricks, **kw):
    c = mo._case("happo", cont, tricks, order=None, ident=False, ref_raises=False)
    c.update(kw)
    return c


CASES = {
    "happo_c_plain": _case(True, False, seed=51),
    "happo_c_tricks": _case(True, True, seed=52),
    # the same inputs under two imposed visiting orders
    "happo_c_order_a": _case(True, False, seed=53, order=(2, 0, 1)),
    "happo_c_order_b": _case(True, False, seed=53, order=(1, 2, 0)),
    # both Huber branches: delta 0.5 against rewards scaled as in MAPPO's Huber cases
    "happo_c_huber": _case(True, False, trick=dict(mo.TRICKS_OFF, huber_loss=True), huber_delta=0.5, reward_scale=0.25, reward_same=True, seed=54),
    # l1.bias = -10 on agent 1: zero-variance LayerNorm rows inside the two horizon passes
    "happo_c_dead": _case(True, True, dead_agent=1, seed=55),
    # the horizon pass's second chunk has 6 rows; one minibatch of the same length, then minibatches of 32 that chunk differently
    "happo_c_chunk": _case(True, True, horizon=RC + 6, minibatch=RC + 6, k_epochs=1, seed=56),
    "happo_c_ragged": _case(True, True, horizon=RC + 6, minibatch=32, seed=57),
    # the scripts' widths
    "happo_c_wide": _case(True, True, dims=((18, 5),) * 3, hidden=128, horizon=64, minibatch=64, k_epochs=1, seed=58),
    # factors far from 1
    "happo_c_hot": _case(True, True, actor_lr=1e-2, critic_lr=1e-2, seed=59),
    # one agent: the factor code never runs
    "happo_d_single": _case(False, False, dims=((5, 3),), seed=60),
    # the one setting in which the reference's discrete branch equals the time-order form: one minibatch of T rows, identity permutations
    "happo_d_ident": _case(False, False, horizon=40, minibatch=40, ident=True, seed=61),
    # discrete with real minibatches: the reference raises RuntimeError (HAPPO.py:453); expected values from this file only
    "happo_d_plain": _case(False, False, ref_raises=True, seed=62),
    "happo_d_tricks": _case(False, True, ref_raises=True, seed=63),
}
# Tolerances are the project's (tests/test_gpu_mappo.py): losses rtol 1e-4 / atol 1e-6, which the factors take too (the loss is linear in
# them), parameters by mo.assert_net's (5e-4, 5e-6).  happo_c_hot alone (lr 1e-2, factors from 2e-3 to 7e2) takes per quantity the larger of
# those and 4 x the deviation of this oracle from the reference measured when the golden was recorded (profiles/happo/README.md): its
# loss trace deviates by 7.47e-5 in rtol units (|diff| / (atol / rtol + |reference|)), so 2.99e-4 / 2.99e-6; its factors (7.99e-6) and
# parameters (0.046 of the element rule) stay under a quarter of the project's, which therefore hold.  4 x covers a second, independent
# fp32 summation order
TOL = dict(trace=(1e-4, 1e-6), factor=(1e-4, 1e-6), param=(5e-4, 5e-6))
TOL_HOT = dict(TOL, trace=(2.99e-4, 2.99e-6))


def tol(name, what):
    return (TOL_HOT if name == "happo_c_hot" else TOL)[what]


FULL_CASES = tuple(k for k, c in CASES.items() if c["hidden"] <= 32 and not c["ref_raises"])


def case(name):
    return dict(CASES[name], name=name)


def joint(c):
    """the case as tests/mappo_oracle.py's functions want it: they decide 'global critic, all columns' by kind == 'mappo'"""
    return dict(c, kind="mappo")


def inputs(c, seed=None):
    return mo.inputs(joint(c), seed)


def perms(c, order, seed=None):
    """[n_agents][k_epochs][horizon] BY AGENT ID: np.random.permutation after np.random.seed(case seed + 1000), drawn in visiting order"""
    n, K, T = len(c["dims"]), c["k_epochs"], c["horizon"]
    out = np.zeros((n, K, T), np.int64)
    st = np.random.RandomState((c["seed"] if seed is None else seed) + 1000)
    for i in order:
        for k in range(K):
            out[i, k] = np.arange(T) if c["ident"] else st.permutation(T)
    return out


class Oracle(mo.Oracle):
    def __init__(self, c, inp):
        super().__init__(joint(c), inp)
        # two Adams per agent behind clip_grad_norm_(..., 0.5) (HAPPO.py:237-254)
        self.adam_eps, self.critic_lr, self.clip_norm = (1e-5 if self.trick["adam_eps"] else 1e-8), c["critic_lr"], 0.5
        self.aopt = [Adam(p, c["actor_lr"], eps=self.adam_eps) for p in self.actors]
        self.copt = [Adam(p, c["critic_lr"], eps=self.adam_eps) for p in self.critics]

    def _policy(self, i, ix):
        """rows ix of agent i through its actor -> what the step and the horizon pass both need"""
        c, r, p = self.c, self.rows[i], self.actors[i]
        z, cache = mo.forward(p, mo.actor_names(c), r["obs"][ix], self.trick)
        if c["cont"]:
            mean = np.tanh(z).astype(F32)
            log_std = np.clip(np.broadcast_to(p["log_std"], mean.shape), -20, 2).astype(F32)
            var = np.exp(log_std) ** 2
            a = r["act"][ix]
            lp = (-((a - mean) ** 2) / (F32(2) * var) - log_std - F32(LOG_SQRT_2PI)).sum(axis=1, keepdims=True)
            ent = (F32(0.5 + HALF_LOG_2PI) + log_std).sum(axis=1, keepdims=True)
            return lp.astype(F32), ent, cache, dict(mean=mean, var=var, a=a)
        pr = mo.softmax(z)
        logit = np.log(np.clip(pr / pr.sum(axis=1, keepdims=True, dtype=F32), F32_EPS, 1 - F32_EPS)).astype(F32)
        a = r["act"][ix].astype(np.int64).reshape(-1)
        lp = logit[np.arange(len(a)), a].reshape(-1, 1)
        ent = -(logit * pr).sum(axis=1, keepdims=True)
        return lp.astype(F32), ent, cache, dict(pr=pr, logit=logit, a=a)

    def horizon_logp(self, i):
        """sum_c log pi(a | o) over all T rows in time order, with the actor as it stands (HAPPO.py:382-391, :443-452)"""
        return self._policy(i, np.arange(self.c["horizon"]))[0]

    def actor_step(self, i, ix, A, f):
        """HAPPO.py:402-416: -(factor[idx] * min(surr1, surr2)).mean() - c_ent * entropy.mean(); f [m, 1]"""
        c, r, p = self.c, self.rows[i], self.actors[i]
        m, ent_coef, clip = len(ix), c["ent_coef"], c["clip"]
        lp, ent, cache, q = self._policy(i, ix)
        ratio = np.exp(lp - r["logp"][ix].sum(axis=1, keepdims=True)).astype(F32)
        surr1 = ratio * A
        surr2 = np.clip(ratio, 1 - clip, 1 + clip).astype(F32) * A
        loss = F32(-np.mean(f * np.minimum(surr1, surr2), dtype=F32) - F32(ent_coef) * np.mean(ent, dtype=F32))
        dlp = (f * np.where(surr1 <= surr2, A, F32(0)).sum(axis=1, keepdims=True) * F32(-1.0 / A.size) * ratio).astype(F32)
        if c["cont"]:
            mean, var, a, raw = q["mean"], q["var"], q["a"], p["log_std"]
            g = mo.backward(p, mo.actor_names(c), cache, (dlp * (a - mean) / var * (F32(1) - mean * mean)).astype(F32))
            inside = ((raw >= -20) & (raw <= 2)).astype(F32)
            g["log_std"] = ((dlp * ((a - mean) ** 2 / var - F32(1)) - F32(ent_coef / m)).sum(axis=0, keepdims=True) * inside).astype(F32)
        else:
            pr, logit, a = q["pr"], q["logit"], q["a"]
            onehot = np.zeros_like(pr)
            onehot[np.arange(m), a] = 1
            g = mo.backward(p, mo.actor_names(c), cache, (dlp * (onehot - pr) + F32(ent_coef / m) * pr * (logit + ent)).astype(F32))
        g = {k: g[k] for k in p}
        nn.clip_grad_norm(g, self.clip_norm)
        self.aopt[i].step(p, g)
        return loss

    def learn(self, order, perm):
        """order [n] the agent visited at each position, perm [n][K][T] by agent id -> trace [n][K * n_mb][2] by agent id; sets
        self.factors [n][T] by visiting position"""
        c, T, mb, n = self.c, self.c["horizon"], self.c["minibatch"], self.n
        self.gae()
        factor = np.ones((T, 1), F32)
        self.factors = [factor.reshape(-1)]
        trace = [None] * n
        for pos, i in enumerate(int(j) for j in order):
            if pos != n - 1:
                old = self.horizon_logp(i)
            tr = []
            for k in range(c["k_epochs"]):
                for s in range(0, T, mb):
                    ix = np.asarray(perm[i][k][s:s + mb])
                    tr.append((self.actor_step(i, ix, self.adv[ix], factor[ix]), self.critic_step(i, ix, self.v_target[ix])))
            trace[i] = tr
            if pos != n - 1:
                factor = (factor * np.exp(self.horizon_logp(i) - old)).astype(F32)
                self.factors.append(factor.reshape(-1))
        self.factors = np.stack(self.factors)
        return np.array(trace, F32)


def run(c, order, inp=None, perm=None):
    o = Oracle(c, inputs(c) if inp is None else inp)
    o.order = np.asarray(order, np.int64)
    o.trace = o.learn(o.order, perms(c, o.order) if perm is None else perm)
    return o
