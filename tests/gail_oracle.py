"""GAIL's discriminator (GAIL_file/GAIL.py:17-120) restated in NumPy, and the seeded inputs of its golden cases.  The golden
generator (tests/golden/make_gail_golden.py) runs the reference on exactly these inputs; the CPU test holds this oracle to its
output and the GPU test holds the HIP engine to both.

The net is mlp(s_dim + a_dim, [H, H], 1) with LeakyReLU(0.01) (or ReLU) and a linear head; x = [s | a], l = the logit.
    gp_coef == 0:  p = sigmoid(l); d_loss = BCE(p_e, 1) + BCE(p_p, 0) with torch's clamps (log at -100; the backward divides by
                   max(p (1 - p), 1e-12)); Adam betas (0.9, 0.999)
    gp_coef > 0:   d_loss = 0.5 (mean_e softplus(-l) + mean_p softplus(l)) + 5 mean_e ||dl/dx||^2 (the literal 5, expert rows
                   only); Adam betas (0.5, 0.9)
The penalty's gradient is taken in closed form (the second derivative of a piecewise-linear activation is zero): with m1, m2 a
row's slopes, u2 = m2 w3, u1 = m1 (W2^T u2), g = W1^T u1, t0 = 2 c g / E, s1 = m1 (W1 t0), s2 = m2 (W2 s1):
    dW1 += u1 (x) t0, dW2 += u2 (x) s1, dw3 += s2, biases nothing.
tests/test_gail_oracle.py holds that to torch.autograd.grad(create_graph=True) in float64.

`dtype` is the arithmetic's precision (float64: the reference for tolerances; float32: what two fp32 implementations may differ
by).  `p32=True` rounds the sigmoid through float32 as torch does (1 / (1 + exp(-l)) is exactly 1 from l = 17 and exactly 0 below
l = -89), which is what decides where the BCE clamps act.
"""
import math

import numpy as np

from tests.golden import synth

F32 = np.float32
NAMES = ["backbone.0", "backbone.1", "backbone.2"]
SLOPES = {"LeakyReLU": 0.01, "ReLU": 0.0}
GP_WEIGHT = 5.0           # GAIL.py:98, not config['D']['gp_coef']

# the golden cases: both modes at O 3, A 1, H 32, E 37, N 29, three calls; a fixed probe batch for compute_reward
CASES = {
    "bce": dict(gp_coef=0.0, seed=11100),
    "gp": dict(gp_coef=10.0, seed=11200),
}
COMMON = dict(s_dim=3, a_dim=1, hidden=32, n_expert=37, n_policy=29, n_table=120, n_learn=3, n_probe=16, d_lr=4e-4,
              activation="LeakyReLU")
# the class case: freerl_amd.GAIL.GAIL's host side (seeded init, ExpertDataset scaling, torch.randint draws) in the default (gp) mode
CLASS = dict(gp_coef=10.0, seed=11900, n_table=50, n_expert=24, n_policy=24, n_learn=3)


def case(name):
    c = dict(COMMON)
    c.update(CLASS if name == "class" else CASES[name])
    return c


def betas(gp_coef):
    return (0.5, 0.9) if gp_coef > 0 else (0.9, 0.999)


def layers(in_dim, hidden):
    return [(NAMES[0], hidden, in_dim), (NAMES[1], hidden, hidden), (NAMES[2], 1, hidden)]


def config(c):
    """The reference's config dict (GAIL_file/config.py) for a case."""
    return dict(seed=c["seed"], use_gpu=False, s_dim=c["s_dim"], a_dim=c["a_dim"], algo="GAIL",
                D=dict(d_mlp_dim=c["hidden"], activation=c["activation"], dropout=0.0, layernorm=False, d_lr=c["d_lr"], gp_coef=c["gp_coef"]))


def inputs(c, n_learn=None, seed=None, in_dim=None):
    """The net's parameters (PCG64), the expert table [n_table, in_dim] in [-1, 1], every call's expert rows (drawn WITH
    replacement) and policy rows, and the probe batch."""
    s = c["seed"] if seed is None else seed
    calls = c["n_learn"] if n_learn is None else n_learn
    d = c["s_dim"] + c["a_dim"] if in_dim is None else in_dim
    g = np.random.default_rng(s + 1)
    return dict(net=synth.mlp_params(s, layers(d, c["hidden"])),
                expert=g.uniform(-1, 1, (c["n_table"], d)).astype(F32),
                idx=[g.integers(0, c["n_table"], c["n_expert"]).astype(np.int64) for _ in range(calls)],
                policy=[(0.8 * g.standard_normal((c["n_policy"], d))).astype(F32) for _ in range(calls)],
                probe=(0.8 * g.standard_normal((c["n_probe"], d))).astype(F32) if "n_probe" in c else None)


def raw_expert(c, seed):
    """Unscaled expert arrays of the class case: every column gets its own offset and range, so the scaling matters."""
    g = np.random.default_rng(seed + 5)
    n = c["n_table"]
    states = (g.standard_normal((n, c["s_dim"])) * np.array([1.0, 3.0, 0.5])[:c["s_dim"]] + np.array([0.0, -2.0, 4.0])[:c["s_dim"]])
    actions = g.uniform(-2.0, 2.0, (n, c["a_dim"]))
    return states.astype(np.float64), actions.astype(np.float64)


def minmax_scale(x):
    """ExpertDataset (GAIL_utils.py:16-32): per column to [-1, 1]."""
    lo, hi = x.min(axis=0), x.max(axis=0)
    return 2 * (x - lo) / (hi - lo) - 1, lo, hi


class Adam:
    """torch.optim.Adam, single-tensor order (oracle/nn.py's Adam) with the betas given, in the oracle's dtype."""

    def __init__(self, params, lr, betas, eps=1e-8):
        self.lr, self.eps, (self.b1, self.b2) = float(lr), float(eps), betas
        self.t = 0
        self.m = {k: np.zeros_like(v) for k, v in params.items()}
        self.v = {k: np.zeros_like(v) for k, v in params.items()}

    def step(self, params, grads):
        self.t += 1
        dt = next(iter(params.values())).dtype.type
        bc1, bc2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for k in params:
            g, m, v = grads[k], self.m[k], self.v[k]
            m += (g - m) * dt(1.0 - self.b1)
            v *= dt(self.b2)
            v += dt(1.0 - self.b2) * g * g
            params[k] -= dt(self.lr / bc1) * (m / (np.sqrt(v) / dt(math.sqrt(bc2)) + dt(self.eps)))


class Discriminator:
    def __init__(self, net, d_lr, gp_coef, activation="LeakyReLU", dtype=np.float64, p32=False):
        self.dt, self.gp, self.p32 = dtype, gp_coef > 0, p32
        self.slope = dtype(SLOPES[activation])
        self.p = {k: np.array(v, dtype=dtype) for k, v in net.items()}
        self.opt = Adam(self.p, d_lr, betas(gp_coef))
        self.penalty = self.norm = 0.0

    # ---- forward: logits and what the backward needs
    def forward(self, x):
        x = np.asarray(x, self.dt)
        W1, b1, W2, b2, W3, b3 = (self.p[n + s] for n in NAMES for s in (".weight", ".bias"))
        z1 = x @ W1.T + b1
        h1 = np.where(z1 > 0, z1, self.slope * z1)
        z2 = h1 @ W2.T + b2
        h2 = np.where(z2 > 0, z2, self.slope * z2)
        l = (h2 @ W3.T + b3)[:, 0]
        one = self.dt(1)
        return l, (x, h1, h2, np.where(h1 > 0, one, self.slope), np.where(h2 > 0, one, self.slope))

    def sigmoid(self, l):
        with np.errstate(over="ignore"):
            if self.p32:
                l32 = l.astype(F32)
                return (F32(1) / (F32(1) + np.exp(-l32))).astype(self.dt)
            return self.dt(1) / (self.dt(1) + np.exp(-l))

    def _backward(self, cache, dl):
        """First-order backward of sum_r dl[r] l[r] -> grads."""
        x, h1, h2, m1, m2 = cache
        W2, W3 = self.p[NAMES[1] + ".weight"], self.p[NAMES[2] + ".weight"]
        d3 = dl[:, None]
        d2 = (d3 @ W3) * m2
        d1 = (d2 @ W2) * m1
        return {NAMES[2] + ".weight": d3.T @ h2, NAMES[2] + ".bias": d3.sum(axis=0), NAMES[1] + ".weight": d2.T @ h1,
                NAMES[1] + ".bias": d2.sum(axis=0), NAMES[0] + ".weight": d1.T @ x, NAMES[0] + ".bias": d1.sum(axis=0)}

    def input_grad(self, cache):
        """g = dl/dx per row, with u1, u2."""
        _, _, _, m1, m2 = cache
        W1, W2, W3 = (self.p[n + ".weight"] for n in NAMES)
        u2 = m2 * W3[0]
        u1 = m1 * (u2 @ W2)
        return u1 @ W1, u1, u2

    def penalty_grads(self, cache, c):
        """c mean_e ||g||^2 and its gradient, closed form."""
        _, _, _, m1, m2 = cache
        W1, W2 = self.p[NAMES[0] + ".weight"], self.p[NAMES[1] + ".weight"]
        g, u1, u2 = self.input_grad(cache)
        E = g.shape[0]
        pen = np.sum(g * g, dtype=self.dt) / self.dt(E)
        t0 = self.dt(2) * self.dt(c) * g / self.dt(E)
        s1 = m1 * (t0 @ W1.T)
        s2 = m2 * (s1 @ W2.T)
        return pen, {NAMES[0] + ".weight": u1.T @ t0, NAMES[1] + ".weight": u2.T @ s1, NAMES[2] + ".weight": s2.sum(axis=0)[None, :]}

    def loss_and_grads(self, xe, xp):
        """-> ((d_loss, expert_prob, policy_prob, w_dis), grads); self.penalty = the penalty mean."""
        dt = self.dt
        le, ce = self.forward(xe)
        lp, cp = self.forward(xp)
        E, N = dt(len(le)), dt(len(lp))
        pe, pp = self.sigmoid(le), self.sigmoid(lp)
        if self.gp:
            sp = lambda v: np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v)))
            loss = dt(0.5) * (sp(-le).mean(dtype=dt) + sp(lp).mean(dtype=dt))
            grads = self._backward(ce, dt(0.5) * (pe - 1) / E)
            gp_ = self._backward(cp, dt(0.5) * pp / N)
            pen, pg = self.penalty_grads(ce, GP_WEIGHT)
            loss = loss + dt(GP_WEIGHT) * pen
            for k in grads:
                grads[k] = grads[k] + gp_[k] + (pg[k] if k in pg else 0)
            self.penalty = float(pen)
            out = (float(loss), float(pe.mean(dtype=dt)), float(pp.mean(dtype=dt)), float(le.mean(dtype=dt) - lp.mean(dtype=dt)))
        else:
            with np.errstate(divide="ignore"):
                loss = -np.maximum(np.log(pe), -100).mean(dtype=dt) - np.maximum(np.log(1 - pp), -100).mean(dtype=dt)
            qe, qp = (1 - pe) * pe, (1 - pp) * pp
            grads = self._backward(ce, ((pe - 1) / E / np.maximum(qe, dt(1e-12))) * qe)
            gp_ = self._backward(cp, (pp / N / np.maximum(qp, dt(1e-12))) * qp)
            for k in grads:
                grads[k] = grads[k] + gp_[k]
            self.penalty = 0.0
            out = (float(loss), float(pe.mean(dtype=dt)), float(pp.mean(dtype=dt)), 0.0)
        self.norm = float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in grads.values())))
        return out, grads

    def trian_D(self, xe, xp):
        out, grads = self.loss_and_grads(xe, xp)
        self.opt.step(self.p, grads)
        return out

    def compute_reward(self, x):
        l, _ = self.forward(x)
        dt = self.dt
        if self.gp:
            with np.errstate(over="ignore"):
                prob = dt(1) / (dt(1) + np.exp(-l))
            return -np.log(np.maximum(dt(1) - prob, dt(0.0001))) * dt(2)
        return -np.log(dt(1) - self.sigmoid(l) + dt(1e-8))


def make(c, inp, dtype=np.float64, activation=None, p32=False):
    return Discriminator(inp["net"], c["d_lr"], c["gp_coef"], activation or c["activation"], dtype, p32)
