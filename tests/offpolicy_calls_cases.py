"""The cases of tests/test_gpu_offpolicy_calls.py and of its fixture's maker (tests/golden/make_offpolicy_calls_golden.py): three
consecutive calls with device-drawn rows of every off-policy entry point, on an engine created with a fixed seed.

frl_learn: every row of tests/test_gpu_learn_launches.py's CASES, at those shapes and under those knobs (one case per kernel family and
per host decision: who draws, whether the policy step is folded, the pre-drawn multi-agent rows).  The five smaller entry points: one
call shape each, the smallest their own GPU tests use (tests/test_gpu_envelope.py, _envelope_ddpg.py, _gail.py, _cem_gd3pg.py,
_reinforce.py).  Nets are the engine's own initialisation, rows are synthetic under fixed seeds.

What a case yields: `idx` int32 [3][...], the rows each call trained on (REINFORCE draws none: absent); `out` float32, what the three
calls returned (statistics or losses); `digest` uint8 [32], SHA-256 over every net's parameters, targets and Adam moments after the
third call, learner by learner."""
import contextlib
import hashlib
import os

import numpy as np

from tests.test_gpu_learn_launches import CASES as LEARN_CASES, KNOBS

F32 = np.float32
SEED, OTHER_SEED = 7, 77
CALLS = 3
SMALL = ("envelope", "envelope_ddpg", "gail", "cem_gd3pg", "reinforce")
NAMES = ["learn_" + c[0] for c in LEARN_CASES] + list(SMALL)


@contextlib.contextmanager
def _knobs(env):
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _digest(N, e):
    h = hashlib.sha256()
    for p in range(e.P):
        for net in range(e.n_nets):
            for kind in (N.PARAM_ONLINE, N.PARAM_TARGET, N.PARAM_ADAM_M, N.PARAM_ADAM_V):
                h.update(e.get_params(net, kind, p).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def _rows(e, g, n, n_act=0):
    """n synthetic records: small normal columns, done on 1 row in 16, a valid action number where the action is discrete"""
    lay = e.layout
    rec = (g.standard_normal((n, e.width)) * 0.5).astype(F32)
    rec[:, lay.done_off] = g.random(n) < 1 / 16
    if n_act:
        rec[:, lay.act_off[0]] = g.integers(0, n_act, n)
    return rec


def _learn_case(N, name, seed):
    from freerl_amd.engine import Engine
    eng, env, kw = next(c[1:4] for c in LEARN_CASES if "learn_" + c[0] == name)
    B = eng["B"]
    with _knobs(env):
        e = Engine(getattr(N, "ALGO_" + eng["algo"]), eng["obs"], eng["act"], 1024, n_learners=eng["P"], twin_critic=eng.get("twin", False),
                   batch_max=B, hidden=eng.get("hidden", 128), discrete=eng.get("discrete", False), seed=seed)
        try:
            e.fill_synthetic(400, seed=3)
            idx, out = [], []
            for _ in range(CALLS):
                out.append(e.learn(B, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, want_stats=True, **kw))
                idx.append(e.last_indices(B))
            return dict(idx=np.stack(idx).astype(np.int32), out=np.stack(out).astype(F32), digest=_digest(N, e))
        finally:
            e.close()


def _small_case(N, name, seed):
    from freerl_amd.engine import Engine
    g = np.random.default_rng(11)
    idx, out = [], []
    if name == "envelope":
        e = Engine(N.ALGO_ENVELOPE_DQN, 4, 3, 40, discrete=True, hidden=32, batch_max=64, reward_dim=2, seed=seed)
    elif name == "envelope_ddpg":
        e = Engine(N.ALGO_ENVELOPE_DDPG, 4, 3, 40, hidden=32, batch_max=64, reward_dim=2, seed=seed)
    elif name == "gail":
        e = Engine(N.ALGO_GAIL, 3, 1, 40, hidden=32, hidden_act=N.ACT_LEAKY_RELU, batch_max=32, seed=seed)
    elif name == "cem_gd3pg":
        e = Engine(N.ALGO_CEM_GD3PG, 4, 3, 40, hidden=32, hidden_act=N.ACT_TANH, batch_max=16, seed=seed)
    else:
        e = Engine(N.ALGO_REINFORCE, 4, 64, 64, n_learners=2, discrete=True, seed=seed)
    try:
        if name in ("envelope", "envelope_ddpg", "gail"):
            e.add_batch(_rows(e, g, 40, 3 if name == "envelope" else 0))
        elif name == "cem_gd3pg":
            for ring in (0, 1):
                e.ring_add_batch(ring, _rows(e, g, 40), learners=np.zeros(40, np.int32))
        for k in range(CALLS):
            if name == "envelope":
                o = e.envelope_learn(16, 4, gamma=0.99, tau=0.01, lr=1e-3, beta=0.5, want_loss=True, want_weights=True)
                out.append(np.concatenate([o["loss"].ravel(), o["weights"].ravel()]))
                idx.append(e.last_indices(16))
            elif name == "envelope_ddpg":
                o = e.envelope_ddpg_learn(16, 4, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, beta=0.5, want_loss=True, want_weights=True)
                out.append(np.concatenate([o["critic_loss"].ravel(), o["actor_loss"].ravel(), o["weights"].ravel()]))
                idx.append(e.last_indices(16))
            elif name == "gail":
                o = e.gail_learn((g.standard_normal((1, 8, 4)) * 0.5).astype(F32), gp=True, lr=4e-4, beta1=0.5, beta2=0.9, n_expert=8, want_idx=True)
                out.append(o["out"].ravel())
                idx.append(o["idx"])
            elif name == "cem_gd3pg":
                out.append(e.cem_gd3pg_learn(16, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, f1_more=True, delta=0.3).ravel())
                idx.append(e.last_indices(16))
            else:                                              # (the call empties the rings: 40 and 17 fresh steps before each)
                lens = (40, 17)
                rec = np.concatenate([_rows(e, g, n, 64) for n in lens])
                e.add_batch(rec, learners=np.repeat(np.arange(2), lens).astype(np.int32))
                o = e.reinforce_learn(gamma=0.99, lr=1e-3, want_loss=True, want_returns=True)
                out.append(np.concatenate([o["loss"].ravel(), o["returns"][0, :40], o["returns"][1, :17]]))
        res = dict(out=np.stack(out).astype(F32), digest=_digest(N, e))
        if idx:
            res["idx"] = np.stack(idx).astype(np.int32)
        return res
    finally:
        e.close()


def run(N, name, seed=SEED):
    return (_learn_case if name.startswith("learn_") else _small_case)(N, name, seed)
