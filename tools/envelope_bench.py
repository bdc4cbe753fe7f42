"""learn() time of envelope multi-objective DQN (kernels_envelope.hip) at the reference script's shape:

  obs 2, 4 actions, 2 objectives, hidden 256, batch 256 x weight_num 128 = 32768 rows per call

`--ddpg`: envelope multi-objective DDPG (kernels_envelope_ddpg.hip, frl_envelope_ddpg_learn) at the same shape, the 4 a continuous
action's dimensions: a critic step and an actor step per call.

Per population P: rows and preference vectors drawn on the device, warm-up, then timed blocks of calls (one synchronisation per
block), the timing tools/sacd_bench.py uses.  Prints one JSON line per P.
    python tools/envelope_bench.py [--ddpg] [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

O, A, R, H, B, W, ROWS = 2, 4, 2, 256, 256, 128, 2048
WARM, BLOCK, BLOCKS = 3, 5, 4            # 4 blocks of 5 = 20 timed calls per point
KW = dict(gamma=0.99, tau=0.01, lr=1e-3, beta=0.95)
KW_DDPG = dict(gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, beta=0.95)


def _engine(P, ddpg=False):
    if ddpg:
        e = Engine(N.ALGO_ENVELOPE_DDPG, O, A, ROWS, n_learners=P, hidden=H, batch_max=B * W, reward_dim=R)
    else:
        e = Engine(N.ALGO_ENVELOPE_DQN, O, A, ROWS, n_learners=P, discrete=True, hidden=H, batch_max=B * W, reward_dim=R)
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            flat = (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32)
            for k in (N.PARAM_ONLINE, N.PARAM_TARGET):
                e.set_params(net, flat, k, learner=p)
    e.fill_synthetic(ROWS, seed=3)
    return e


def _learn(e, ddpg, **kw):
    return e.envelope_ddpg_learn(B, W, **KW_DDPG, **kw) if ddpg else e.envelope_learn(B, W, **KW, **kw)


def _block(e, n, ddpg):
    e.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        _learn(e, ddpg)
    e.sync()
    return time.perf_counter() - t0


def main(ps, ddpg=False):
    for P in ps:
        e = _engine(P, ddpg)
        _block(e, WARM, ddpg)
        tot = sum(_block(e, BLOCK, ddpg) for _ in range(BLOCKS))
        calls = BLOCKS * BLOCK
        us = 1e6 * tot / calls
        out = _learn(e, ddpg, want_loss=True)
        loss = np.stack([out["critic_loss"], out["actor_loss"]]) if ddpg else out["loss"]
        print(json.dumps(dict(algo="envelope_ddpg" if ddpg else "envelope_dqn", P=P, obs=O, actions=A, objectives=R, hidden=H, batch=B, weight_num=W, rows=B * W, calls=calls,
                              learn_us=round(us, 1), updates_per_s=round(P / us * 1e6, 1), rows_per_s=round(P * B * W / us * 1e6),
                              finite=bool(np.all(np.isfinite(loss))), lds_rc=e.lds_bytes())), flush=True)
        e.close()


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--ddpg"]
    main([int(x) for x in argv] or [1, 64], ddpg="--ddpg" in sys.argv[1:])
