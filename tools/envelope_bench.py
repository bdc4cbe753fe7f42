"""learn() time of envelope multi-objective DQN (kernels_envelope.hip) at the reference script's shape:

  obs 2, 4 actions, 2 objectives, hidden 256, batch 256 x weight_num 128 = 32768 rows per call

Per population P: rows and preference vectors drawn on the device, warm-up, then timed blocks of calls (one synchronisation per
block), the timing tools/sacd_bench.py uses.  Prints one JSON line per P.
    python tools/envelope_bench.py [P ...]      (default P = 1 64)
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


def _engine(P):
    e = Engine(N.ALGO_ENVELOPE_DQN, O, A, ROWS, n_learners=P, discrete=True, hidden=H, batch_max=B * W, reward_dim=R)
    g = np.random.default_rng(1)
    for p in range(P):
        flat = (g.standard_normal(e.num_params(0)) * 0.05).astype(np.float32)
        for k in (N.PARAM_ONLINE, N.PARAM_TARGET):
            e.set_params(0, flat, k, learner=p)
    e.fill_synthetic(ROWS, seed=3)
    return e


def _block(e, n):
    e.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        e.envelope_learn(B, W, **KW)
    e.sync()
    return time.perf_counter() - t0


def main(ps):
    for P in ps:
        e = _engine(P)
        _block(e, WARM)
        tot = sum(_block(e, BLOCK) for _ in range(BLOCKS))
        calls = BLOCKS * BLOCK
        us = 1e6 * tot / calls
        loss = e.envelope_learn(B, W, want_loss=True, **KW)["loss"]
        print(json.dumps(dict(P=P, obs=O, actions=A, objectives=R, hidden=H, batch=B, weight_num=W, rows=B * W, calls=calls,
                              learn_us=round(us, 1), updates_per_s=round(P / us * 1e6, 1), rows_per_s=round(P * B * W / us * 1e6),
                              finite=bool(np.all(np.isfinite(loss))), lds_rc=e.lds_bytes())), flush=True)
        e.close()


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or [1, 64])
