"""learn() time of discrete SAC (kernels_sacd.hip) against continuous SAC on the same row-chunk chain.

  discrete SAC    obs 8, 4 actions, batch 256, hidden 128
  continuous SAC  obs 8, act 2,     batch 256, hidden 128, FRL_CRITIC_V2=0 (the row-chunk kernels, not the chained family)

Per population P: both engines built in this process, device-drawn rows, warm-up, then alternating timed blocks of calls
(one synchronisation per block) until each side has >= 60 timed calls.  Prints one JSON line per P.
    python tools/sacd_bench.py [P ...]      (default P = 1 16 64 128 512)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

O, B, H, ROWS = 8, 256, 128, 2048
WARM, BLOCK, BLOCKS = 20, 20, 4          # 4 blocks of 20 = 80 timed calls per side and point


def _engine(discrete, P):
    if discrete:
        e = Engine(N.ALGO_SAC_DISCRETE, O, 4, ROWS, n_learners=P, twin_critic=True, hidden=H, batch_max=B)
    else:
        os.environ["FRL_CRITIC_V2"] = "0"        # read at frl_create: the row-chunk family whatever P
        try:
            e = Engine(N.ALGO_SAC, O, 2, ROWS, n_learners=P, twin_critic=True, hidden=H, batch_max=B)
        finally:
            del os.environ["FRL_CRITIC_V2"]
        assert e.learn_path(B)[0] == 0
    g = np.random.default_rng(1)
    for p in range(P):
        for k in (N.PARAM_ONLINE, N.PARAM_TARGET):
            for net in (0, 1):
                e.set_params(net, (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32), k, learner=p)
        e.set_alpha_state([np.log(0.01), 0.0, 0.0, 0.01], 0, learner=p)
    A = 1 if discrete else 2
    n = P * ROWS
    rec = np.concatenate([g.standard_normal((n, O)),
                          g.integers(0, 4, (n, 1)) if discrete else g.uniform(-1, 1, (n, A)),
                          g.standard_normal((n, 1)), (g.random((n, 1)) < 0.05), g.standard_normal((n, O))], axis=1)
    e.add_batch(rec.astype(np.float32), learners=np.repeat(np.arange(P, dtype=np.int32), ROWS))
    return e


def _kw(discrete):
    return dict(gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=3e-4, alpha_lr=1e-4,
                target_entropy=float(0.6 * np.log(4.0)) if discrete else -2.0)


def _block(e, discrete, n):
    kw = _kw(discrete)
    e.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        e.learn(B, **kw)
    e.sync()
    return time.perf_counter() - t0


def main(ps):
    for P in ps:
        eng = {d: _engine(d, P) for d in (True, False)}
        for d, e in eng.items():
            _block(e, d, WARM)
        tot = {True: 0.0, False: 0.0}
        for _ in range(BLOCKS):
            for d in (True, False):
                tot[d] += _block(eng[d], d, BLOCK)
        calls = BLOCKS * BLOCK
        us = {d: 1e6 * tot[d] / calls for d in tot}
        st = eng[True].learn(B, want_stats=True, **_kw(True))
        print(json.dumps(dict(P=P, calls=calls, sacd_us=round(us[True], 2), sac_rowchunk_us=round(us[False], 2),
                              sacd_updates_per_s=round(P / us[True] * 1e6), sac_updates_per_s=round(P / us[False] * 1e6),
                              ratio=round(us[True] / us[False], 3), sacd_finite=bool(np.all(np.isfinite(st))),
                              rc=eng[True].learn_path(B)[2])), flush=True)
        for e in eng.values():
            e.close()


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or [1, 16, 64, 128, 512])
