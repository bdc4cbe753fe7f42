"""Time of one action-masked MAPPO `learn()` (kernels_mappo_mask.hip) against the unmasked one (kernels_mappo.hip) on the same
discrete shape, from the same build, in one command:

  3 agents x (80 obs, 9 actions), hidden 128, horizon 256 in one minibatch of 256, K_epochs 15, every trick on

a STAND-IN for the script's SMACv2 shape, whose dimensions come from the environment and cannot be read without it.  Per population P,
two engines hold the same rows and parameters; the masked one has a random mask per row and agent with the stored action open.  Both
run `frl_mappo_learn` with device-drawn permutations and the masked class's settings (two Adams, eps 1e-5, clip_norm 0.5).  The two
sides run ALTERNATELY, block by block; a block is a few calls between two synchronisations (host clock), after a warm-up call of each
side.  Prints one JSON line per (P, side), then one with the ratio.
    python tools/mappo_mask_bench.py [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

NA, O, A, H, T, K = 3, 80, 9, 128, 256, 15
HYPER = dict(gamma=0.95, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3, adam_eps=1e-5, clip_norm=0.5, adv_norm=True,
             value_clip=True, huber_delta=10.0)
BLOCKS = 5


def _rows(P, seed):
    g = np.random.default_rng(seed)
    obs = g.standard_normal((P, T, NA, O)).astype(np.float32)
    act = g.integers(0, A, (P, T, NA, 1))
    mask = g.random((P, T, NA, A)) < 0.5
    np.put_along_axis(mask, act, True, axis=3)
    return dict(obs=obs, nobs=(obs + 0.3 * g.standard_normal(obs.shape)).astype(np.float32), act=act.astype(np.float32),
                logp=np.log(g.uniform(0.15, 0.6, (P, T, NA, 1))).astype(np.float32), rew=g.standard_normal((P, T, NA)).astype(np.float32),
                done=np.zeros((P, T, NA), np.float32), adv_done=(np.arange(T) % 25 == 24).astype(np.float32)[None, :, None].repeat(P, 0).repeat(NA, 2),
                mask=mask.astype(np.float32))


def _engine(P, rows, masked):
    e = Engine(N.ALGO_MAPPO, [O] * NA, [A] * NA, T, n_learners=P, discrete=True, hidden=H, batch_max=T, extra_cols=2 * NA + (NA * A if masked else 0))
    e.net_norm_set(True, True)
    if masked:
        e.action_mask_set(True)
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            e.set_params(net, (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32), learner=p)
    f = lambda x: x.reshape(P * T, -1)
    cols = [f(rows["obs"]), f(rows["act"]), f(rows["rew"]), f(rows["done"]), f(rows["nobs"]), f(rows["logp"]), f(rows["adv_done"])]
    if masked:
        cols.append(f(rows["mask"]))
    e.add_batch(np.concatenate(cols, axis=1), learners=np.repeat(np.arange(P), T).astype(np.int32))
    e.flush()
    return e


def _block(e, n):
    e.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        e.mappo_learn(T, T, K, **HYPER)      # (the rows stay: learn() resets the counters only, and reads the whole capacity)
    e.sync()
    return time.perf_counter() - t0


def main(ps):
    for P in ps:
        rows = _rows(P, 2)
        sides = [("unmasked", _engine(P, rows, False)), ("masked", _engine(P, rows, True))]
        n = 20 if P == 1 else 5
        total = {s: 0.0 for s, _ in sides}
        for _, e in sides:
            _block(e, 1)                                   # warm-up
        for _ in range(BLOCKS):                            # the two sides alternately
            for side, e in sides:
                total[side] += _block(e, n)
        ms = {}
        for side, e in sides:
            ms[side] = 1e3 * total[side] / (BLOCKS * n)
            finite = all(np.isfinite(e.get_params(net)).all() for net in range(e.n_nets))
            print(json.dumps(dict(algo="mappo", side=side, P=P, agents=NA, obs=O, act=A, hidden=H, horizon=T, minibatch=T, k_epochs=K,
                                  calls=BLOCKS * n, call_ms=round(ms[side], 3), finite=finite, lds_rc=e.lds_bytes())), flush=True)
            e.close()
        print(json.dumps(dict(P=P, masked_over_unmasked=round(ms["masked"] / ms["unmasked"], 4))), flush=True)


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or [1, 64])
