"""One hindsight relabel at an episode's end (frl_her_relabel, kernels_her.hip) against the same rows built on the host and pushed
through frl_buffer_add_batch + frl_buffer_flush, on the same build.

  DDPG engine, obs [3 | 3], act 1, hidden 128; every learner's episode is L = 200 steps, sample_num 4, sample_range 200: 794 rows each.

Per population P, after warm-up, REPS timed calls per side, each from the same cursor (the cursors are put back outside the timed
window) and each ending in a device synchronise:
  relabel_device    picks drawn by the kernel, env actions uploaded
  relabel_injected  picks drawn on the host beforehand and uploaded with the env actions
  host_build_push   the rows assembled in NumPy (vectorised over the episode: the host's best case, not the script's per-row loop)
                    from a host copy of the episode, then add_batch + flush
  host_push         add_batch + flush of rows assembled beforehand
  host_per_row_add  the script's shape: one Engine.add call per row assembled beforehand (what policy.add does), then flush; 5 timed calls
Prints one JSON line per P (median and range in us).
    python tools/her_bench.py [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

S, G, A, H, L, K, R, CAP = 3, 3, 1, 128, 200, 4, 200, 2048
W = np.array([1.0, 1.0, 0.1])
WARM, REPS = 5, 30


def _counts():
    return np.array([min(K, R, L - i) for i in range(L)])


def _picks(rng):
    out = []
    for i in range(L):
        m = min(R, L - i)
        out.extend(range(m) if m < K else rng.choice(m, K, replace=False))
    return np.asarray(out, np.int32)


def _build(lay, obs, nobs, env_act, picks):
    """The relabelled records of one episode, vectorised."""
    i = np.repeat(np.arange(L), _counts())
    g = nobs[i + picks, :G]
    rec = np.zeros((i.size, lay.width), np.float32)
    rec[:, lay.obs_off[0]:lay.obs_off[0] + S] = obs[i, :S]
    rec[:, lay.obs_off[0] + S:lay.obs_off[0] + S + G] = g
    rec[:, lay.act_off[0]:lay.act_off[0] + A] = env_act[i]
    d = g.astype(np.float64) - obs[i, :G].astype(np.float64)
    cost = W[0] * (d[:, 0] * d[:, 0]) + W[1] * (d[:, 1] * d[:, 1]) + W[2] * (d[:, 2] * d[:, 2])
    rec[:, lay.rew_off] = np.where(cost < 0.5, 0.0, -1.0)
    rec[:, lay.next_obs_off[0]:lay.next_obs_off[0] + S] = nobs[i, :S]
    rec[:, lay.next_obs_off[0] + S:lay.next_obs_off[0] + S + G] = g
    return rec


def _timed(eng, P, fn, warm=WARM, reps=REPS):
    t = []
    for rep in range(warm + reps):
        for p in range(P):
            eng.set_cursor(p, L, L)
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        if rep >= warm:
            t.append(1e6 * (time.perf_counter() - t0))
    return dict(median=round(float(np.median(t)), 1), min=round(min(t), 1), max=round(max(t), 1))


def main(ps):
    total = int(_counts().sum())
    for P in ps:
        eng = Engine(N.ALGO_DDPG, S + G, A, CAP, n_learners=P, hidden=H, batch_max=256)
        lay = eng.layout
        rng = np.random.default_rng(1)
        states = (0.5 * rng.standard_normal((P, L + 1, S))).astype(np.float32)
        goal = (0.5 * rng.standard_normal((P, 1, G))).astype(np.float32)
        obs = np.concatenate((states[:, :-1], np.repeat(goal, L, 1)), 2)
        nobs = np.concatenate((states[:, 1:], np.repeat(goal, L, 1)), 2)
        env_act = rng.uniform(-2, 2, (P, L, A)).astype(np.float32)
        real = np.zeros((P, L, lay.width), np.float32)
        real[:, :, lay.obs_off[0]:lay.obs_off[0] + S + G] = obs
        real[:, :, lay.act_off[0]:lay.act_off[0] + A] = rng.uniform(-1, 1, (P, L, A))
        real[:, :, lay.next_obs_off[0]:lay.next_obs_off[0] + S + G] = nobs
        learners = np.repeat(np.arange(P, dtype=np.int32), L)
        eng.add_batch(real.reshape(-1, lay.width), learners)
        eng.flush()
        picks = np.concatenate([_picks(rng) for _ in range(P)])
        kw = dict(state_dim=S, goal_dim=G, sample_num=K, sample_range=R, env_actions=env_act)
        ids, lens = np.arange(P), np.full(P, L)
        out_learners = np.repeat(np.arange(P, dtype=np.int32), total)
        prebuilt = np.concatenate([_build(lay, obs[p], nobs[p], env_act[p], picks[p * total:(p + 1) * total]) for p in range(P)])

        def build_push():
            rows = np.concatenate([_build(lay, obs[p], nobs[p], env_act[p], picks[p * total:(p + 1) * total]) for p in range(P)])
            eng.add_batch(rows, out_learners)
            eng.flush()

        def push():
            eng.add_batch(prebuilt, out_learners)
            eng.flush()

        def per_row():
            for row, p in zip(prebuilt, out_learners):
                eng.add(p, row)
            eng.flush()

        res = dict(P=P, L=L, rows_per_episode=total, reps=REPS,
                   relabel_device=_timed(eng, P, lambda: eng.her_relabel(ids, lens, **kw)),
                   relabel_injected=_timed(eng, P, lambda: eng.her_relabel(ids, lens, picks=picks, **kw)),
                   host_build_push=_timed(eng, P, build_push), host_push=_timed(eng, P, push),
                   host_per_row_add=_timed(eng, P, per_row, 1, 5))
        # the two paths leave the same ring (injected picks)
        for p in range(P):
            eng.set_cursor(p, L, L)
        eng.her_relabel(ids, lens, picks=picks, **kw)
        a = [eng.read_rows(p, 0, L + total) for p in (0, P - 1)]
        for p in range(P):
            eng.set_cursor(p, L, L)
        push()
        b = [eng.read_rows(p, 0, L + total) for p in (0, P - 1)]
        res["same_ring"] = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        res["host_push_over_relabel_injected"] = round(res["host_push"]["median"] / res["relabel_injected"]["median"], 1)
        res["host_per_row_add_over_relabel_injected"] = round(res["host_per_row_add"]["median"] / res["relabel_injected"]["median"], 1)
        res["host_build_push_over_relabel_injected"] = round(res["host_build_push"]["median"] / res["relabel_injected"]["median"], 1)
        print(json.dumps(res), flush=True)
        eng.close()


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or [1, 64])
