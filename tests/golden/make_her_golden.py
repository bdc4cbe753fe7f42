#!/usr/bin/env python3
"""Golden run of the reference's hindsight-replay loop (DDPG_file/DDPG_simple_try_HER.py's `__main__`).

Run by hand in the build container only:   python -m tests.golden.make_her_golden
The script is executed in memory the way tests/golden/make_loop_golden.py does it (same stubs, imported from there).  The one
difference: the reference `Buffer.add` is wrapped so that every added row is recorded in order, and `random.sample` is wrapped so that
the picks of every generate_goals call are recorded as offsets.

  her.npz                 the 776 rows the script added (float32, as Buffer.sample hands them on), which of them are relabelled, the
                          picks, the env actions and the goals of the four episodes
  loop_her_pendulum.npz   what the other loop_*.npz hold: flags, env actions and rewards per step, returns, checkpoint digest, file names
"""
import contextlib
import glob
import io
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import her_oracle as oracle  # noqa: E402
from tests.golden import synth  # noqa: E402
from tests.golden._ref_import import REF_ROOT  # noqa: E402
from tests.golden.make_loop_golden import install_stubs, torch_dtype_tolerant_zeros  # noqa: E402

DIRECTORY, SCRIPT = "DDPG_file", "DDPG_simple_try_HER"
FLAGS = ("--env_name PendulumShort-v1 --seed 0 --max_episodes 4 --save_freq 2 --start_steps 100 --batch_size 64 --buffer_size 1000 "
         "--device cpu")
L, K, R, EPISODES = 40, 4, 200, 4


def run_reference():
    log = dict(actions=[], rewards=[])
    rows, samples = [], []
    install_stubs(log)
    path = os.path.join(REF_ROOT, DIRECTORY, SCRIPT + ".py")
    src = open(path, encoding="utf-8").read()
    tmp = tempfile.mkdtemp(prefix="frl_her_")
    fake = os.path.join(tmp, SCRIPT + ".py")
    sys.modules.pop("Buffer", None)
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REF_ROOT, DIRECTORY))
    import Buffer as ref_buffer                      # the reference's, left in sys.modules for the script's own import
    add = ref_buffer.Buffer.add

    def recording_add(self, obs, action, reward, next_obs, done):
        rows.append((np.array(obs, np.float64), np.array(action, np.float64).reshape(-1), float(reward), np.array(next_obs, np.float64), bool(done)))
        return add(self, obs, action, reward, next_obs, done)
    ref_buffer.Buffer.add = recording_add
    sample = random.sample

    def recording_sample(population, k):
        out = sample(population, k)
        samples.append([next(j for j, t in enumerate(population) if t is el) for el in out])
        return out
    random.sample = recording_sample
    argv, sys.argv = sys.argv, [fake] + FLAGS.split()
    torch.set_num_threads(1)
    try:
        with torch_dtype_tolerant_zeros(), contextlib.redirect_stdout(io.StringIO()):
            exec(compile(src, fake, "exec"), {"__name__": "__main__", "__file__": fake})
    finally:
        sys.argv = argv
        random.sample = sample
        ref_buffer.Buffer.add = add
        sys.path.remove(os.path.join(REF_ROOT, DIRECTORY))
        sys.modules.pop("Buffer", None)
    npys = glob.glob(os.path.join(tmp, "results", "*", "*", "*.npy"))
    ckpt = glob.glob(os.path.join(tmp, "results", "*", "*", "*.pt"))
    assert len(npys) == 1 and len(ckpt) == 1, (npys, ckpt)
    return log, rows, samples, np.load(npys[0]), torch.load(ckpt[0]), os.path.basename(npys[0]), os.path.basename(ckpt[0])


def main():
    log, rows, samples, returns, sd, npy_name, ckpt_name = run_reference()
    per_ep = oracle.total(L, K, R)
    assert per_ep == 154 and len(rows) == EPISODES * (L + per_ep) == 776, (per_ep, len(rows))
    obs = np.stack([r[0] for r in rows]); act = np.stack([r[1] for r in rows]); rew = np.array([r[2] for r in rows])
    nobs = np.stack([r[3] for r in rows]); done = np.array([r[4] for r in rows])
    relabelled = np.zeros(len(rows), bool)
    picks, goals, it = [], [], iter(samples)
    for e in range(EPISODES):
        base = e * (L + per_ep)
        relabelled[base + L:base + L + per_ep] = True
        goals.append(obs[base, 3:])                                 # the episode's goal, float64 as the script held it
        assert all((obs[base + t, 3:] == goals[-1]).all() for t in range(L))
        for i in range(L):
            m = min(R, L - i)
            picks.extend(range(m) if m < K else next(it))
    assert next(it, None) is None
    picks = np.asarray(picks, np.int32)
    # the random.sample(range(m), k) equivalence against the recorded picks
    random.seed(0)
    replay = []
    for e in range(EPISODES):
        for i in range(L):
            m = min(R, L - i)
            replay.extend(range(m) if m < K else random.sample(range(m), K))
    assert (np.asarray(replay) == picks).all(), "random.sample(list, k) is not random.sample(range(len(list)), k) shifted"
    ms = [min(R, L - i) for i in range(L)]
    assert ms.count(K) >= 1 and sum(m < K for m in ms) == 3           # one shuffle, three transitions that take every candidate
    for kind in (relabelled, ~relabelled):
        assert set(np.unique(rew[kind])) == {-1.0, 0.0}, np.unique(rew[kind])
    assert not done.any() or not done[relabelled].any()
    # every cost is clear of the threshold: the recorded rewards cannot hinge on rounding
    for t in range(len(rows)):
        c = oracle.cost(obs[t, 3:], obs[t, :3])
        assert abs(c - 0.5) > 1e-9, (t, c)
    env_actions = np.stack(log["actions"])                            # [160][1] float64, the `action_` of every step
    differs = 0
    for e in range(EPISODES):
        base = e * (L + per_ep)
        p = 0
        for i, n in enumerate(oracle.counts(L, K, R)):
            for s in range(n):
                row = base + L + p
                assert (act[row] == env_actions[e * L + i]).all()    # transition[1]
                differs += bool((act[row].astype(np.float32) != act[base + i].astype(np.float32)).any())
                p += 1
    assert differs > 0, "the relabelled action never differs from the real row's stored action"
    out = dict(obs=obs.astype(np.float32), act=act.astype(np.float32), rew=rew.astype(np.float32), next_obs=nobs.astype(np.float32),
               done=done.astype(np.uint8), relabelled=relabelled, picks=picks, env_actions=env_actions.astype(np.float32),
               goals=np.stack(goals).astype(np.float64), dims=np.array([L, K, R, EPISODES, 3, 3], np.int32))
    path = os.path.join(HERE, "her.npz")
    np.savez_compressed(path, **out)
    print("her.npz: %d rows, %d picks -> %.1f KB" % (len(rows), picks.size, os.path.getsize(path) / 1024))

    loop = {"flags": np.array(FLAGS), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
            "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
    synth.pack_digest("ckpt", {k: v.numpy() for k, v in sd.items()}, loop, full_limit=0)
    path = os.path.join(HERE, "loop_her_pendulum.npz")
    np.savez_compressed(path, **loop)
    print("loop_her_pendulum.npz: steps %d episodes %d returns[:3] %s -> %.1f KB" % (
        len(log["actions"]), np.asarray(returns).shape[-1], np.round(np.asarray(returns).reshape(-1)[:3], 3), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
