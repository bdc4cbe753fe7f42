#!/usr/bin/env python3
"""Golden run of the reference's own `__main__` loop of MAAC_file/MASAC.py on the in-repo SpreadEnv stand-in, exactly as
tests/golden/make_loop_golden.py runs the MADDPG scripts.  Run by hand where the reference tree exists:

    python -m tests.golden.make_masac_loop_golden

6 episodes of 25 steps, learn() from step 51 on: 100 updates of 3 agents.  Writes tests/golden/loop_masac.npz (outputs only).  The
script keeps the returns of every 100th episode only, so the returns array of this run is empty ([3, 0]): the env actions and rewards
step by step and the checkpoint are what the test follows.

The script resets its env WITHOUT a seed (its own comment says the seed is lost that way), and the stand-in's generator is unseeded
until a reset names one: the recording seeds it with ENV_SEED at construction (`seeded_spread_env`), and the test does the same."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import synth  # noqa: E402
from tests.golden.make_loop_golden import run_reference  # noqa: E402

import contextlib  # noqa: E402

NAME = "loop_masac"
ENV_SEED = 100
FLAGS = "--env_name simple_spread_v3 --N 3 --seed 100 --max_episodes 6 --start_steps 50 --batch_size 32 --buffer_size 500 --device cpu"


@contextlib.contextmanager
def seeded_spread_env():
    """every SpreadEnv built inside starts from default_rng(ENV_SEED) instead of OS entropy"""
    from freerl_amd import envs as E
    init = E.SpreadEnv.__init__

    def seeded(self, *a, **k):
        init(self, *a, **k)
        self.np_random = np.random.default_rng(ENV_SEED)
    E.SpreadEnv.__init__ = seeded
    try:
        yield
    finally:
        E.SpreadEnv.__init__ = init


def main():
    with seeded_spread_env():
        log, returns, sd, npy_name, ckpt_name = run_reference("MAAC_file", "MASAC", FLAGS)
    out = {"flags": np.array(FLAGS), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
           "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
    for a, d in sd.items():
        synth.pack_digest("ckpt/" + a, {k: v.numpy() for k, v in d.items()}, out, full_limit=0)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print("%s steps %d returns shape %s -> %.1f KB" % (NAME, len(log["actions"]), np.asarray(returns).shape, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
