#!/usr/bin/env python3
"""Golden run of the reference's own `__main__` loop of MADDPG_file/MADDPG_simple_with_tricks.py (trick = {'ATT': True}, its default) on
the in-repo SpreadEnv stand-in, exactly as tests/golden/make_loop_golden.py runs MADDPG_simple.  Run by hand where the reference tree exists:

    python -m tests.golden.make_att_loop_golden

6 episodes of 25 steps, learn() from step 51 on: 100 updates.  Writes tests/golden/loop_maddpg_att.npz (outputs only)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import synth  # noqa: E402
from tests.golden.make_loop_golden import run_reference  # noqa: E402

NAME = "loop_maddpg_att"
FLAGS = "--env_name simple_spread_v3 --N 3 --seed 100 --max_episodes 6 --start_steps 50 --batch_size 32 --buffer_size 500 --device cpu"


def main():
    sys.modules.pop("ATT", None)          # a fresh ATT_critic.id_num (a class-level counter: one policy per process)
    log, returns, sd, npy_name, ckpt_name = run_reference("MADDPG_file", "MADDPG_simple_with_tricks", FLAGS)
    out = {"flags": np.array(FLAGS), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
           "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
    for a, d in sd.items():
        synth.pack_digest("ckpt/" + a, {k: v.numpy() for k, v in d.items()}, out, full_limit=0)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print("%s steps %d episodes %d returns[:3] %s -> %.1f KB" % (NAME, len(log["actions"]), np.asarray(returns).shape[-1],
                                                               np.round(np.asarray(returns).reshape(-1)[:3], 3), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
