#!/usr/bin/env python3
"""Golden run of the reference's own `__main__` loop of CEM_GD3PG_file/CEM_GD3PG.py on the in-repo short Pendulum, through
tests/golden/make_loop_golden.py's run_reference, unchanged.  Run by hand where the reference tree exists:

    python -m tests.golden.make_cem_gd3pg_loop_golden

--pop_size 4: four population episodes into `buffer`, then seven training episodes (two fitness episodes and one noisy domain episode
each), a generation step (tell, ask, four evaluations, the mix into the poorer actor) before the fifth, and one learn() per step from the
third on (40 steps each): 200 learn() calls.  The fixture holds every env action and reward of every episode, the returns the script saved and digests
of the actor_domain checkpoint it wrote."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden import synth  # noqa: E402
from tests.golden.make_loop_golden import run_reference  # noqa: E402

NAME = "loop_cem_gd3pg"
FLAGS = "--env_name PendulumShort-v1 --seed 0 --max_episodes 7 --start_steps 100 --batch_size 64 --buffer_size 1000 --pop_size 4"


def main():
    log, returns, sd, npy_name, ckpt_name = run_reference("CEM_GD3PG_file", "CEM_GD3PG", FLAGS)
    out = {"flags": np.array(FLAGS), "returns": np.asarray(returns, np.float64), "actions": np.stack(log["actions"]),
           "rewards": np.stack(log["rewards"]), "npy_name": np.array(npy_name), "ckpt_name": np.array(ckpt_name)}
    synth.pack_digest("ckpt", {k: v.numpy() for k, v in sd.items()}, out, full_limit=0)
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d env steps, returns %s -> %.1f KB" % (NAME, len(log["actions"]), np.round(out["returns"], 2), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
