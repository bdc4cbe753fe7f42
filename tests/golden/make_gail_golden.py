#!/usr/bin/env python3
"""Golden OUTPUT vectors of GAIL's discriminator (GAIL_file/GAIL.py), by running the imported reference (PyTorch CPU) on the seeded
cases of tests/gail_oracle.py.  Run by hand where the reference tree exists:

    python -m tests.golden.make_gail_golden

`GAIL(config)` also builds the script's PPO (GAIL_file/PPO2.py), which is not ported: the config carries a small 'PPO' section for
its constructor and nothing of it is recorded.  A case's discriminator takes PCG64 parameters through `load_state_dict`; every
call's expert rows (indices drawn with replacement) and policy rows come from the oracle module.  The fixture records, per call,
trian_D's 4-tuple, and at the end compute_reward on the probe batch and digests of the net and Adam's moments.

The class case runs the host side as well: `ExpertDataset` on an .npz of unscaled arrays (the scaled rows and the four bounds are
recorded as digests), the seeded default init of `GAIL(config)`, and `torch.randint` draws after `torch.manual_seed(seed + 1)`.

The reference's helper modules (PPO2, PPO2_utils, GAIL_utils, config) are popped from sys.modules afterwards.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import gail_oracle as go  # noqa: E402
from tests.golden import synth  # noqa: E402
from tests.golden._ref_import import import_reference  # noqa: E402
from tests.golden.make_golden import adam_state, load, t2n  # noqa: E402

_HELPERS = ("PPO2", "PPO2_utils", "GAIL_utils", "config")
PPO_SECTION = dict(policy_mlp_dim=32, activation="LeakyReLU", dropout=0.0, layernorm=False, log_std_min=-10, log_std_max=2, p_lr=1e-4,
                   v_lr=3e-4, horizon=64, gamma=0.99, lam=0.95, clip_epsilon=0.2, K_epochs=1, value_loss_coef=1, ent_weight=0.01,
                   mini_batch_size=16, eval_interval=10, eval_episodes=1)


def reference():
    mod = import_reference("GAIL_file", "GAIL")
    utils = sys.modules.get("GAIL_utils")
    for name in _HELPERS:
        sys.modules.pop(name, None)
    return mod, utils


def ref_config(c):
    cfg = go.config(c)
    cfg["PPO"] = dict(PPO_SECTION)
    return cfg


def split(rows, c):
    t = torch.as_tensor(np.asarray(rows, np.float32))
    return t[:, :c["s_dim"]], t[:, c["s_dim"]:]


def pack_state(name, gail, out):
    synth.pack_digest(name + "/net", t2n(gail.D_model.state_dict()), out)
    m, v, step = adam_state(gail.D_optimizer, gail.D_model)
    synth.pack_digest(name + "/m", m, out)
    synth.pack_digest(name + "/v", v, out)
    out[name + "/step"] = np.int64(step)


def run_case(mod, name, out):
    c = go.case(name)
    inp = go.inputs(c)
    gail = mod.GAIL(ref_config(c))
    load(gail.D_model, inp["net"])
    tuples = []
    for k in range(c["n_learn"]):
        es, ea = split(inp["expert"][inp["idx"][k]], c)
        ps, pa = split(inp["policy"][k], c)
        tuples.append(gail.trian_D(es, ea, ps, pa))
    out[name + "/tuples"] = np.array(tuples, np.float64)
    out[name + "/reward"] = gail.compute_reward(*split(inp["probe"], c)).numpy().astype(np.float32)
    out[name + "/betas"] = np.array(gail.D_optimizer.param_groups[0]["betas"], np.float64)
    pack_state(name, gail, out)
    print("%-6s d_loss %s  probs %.6g %.6g  w_dis %.6g" % (name, [round(t[0], 6) for t in tuples], tuples[-1][1], tuples[-1][2], tuples[-1][3]))


def run_class(mod, utils, out):
    c = go.case("class")
    seed = c["seed"]
    inp = go.inputs(c)
    states, actions = go.raw_expert(c, seed)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "expert.npz")
        np.savez(path, states=states, actions=actions)
        ds = utils.ExpertDataset(path)
    out["class/n"] = np.int64(len(ds))
    synth.pack_digest("class/dataset", dict(states=ds.states, actions=ds.actions, space_low=ds.space_low, space_high=ds.space_high,
                                            action_low=ds.action_low, action_high=ds.action_high), out, full_limit=0)
    gail = mod.GAIL(ref_config(c))
    synth.pack_digest("class/init", t2n(gail.D_model.state_dict()), out)
    torch.manual_seed(seed + 1)
    tuples, idxs = [], []
    for k in range(c["n_learn"]):
        idx = torch.randint(high=len(ds), size=(c["n_expert"],), dtype=torch.int64)
        idxs.append(idx.numpy().copy())
        es = torch.as_tensor(ds.states[idx.numpy()], dtype=torch.float32)
        ea = torch.as_tensor(ds.actions[idx.numpy()], dtype=torch.float32)
        ps, pa = split(inp["policy"][k], c)
        tuples.append(gail.trian_D(es, ea, ps, pa))
    out["class/idx"] = np.stack(idxs)
    out["class/tuples"] = np.array(tuples, np.float64)
    out["class/reward"] = gail.compute_reward(*split(inp["probe"], c)).numpy().astype(np.float32)
    pack_state("class", gail, out)
    print("class  d_loss %s" % [round(t[0], 6) for t in tuples])


def gen():
    mod, utils = reference()
    out = {}
    for name in go.CASES:
        run_case(mod, name, out)
    run_class(mod, utils, out)
    np.savez_compressed(os.path.join(HERE, "gail.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(1)
    gen()
    print("wrote gail.npz")
