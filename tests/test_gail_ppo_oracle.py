"""CPU: tests/gail_ppo_oracle.py (GAIL_file/PPO2.py's PPO_learn in NumPy float64) against tests/golden/gail_ppo.npz, the reference's own
output on the same inputs, at the tolerances tests/test_gpu_ppo_edges.py uses for the same arithmetic — and, from the oracle alone, the
conditioning rules every case has to meet before an engine is held to it."""
import os

import numpy as np
import pytest

from tests import gail_ppo_oracle as go
from tests.golden import synth

ACTOR_TOL = dict(rtol=2e-4, atol=5e-6)
CRITIC_TOL = dict(rtol=2e-4)
PARAM_TOL = dict(rtol=2e-3, atol=2e-5)
ADV_TOL = dict(rtol=1e-4, atol=1e-5)
ALL = go.CASES + go.POPULATION


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "gail_ppo.npz"))


def check_against_fixture(name, orc, outs, fx, label):
    """An oracle-shaped result (nets, moments, step, per-call GAE outputs, loss lists) against the fixture's record `name`."""
    np.testing.assert_allclose(np.stack([o["adv_norm"] for o in outs]), fx[name + "/advantages"], err_msg=label + " advantages", **ADV_TOL)
    np.testing.assert_allclose(np.stack([o["returns"] for o in outs]), fx[name + "/returns"], err_msg=label + " returns", **ADV_TOL)
    np.testing.assert_allclose(orc.actor_losses, fx[name + "/actor_losses"], err_msg=label + " actor losses", **ACTOR_TOL)
    np.testing.assert_allclose(orc.critic_losses, fx[name + "/critic_losses"], err_msg=label + " critic losses", **CRITIC_TOL)
    assert orc.step == int(fx[name + "/step"])
    for net, params in (("actor", orc.actor), ("critic", orc.critic)):
        synth.check_digest("%s/%s" % (name, net), params, fx, PARAM_TOL["rtol"], PARAM_TOL["atol"], label)
        # Adam's moments: m at the gradient's scale (clipped to norm 0.5), v at its square
        synth.check_digest("%s/%s_m" % (name, net), orc.m[net], fx, 2e-3, 1e-6, label)
        synth.check_digest("%s/%s_v" % (name, net), orc.v[net], fx, 4e-3, 1e-9, label)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c["name"])
def test_oracle_reproduces_the_reference(c, fx):
    name = c["name"]
    np.testing.assert_array_equal(np.stack(go.inputs(c)["perms"]), fx[name + "/perms"])      # the reference consumed the case's permutations
    r = go.oracle_run(c)
    check_against_fixture(name, r["orc"], r["outs"], fx, name)
    orc, probe = r["orc"], go.inputs(c)["probe"]
    if c["discrete"]:
        np.testing.assert_array_equal(orc.pi_mean(probe), fx[name + "/probe_pi"])
    else:
        np.testing.assert_allclose(orc.pi_mean(probe), fx[name + "/probe_pi"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(orc.value(probe), fx[name + "/probe_value"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c["name"])
def test_conditioning_rules_hold_from_the_oracle_alone(c):
    go.assert_conditions(c)


def test_the_cases_reach_what_they_are_for():
    r = {c["name"]: go.oracle_run(c) for c in ALL}
    # some case puts rows on the clamped branch of the surrogate
    assert sum(int(x[1].sum()) for x in r["relu-17-6"]["orc"].ratio_log) > 0
    # clamp: the on-bound columns 0 and 2 move by p_lr in the first step, the past-bound columns 1 and 3 never move and keep zero moments
    c = go.BY_NAME["clamp"]
    first = dict(c, K=1, T=c["mb"], name="clamp-first")
    o1 = go.Oracle(first, go.inputs(c)["params"])
    tab = {k: v[:c["mb"]] for k, v in go.inputs(c)["table"].items()}
    o1.learn(tab, [np.arange(c["mb"])], 0.0)
    moved = np.abs(o1.actor["log_std"].reshape(-1) - np.array(c["log_std"]))
    # (Adam's first step is lr g / (|g| + 1e-8): a clipped gradient of order 1e-5 leaves it a few 1e-4 short of lr)
    np.testing.assert_allclose(moved[[0, 2]], go.HYPER["p_lr"], rtol=1e-3)
    full = r["clamp"]["orc"]
    assert (full.actor["log_std"].reshape(-1)[[1, 3]] == np.array(c["log_std"])[[1, 3]]).all()
    assert (full.m["actor"]["log_std"].reshape(-1)[[1, 3]] == 0).all() and (full.v["actor"]["log_std"].reshape(-1)[[1, 3]] == 0).all()
    # range: the same net under two ranges gives different results
    a, b = r["range-wide"]["orc"], r["range-narrow"]["orc"]
    assert np.abs(np.array(a.actor_losses) - np.array(b.actor_losses)).max() > 1e-3
    assert np.abs(a.actor["backbone.2.weight"] - b.actor["backbone.2.weight"]).max() > 1e-4


def test_gae_bootstraps_across_an_episode_end():
    """mask_1 == 1: behind a `done` row the TD residual still takes the next row's value.  On the first case's table the two recurrences
    differ on the done rows by far more than the tolerance the engine is held to."""
    c = go.BY_NAME["leaky-3-1"]
    inp = go.inputs(c)
    orc = go.Oracle(c, inp["params"])
    tab = inp["table"]
    vs = orc.value(tab["states"])
    kept = orc.gae(tab["rewards"].astype(np.float64), vs, tab["done"].astype(np.float64), c["last_value"])[0]
    other = orc.gae(tab["rewards"].astype(np.float64), vs, tab["done"].astype(np.float64), c["last_value"], bootstrap_done=True)[0]
    rows = np.nonzero(tab["done"])[0]
    assert list(rows) == [17, 39]
    assert (np.abs(kept - other)[rows] > 1000 * (ADV_TOL["atol"] + ADV_TOL["rtol"] * np.abs(kept[rows]))).all()


def test_class_case_from_the_recorded_init_and_permutations(fx):
    """The fixture's class record: PPO(config)'s seeded init and torch's own randperm draws; the oracle, started from the recorded init and
    given the recorded draws, lands where the reference did."""
    c = dict(go.BY_NAME["leaky-3-1"], name="class")
    params = {net: {k[len("class/init_%s/" % net):-len("/full")]: fx[k] for k in fx.files if k.startswith("class/init_%s/" % net) and k.endswith("/full")}
              for net in ("actor", "critic")}
    assert set(params["actor"]) == {"log_std"} | {n + s for n in go.NAMES for s in (".weight", ".bias")} and params["actor"]["log_std"].shape == (1, 1)
    assert (params["actor"]["log_std"] == 0).all()
    inp = go.inputs(go.BY_NAME["leaky-3-1"])
    orc = go.Oracle(c, params)
    outs = [orc.learn(inp["table"], fx["class/perms"][call], c["last_value"]) for call in range(c["calls"])]
    check_against_fixture("class", orc, outs, fx, "class")
