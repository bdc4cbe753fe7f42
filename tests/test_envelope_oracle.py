"""CPU: the NumPy restatement of envelope multi-objective DQN (tests/envelope_oracle.py) against the reference's outputs
(tests/golden/envelope_dqn.npz: ENVELOPE_MORL_file/ENVELOPE_DQN.py run by make_envelope_golden.py).  Every call trains on the rows
and preference vectors the reference drew; no row is left out of any comparison: the generator kept only seeds whose argmax
margins are at least envelope_oracle.MARGIN."""
import os

import numpy as np
import pytest

from tests import envelope_oracle as eo
from tests.golden import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "envelope_dqn.npz")))


def run_golden(fx, name, dtype=np.float32):
    c = eo.case(name)
    inp = eo.inputs(c, seed=int(fx[name + "/seed"]))
    inp["idx"], inp["weights"] = list(fx[name + "/idx"]), list(fx[name + "/weights"])
    return c, eo.run(c, inp, dtype=dtype)


def check_state(fx, name, o, c):
    for key, p in (("net", o.q), ("target", o.q_t)):
        synth.check_digest(name + "/" + key, p, fx, rtol=2e-4, atol=2e-6, label=name)
    # Adam's first moment: a bias gradient is a sum over the rows with cancellation (test_sacd_oracle.py's rule)
    synth.check_digest(name + "/m", o.opt.m, fx, rtol=5e-3, atol=2e-5, label=name)
    assert int(fx[name + "/step"]) == o.opt.t == c["n_learn"]


@pytest.mark.parametrize("name", list(eo.CASES))
def test_oracle_matches_reference(fx, name):
    c, (o, losses) = run_golden(fx, name)
    assert fx[name + "/idx"].shape == (c["n_learn"], c["batch"]) and fx[name + "/weights"].shape == (c["n_learn"], c["weight_num"], c["rdim"])
    np.testing.assert_allclose(losses, fx[name + "/loss"], rtol=1e-4, atol=1e-6)
    check_state(fx, name, o, c)
    # the margin the generator kept the seed for holds on the oracle's values too
    assert float(fx[name + "/min_gap"]) >= eo.MARGIN and o.min_gap >= 0.5 * eo.MARGIN


@pytest.mark.parametrize("name", list(eo.CASES))
def test_float64_mode_agrees(fx, name):
    c, (o64, l64) = run_golden(fx, name, dtype=np.float64)
    _, (o32, l32) = run_golden(fx, name)
    assert l64.dtype == np.float64 and o64.q["l1.weight"].dtype == np.float64
    np.testing.assert_allclose(l32, l64, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(l64, fx[name + "/loss"], rtol=1e-4, atol=1e-6)
    for k in o32.q:
        np.testing.assert_allclose(o32.q[k], o64.q[k], rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(o32.q_t[k], o64.q_t[k], rtol=2e-4, atol=2e-6)
        np.testing.assert_allclose(o32.opt.m[k], o64.opt.m[k], rtol=5e-3, atol=2e-5)


def replay_class(fx, dtype=np.float32):
    """The class case's script on the oracle, with the preference vectors and sampled rows the reference drew."""
    c = eo.case("class")
    inp = eo.inputs(c, seed=int(fx["class/seed"]))
    t, o = inp["table"], eo.make(c, inp, dtype)
    pref, learn_at = fx["class/pref"], eo.class_schedule(c)
    choices, prios, losses = [], [], []
    for i in range(c["n_steps"]):
        choices.append(o.choose(t["obs"][i], pref[2 * i])[0])
        o.add(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]))
        prios.append(o.priority(t["obs"][i], t["act"][i, 0], t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"], pref[2 * i + 1]))
        if i in learn_at:
            k = len(losses)
            losses.append(o.learn_with(fx["class/idx"][k], fx["class/weights"][k], c["gamma"], c["tau"], fx["class/beta"][i]))
    return c, o, np.array(choices), np.array(prios), np.array(losses)


def test_class_case(fx):
    c, o, choices, prios, losses = replay_class(fx)
    assert len(fx["class/pref"]) == 2 * c["n_steps"] and c["n_steps"] > c["capacity"]       # the ring wraps
    assert len(losses) == c["n_learn"] and eo.class_schedule(c)[4] >= c["capacity"]         # ... and half the calls come after
    np.testing.assert_array_equal(choices, fx["class/choice"])
    np.testing.assert_allclose(prios, fx["class/priority"], rtol=1e-4)
    np.testing.assert_allclose(fx["class/final_priority"], fx["class/priority"][-c["capacity"]:], rtol=0)    # the deque: oldest first
    np.testing.assert_allclose(losses, fx["class/loss"], rtol=1e-4, atol=1e-6)
    check_state(fx, "class", o, c)
    # the homotopy on beta: the reference's Python-float recurrence, advanced on every done
    done = eo.inputs(c, seed=int(fx["class/seed"]))["table"]["done"]
    beta = b0 = c["beta"]
    base = float(np.power(1000. * (1.0 - b0), 1. / c["max_episodes"]))
    delta, want = base / 1000., []
    for d in done:
        if d:
            beta += delta
            delta = (beta - b0) * base + b0 - beta
        want.append(beta)
    np.testing.assert_allclose(fx["class/beta"], want, rtol=0, atol=1e-12)
    assert done.sum() >= 2 and float(fx["class/select_gap"]) >= eo.MARGIN and float(fx["class/min_gap"]) >= eo.MARGIN
