"""CPU: the NumPy restatement of envelope multi-objective DDPG (tests/envelope_ddpg_oracle.py) against the reference's outputs
(tests/golden/envelope_ddpg.npz: ENVELOPE_MORL_file/ENVELOPE_DDPG.py run by make_envelope_ddpg_golden.py).  Every call trains on
the rows and preference vectors the reference drew.  There is no argmax here, so no margin condition and no row left out."""
import os

import numpy as np
import pytest

from tests import envelope_ddpg_oracle as eo
from tests.golden import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = (("actor", "actor"), ("critic", "critic"), ("actor_target", "actor_t"), ("critic_target", "critic_t"))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "envelope_ddpg.npz")))


def run_golden(fx, name, dtype=np.float32):
    c = eo.case(name)
    inp = eo.inputs(c, seed=int(fx[name + "/seed"]))
    inp["idx"], inp["weights"] = list(fx[name + "/idx"]), list(fx[name + "/weights"])
    return c, eo.run(c, inp, dtype=dtype)


def check_state(fx, name, o, c):
    for key, attr in NETS:
        synth.check_digest(name + "/" + key, getattr(o, attr), fx, rtol=2e-4, atol=2e-6, label=name)
    # Adam's first moment: a bias gradient is a sum over the rows with cancellation (test_sacd_oracle.py's rule)
    synth.check_digest(name + "/actor_m", o.aopt.m, fx, rtol=5e-3, atol=2e-5, label=name)
    synth.check_digest(name + "/critic_m", o.copt.m, fx, rtol=5e-3, atol=2e-5, label=name)
    assert int(fx[name + "/actor_step"]) == o.aopt.t == c["n_learn"] == o.copt.t == int(fx[name + "/critic_step"])


@pytest.mark.parametrize("name", list(eo.CASES))
def test_oracle_matches_reference(fx, name):
    c, (o, closs, aloss) = run_golden(fx, name)
    assert fx[name + "/idx"].shape == (c["n_learn"], c["batch"]) and fx[name + "/weights"].shape == (c["n_learn"], c["weight_num"], c["rdim"])
    np.testing.assert_allclose(closs, fx[name + "/critic_loss"], rtol=1e-5)
    np.testing.assert_allclose(aloss, fx[name + "/actor_loss"], rtol=1e-5)
    np.testing.assert_allclose(o.critic_norms, fx[name + "/critic_norm"], rtol=1e-4)
    np.testing.assert_allclose(o.actor_norms, fx[name + "/actor_norm"], rtol=1e-4)
    check_state(fx, name, o, c)


def assert_within_gpu_tolerances(a, b, label):
    """The GPU test's rule for a net (rtol 5e-4, atol 5e-6) with NO element excused."""
    for k in a:
        d = np.abs(a[k] - b[k])
        assert np.all(d <= 5e-6 + 5e-4 * np.abs(b[k])), "%s/%s: max |diff| %.3g" % (label, k, d.max())


@pytest.mark.parametrize("name", list(eo.CASES) + ["class"])
def test_float64_mode_agrees(fx, name):
    """float64 mode against float32 mode within the GPU test's tolerances: losses (1e-4, 1e-6); every element of the four nets
    within (5e-4, 5e-6) — the 1 % allowance of the GPU test is not used by these inputs; Adam m by _assert_m's rule."""
    if name == "class":
        c, o64, _, _, l64 = replay_class(fx, np.float64)
        _, o32, _, _, l32 = replay_class(fx)
        l64, l32 = np.array(l64), np.array(l32)
    else:
        c, (o64, c64, a64) = run_golden(fx, name, dtype=np.float64)
        _, (o32, c32, a32) = run_golden(fx, name)
        l64, l32 = np.stack([c64, a64], 1), np.stack([c32, a32], 1)
        np.testing.assert_allclose(c64, fx[name + "/critic_loss"], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(a64, fx[name + "/actor_loss"], rtol=1e-4, atol=1e-6)
    assert l64.dtype == np.float64 and o64.critic["l1.weight"].dtype == np.float64
    np.testing.assert_allclose(l32, l64, rtol=1e-4, atol=1e-6)
    for _, attr in NETS:
        assert_within_gpu_tolerances(getattr(o32, attr), getattr(o64, attr), name + " " + attr)
    for m32, m64 in ((o32.aopt.m, o64.aopt.m), (o32.copt.m, o64.copt.m)):
        for k in m32:
            scale = float(np.abs(m64[k]).max())
            d = np.abs(m32[k] - m64[k]).reshape(-1)
            if d.size < 2048:
                assert d.max() <= 2e-2 * scale, k
            else:
                assert np.quantile(d, 0.99) <= 2e-3 * scale and d.max() <= 5e-2 * scale, k


def test_fixture_exercises_both_clips(fx):
    """The critic's clip is on for some calls and off for others; the scaled-head case turns the actor's on; elsewhere the actor's
    norm stays below 0.5, so both branches of both clips are compared against the reference."""
    cn = np.concatenate([fx[n + "/critic_norm"] for n in eo.CASES])
    assert (cn > eo.CLIP).any() and (cn < eo.CLIP).any()
    assert eo.CASES["scaled_head"]["critic_head_scale"] > 1 and (fx["scaled_head/actor_norm"] > eo.CLIP).any()
    assert (fx["o5_a3_r2/actor_norm"] < eo.CLIP).all()


def replay_class(fx, dtype=np.float32):
    """The class case's script on the oracle, with the preference vectors and sampled rows the reference drew."""
    c = eo.case("class")
    inp = eo.inputs(c, seed=int(fx["class/seed"]))
    t, o = inp["table"], eo.make(c, inp, dtype)
    pref, learn_at = fx["class/pref"], eo.class_schedule(c)
    actions, prios, losses = [], [], []
    for i in range(c["n_steps"]):
        actions.append(o.choose(t["obs"][i], pref[2 * i]))
        o.add(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]))
        prios.append(o.priority(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"], pref[2 * i + 1]))
        if i in learn_at:
            k = len(losses)
            losses.append(o.learn_with(fx["class/idx"][k], fx["class/weights"][k], c["gamma"], c["tau"], fx["class/beta"][i]))
    return c, o, np.array(actions), np.array(prios), losses


def test_class_case(fx):
    c, o, actions, prios, losses = replay_class(fx)
    assert len(fx["class/pref"]) == 2 * c["n_steps"] and c["n_steps"] > c["capacity"]       # the ring wraps
    assert len(losses) == c["n_learn"] and eo.class_schedule(c)[4] >= c["capacity"]         # ... and half the calls come after
    np.testing.assert_allclose(actions, fx["class/action"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(prios, fx["class/priority"], rtol=1e-4)
    np.testing.assert_allclose(fx["class/final_priority"], fx["class/priority"][-c["capacity"]:], rtol=0)    # the deque: oldest first
    np.testing.assert_allclose([x[0] for x in losses], fx["class/critic_loss"], rtol=1e-5)
    np.testing.assert_allclose([x[1] for x in losses], fx["class/actor_loss"], rtol=1e-5)
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
    assert done.sum() >= 2
