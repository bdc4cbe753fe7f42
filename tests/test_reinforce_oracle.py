"""CPU: the NumPy restatement of REINFORCE (tests/reinforce_oracle.py) against the reference's outputs
(tests/golden/reinforce.npz, long_reinforce.npz: REINFORCE_file/REINFORCE.py run by make_reinforce_golden.py).

The loss is a signed sum with cancellation, so its tolerances are stated against s = sum_t |log pi_t * g_t|, never against
the loss.  Measured on the CPU, per case, the largest over the case's calls of
    loss : |reference loss - float64 oracle loss| / s          ghat : max |float32 ghat - float64 ghat| / max |ghat|

    case         loss       ghat
    o4_a2        1.03e-07   1.09e-07
    o17_a3       1.82e-07   1.77e-07
    o8_a20       6.75e-07   1.68e-07
    o8_a4_h256   1.16e-07   1.30e-07
    multi        1.49e-07   1.45e-07
    flat         0          0            (every normalised return is exactly zero)
    clamp        2.98e-07   2.63e-07

FIGURES holds them; tests/test_gpu_reinforce.py takes its loss and returns tolerances from it (four times each).  The float32
oracle itself is within 7.8e-7 s of the reference's loss in every call, and every parameter of every case is within
rtol 5e-4 / atol 5e-6 of the reference after the case's 12 calls (the >= 99 % share the GPU test asks for is 100 % here).
"""
import os

import numpy as np
import pytest

from tests import reinforce_oracle as ro
from tests.golden import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# case -> (loss figure, ghat figure), as measured above
FIGURES = {"o4_a2": (1.03e-07, 1.09e-07), "o17_a3": (1.82e-07, 1.77e-07), "o8_a20": (6.75e-07, 1.68e-07),
           "o8_a4_h256": (1.16e-07, 1.30e-07), "multi": (1.49e-07, 1.45e-07), "flat": (0.0, 0.0), "clamp": (2.98e-07, 2.63e-07)}


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "reinforce.npz")))


@pytest.mark.parametrize("name", list(ro.CASES))
def test_oracle_matches_reference(fx, name):
    c = ro.case(name)
    inp = ro.inputs(c)
    assert c["n_learn"] >= 12
    o, outs = ro.run(c, inp)
    o64, outs64 = ro.run(c, inp, np.float64)
    ref = fx[name + "/loss"]
    for k, (r32, r64) in enumerate(zip(outs, outs64)):
        # the float32 oracle and the reference are two float32 roundings of one sum: 2e-6 of s covers both (measured 7.8e-7)
        assert abs(float(r32["loss"]) - float(ref[k])) <= 2e-6 * r64["s"], (name, k)
        # ... and the recorded figures are what this machine-independent arithmetic gives (10 % slack for libm differences)
        assert abs(float(ref[k]) - float(r64["loss"])) <= 1.1 * FIGURES[name][0] * r64["s"] + 1e-12 * (name != "flat"), (name, k)
        d = np.abs(r32["ghat"].astype(np.float64) - r64["ghat"]).max()
        assert d <= 1.1 * FIGURES[name][1] * max(np.abs(r64["ghat"]).max(), 1e-30), (name, k)
    np.testing.assert_allclose(np.concatenate([r["logp"] for r in outs]), fx[name + "/logp"], rtol=1e-5, atol=1e-5)
    synth.check_digest(name + "/policy", o.p, fx, rtol=2e-4, atol=2e-6, label=name)
    synth.check_digest(name + "/policy_m", o.m, fx, rtol=5e-3, atol=2e-5, label=name)
    assert int(fx[name + "/step"]) == o.t == c["n_learn"]
    for k, v in o.p.items():            # the share condition of the GPU test's _assert_net, oracle against reference
        want = fx["%s/policy/%s/full" % (name, k)].reshape(v.shape)
        assert (np.abs(v - want) > 5e-6 + 5e-4 * np.abs(want)).mean() <= 0.01, (name, k)


def test_flat_leaves_the_net_alone(fx):
    """All returns equal: std = 0, every normalised return 0, zero gradient — parameters, m and v stay, the step count moves."""
    c = ro.case("flat")
    inp = ro.inputs(c)
    o, outs = ro.run(c, inp)
    assert all(float(r["loss"]) == 0.0 and not r["ghat"].any() for r in outs)
    assert np.all(fx["flat/loss"] == 0)
    for k, v in o.p.items():
        np.testing.assert_array_equal(v, inp["params"][k])
        np.testing.assert_array_equal(fx["flat/policy/%s/full" % k].reshape(v.shape), inp["params"][k])
        assert not o.m[k].any() and not o.v[k].any()
        assert fx["flat/policy_m/%s/abssum" % k] == 0 and fx["flat/policy_v/%s/abssum" % k] == 0
    assert int(fx["flat/step"]) == o.t == 12


def test_clamp_rows(fx):
    """The clamped rows' log-probs in the reference are log(eps) / log(1 - eps) exactly, on both sides, in every call."""
    c = ro.case("clamp")
    inp = ro.inputs(c)
    lo, hi = np.log(np.float32(ro.EPS)), np.log(np.float32(1) - np.float32(ro.EPS))
    logp, pos = fx["clamp/logp"], 0
    for call in inp["calls"]:
        T = len(call["rew"])
        lp = logp[pos:pos + T]
        pos += T
        shut = call["obs"][:, -1] == 0
        assert (lp[shut & (call["act"] == 0)] == hi).all() and (lp[shut & (call["act"] != 0)] == lo).all()
        assert (lp[shut] == hi).any() and (lp[shut] == lo).any()
        if (~shut).any():
            assert ((lp[~shut] > lo) & (lp[~shut] < hi)).all()


def test_long_curve():
    """150 calls, T from 8..200: the float32 oracle stays with the reference's loss curve (measured: within 5.6e-7 s at every
    call; the float64 oracle within 2.6e-7 s), held to 5e-6 s."""
    g = np.load(os.path.join(GOLDEN, "long_reinforce.npz"))
    c = ro.case("long")
    inp = ro.inputs(c)
    _, outs = ro.run(c, inp)
    _, outs64 = ro.run(c, inp, np.float64)
    assert len(outs) == 150 == len(g["loss"]) and min(c["Ts"]) >= 8 and max(c["Ts"]) <= 200
    for k, (r, r64) in enumerate(zip(outs, outs64)):
        assert abs(float(r["loss"]) - float(g["loss"][k])) <= 5e-6 * r64["s"], k
