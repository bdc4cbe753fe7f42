"""CPU: the NumPy restatement of MAPPO / IPPO's learn (tests/mappo_oracle.py) against the reference's recorded outputs
(tests/golden/mappo.npz) on every case: advantages and value targets to rtol 1e-5, the loss of every step to rtol 1e-4 / atol 1e-6,
final parameters by the project's parameter rule (tests/mappo_oracle.py: assert_net), Adam's moments and step counts."""
import os

import numpy as np
import pytest

from tests import mappo_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mappo.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mo.run(mo.case(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(mo.CASES))
def test_oracle_against_reference(fx, runs, name):
    c, o = mo.case(name), runs(name)
    n, steps = len(c["dims"]), c["k_epochs"] * -(-c["horizon"] // c["minibatch"])
    assert np.array_equal(fx[name + "/perms"], mo.perms(c))
    # (adv's atol: an advantage is a sum of up to ten discounted TD errors of size ~1, each carrying fp32 rounding; one near zero has no relative accuracy)
    np.testing.assert_allclose(o.adv_raw, fx[name + "/adv"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(o.v_target, fx[name + "/v_target"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(o.trace, fx[name + "/trace"], rtol=1e-4, atol=1e-6)
    for i in range(n):
        for tag, p, opt, lr in (("actor", o.actors[i], o.aopt[i], c["actor_lr"]), ("critic", o.critics[i], o.copt[i], o.critic_lr)):
            key = "%s/%d/%s" % (name, i, tag)
            assert opt.t == steps == int(fx[key + "/step"])
            dg = fx[key + "/digest"]
            if key + "/p" in fx:
                mo.assert_net(mo.flat(c, tag, p), fx[key + "/p"], lr, steps, key)
            mo.assert_digest(mo.flat(c, tag, p), dg[0], key + " parameters")
            mo.assert_digest(mo.flat(c, tag, opt.m), dg[1], key + " m", rtol=2e-3, atol=1e-7)
            mo.assert_digest(mo.flat(c, tag, opt.v), dg[2], key + " v", rtol=4e-3, atol=1e-9)


def test_conditions_recorded(fx):
    """what the golden maker enforced at recording time, on the reference's numbers"""
    for name in mo.CASES:
        c = mo.case(name)
        if c["trick"]["huber_loss"] and c["huber_delta"] < 1:
            assert ((fx[name + "/frac_small"] >= 0.1) & (fx[name + "/frac_small"] <= 0.9)).all(), name
        if c["trick"]["ValueClip"]:
            assert (fx[name + "/frac_clamped"] >= 0.25).all(), name


def test_value_clip_changes_nothing(fx, runs):
    """MAPPO.py:422-431: the clamped loss never exceeds the original, so the step and the reported loss are the unclipped ones': in the
    reference's own runs (bit for bit) and in the oracle, which computes the clamp literally"""
    a, b = "mappo_c_vclip", "mappo_c_vclip_off"
    assert np.array_equal(fx[a + "/trace"], fx[b + "/trace"])
    for i in range(3):
        for tag in ("actor", "critic"):
            assert np.array_equal(fx["%s/%d/%s/digest" % (a, i, tag)], fx["%s/%d/%s/digest" % (b, i, tag)])
    oa, ob = runs(a), runs(b)
    assert np.array_equal(oa.trace, ob.trace)
    for i in range(3):
        assert all(np.array_equal(oa.critics[i][k], ob.critics[i][k]) for k in oa.critics[i])


def test_dead_layer_stays_finite(runs):
    for name in ("mappo_c_dead", "ippo_d_dead"):
        o = runs(name)
        assert np.isfinite(o.trace).all()
        assert all(np.isfinite(v).all() for p in o.actors + o.critics for v in p.values())
