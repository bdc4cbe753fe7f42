"""CPU: the NumPy restatement of HAPPO's learn (tests/happo_oracle.py) against the reference's recorded outputs
(tests/golden/happo.npz) on every case the reference runs: advantages and value targets to rtol 1e-5 / atol 2e-6, the loss of every
step and the factors of every visiting position to rtol 1e-4 / atol 1e-6 (the loss is linear in the factors), final parameters by
the project's parameter rule, Adam's moments and step counts; the recorded order and permutations; and the stored facts about the two
discrete cases in which the reference raises."""
import os

import numpy as np
import pytest

from tests import happo_oracle as ho
from tests import mappo_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "happo.npz")
tol = ho.tol          # the project's tolerances; happo_c_hot's own are derived in tests/happo_oracle.py


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def runs(fx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ho.run(ho.case(name), fx[name + "/order"])
        return cache[name]
    return get


RECORDED = [k for k, c in ho.CASES.items() if not c["ref_raises"]]


@pytest.mark.parametrize("name", RECORDED)
def test_oracle_against_reference(fx, runs, name):
    c, o = ho.case(name), runs(name)
    n, steps = len(c["dims"]), c["k_epochs"] * -(-c["horizon"] // c["minibatch"])
    order = fx[name + "/order"]
    assert sorted(order) == list(range(n)) and not bool(fx[name + "/ref_raises"])
    if c["order"] is not None:
        assert tuple(order) == c["order"]
    assert np.array_equal(fx[name + "/perms"], ho.perms(c, order))
    np.testing.assert_allclose(o.adv_raw, fx[name + "/adv"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(o.v_target, fx[name + "/v_target"], rtol=1e-5, atol=2e-6)
    rt, at = tol(name, "trace")
    np.testing.assert_allclose(o.trace, fx[name + "/trace"], rtol=rt, atol=at)
    rt, at = tol(name, "factor")
    assert o.factors.shape == fx[name + "/factor"].shape == (n, c["horizon"]) and np.all(o.factors[0] == 1)
    np.testing.assert_allclose(o.factors, fx[name + "/factor"], rtol=rt, atol=at)
    rt, at = tol(name, "param")
    for i in range(n):
        for tag, p, opt, lr in (("actor", o.actors[i], o.aopt[i], c["actor_lr"]), ("critic", o.critics[i], o.copt[i], c["critic_lr"])):
            key = "%s/%d/%s" % (name, i, tag)
            assert opt.t == steps == int(fx[key + "/step"])
            dg = fx[key + "/digest"]
            if key + "/p" in fx:
                mo.assert_net(mo.flat(c, tag, p), fx[key + "/p"], lr, steps, key, rtol=rt, atol=at)
            mo.assert_digest(mo.flat(c, tag, p), dg[0], key + " parameters", rtol=rt, atol=at)
            mo.assert_digest(mo.flat(c, tag, opt.m), dg[1], key + " m", rtol=2e-3, atol=1e-7)
            mo.assert_digest(mo.flat(c, tag, opt.v), dg[2], key + " v", rtol=4e-3, atol=1e-9)


def test_conditions_recorded(fx):
    """what the golden maker enforced at recording time, on the reference's numbers"""
    for name in RECORDED:
        c = ho.case(name)
        if c["cont"] and len(c["dims"]) == 3:
            assert float(fx[name + "/frac_far"]) >= 0.5, name
        if c["trick"]["huber_loss"] and c["huber_delta"] < 1:
            assert ((fx[name + "/frac_small"] >= 0.1) & (fx[name + "/frac_small"] <= 0.9)).all(), name
    a, b = "happo_c_order_a", "happo_c_order_b"
    assert np.array_equal(fx[a + "/adv"], fx[b + "/adv"])                       # the same inputs ...
    for i in range(3):
        assert not np.array_equal(fx["%s/%d/actor/p" % (a, i)], fx["%s/%d/actor/p" % (b, i)])      # ... another order, other actors


def test_reference_raises_on_discrete_minibatches(fx, runs):
    """HAPPO.py:449-453 on 3 agents, T 40, minibatch 16: RuntimeError in the reference (recorded), so these two cases' expected values
    are this oracle's; it runs them to the end, finite, with factors that moved"""
    for name in ("happo_d_plain", "happo_d_tricks"):
        assert bool(fx[name + "/ref_raises"]) and name + "/trace" not in fx
        o = runs(name)
        assert np.isfinite(o.trace).all() and np.isfinite(o.factors).all()
        assert np.all(o.factors[0] == 1) and (np.abs(o.factors[-1] - 1) > 1e-3).mean() > 0.5
    assert not bool(fx["happo_d_ident/ref_raises"]) and not bool(fx["happo_d_single/ref_raises"])


def test_order_changes_the_later_actors_only(runs):
    """the first visited agent's steps do not see the factor; the later ones do"""
    o = runs("happo_c_plain")
    plain = mo.run(ho.joint(dict(ho.case("happo_c_plain"))), perm=ho.perms(ho.case("happo_c_plain"), o.order))
    first = int(o.order[0])
    # (mappo_oracle's Adam settings differ: one optimiser, eps 1e-5, no clip - so only the FIRST step's actor loss is comparable)
    assert o.trace[first, 0, 0] == plain.trace[first, 0, 0]
    assert all(o.trace[int(i), 0, 0] != plain.trace[int(i), 0, 0] for i in o.order[1:])


def test_dead_layer_stays_finite(runs):
    o = runs("happo_c_dead")
    assert np.isfinite(o.trace).all() and np.isfinite(o.factors).all()
    assert all(np.isfinite(v).all() for p in o.actors + o.critics for v in p.values())
