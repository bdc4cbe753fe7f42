"""CPU: the NumPy restatement of MAPPO_for_mask_action_state.py (tests/mappo_state_oracle.py) against the reference's recorded outputs
(tests/golden/mappo_state.npz, loop_mappo_state.npz) on every case, at tests/test_mappo_mask_oracle.py's tolerances: advantages and
value targets rtol 1e-5 / atol 2e-6, the loss of every step rtol 1e-4 / atol 1e-6, final parameters by the project's parameter rule,
Adam's moments and step counts, the recorded permutations; what the golden maker recorded about the two pairings and the zeroed state
block; the two pairings under the identity permutation; the masked sample against the reference class's episode run."""
import os

import numpy as np
import pytest

from tests import mappo_mask_oracle as mm
from tests import mappo_oracle as mo
from tests import mappo_state_oracle as ms

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mappo_state.npz")
LOOP = os.path.join(HERE, "golden", "loop_mappo_state.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def test_cases_are_the_issues():
    assert set(ms.CASES) == {"plain", "tricks", "partial", "stale", "cont", "wide", "sd1", "sd2", "sd3", "sd23"}
    assert {n: ms.CASES[n]["state_dim"] for n in ("sd1", "sd2", "sd3", "sd23", "wide", "plain")} == dict(sd1=1, sd2=2, sd3=3, sd23=23, wide=45, plain=7)
    assert sum(o for o, _ in ms.DIMS) == 14 and ms.critic_width(ms.case("wide")) == 99 and ms.case("wide")["hidden"] == 128
    assert ms.case("partial")["fill"] == 27 and ms.case("stale")["second"] == 18 and ms.case("cont")["cont"]
    assert all(ms.case("tricks")["trick"][k] for k in mo.TRICKS_ON)
    for name, c in ms.CASES.items():
        assert c["minibatch"] == c["horizon"] == (64 if name == "wide" else 40) and c["k_epochs"] == (1 if name == "wide" else 2)
    assert os.path.getsize(GOLDEN) < 1 << 20 and os.path.getsize(LOOP) < 1 << 20


@pytest.mark.parametrize("name", list(ms.CASES))
def test_oracle_against_reference(fx, name):
    c = ms.case(name)
    o = ms.run(c)
    n, steps = len(c["dims"]), c["k_epochs"] * ms.calls(c)
    assert np.array_equal(fx[name + "/perms"], ms.perms(c))
    np.testing.assert_allclose(o.adv_raw, fx[name + "/adv"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(o.v_target, fx[name + "/v_target"], rtol=1e-5, atol=2e-6)
    assert o.trace.shape == fx[name + "/trace"].shape == (n, steps, 2)
    np.testing.assert_allclose(o.trace, fx[name + "/trace"], rtol=1e-4, atol=1e-6)
    for i in range(n):
        for tag, p, opt, lr in (("actor", o.actors[i], o.aopt[i], c["actor_lr"]), ("critic", o.critics[i], o.copt[i], c["critic_lr"])):
            key = "%s/%d/%s" % (name, i, tag)
            assert opt.t == steps == int(fx[key + "/step"])
            dg = fx[key + "/digest"]
            if key + "/p" in fx:
                mo.assert_net(mo.flat(c, tag, p), fx[key + "/p"], lr, steps, key)
            mo.assert_digest(mo.flat(c, tag, p), dg[0], key + " parameters")
            mo.assert_digest(mo.flat(c, tag, opt.m), dg[1], key + " m", rtol=2e-3, atol=1e-7)
            mo.assert_digest(mo.flat(c, tag, opt.v), dg[2], key + " v", rtol=4e-3, atol=1e-9)


@pytest.mark.parametrize("name", list(ms.CASES))
def test_pairing_and_state_block_are_observable(fx, name):
    """the reference's first critic loss is the POSITION pairing's, and further than 1e-3 relative - ten times the loss tolerance - from
    the SAMPLE pairing's and from the loss with the state block zeroed (recorded by the maker on the reference's numbers)"""
    c = ms.case(name)
    ref = fx[name + "/trace"][:, 0, 1]
    sample, zeroed = fx[name + "/first_critic_loss_sample"], fx[name + "/first_critic_loss_zero_state"]
    assert (np.abs(ref - sample) > 1e-3 * np.abs(ref)).all() and (np.abs(ref - zeroed) > 1e-3 * np.abs(ref)).all()
    np.testing.assert_allclose(ms.run(c, calls_max=1).trace[:, 0, 1], ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ms.run(dict(c, state_rows="sample"), calls_max=1).trace[:, 0, 1], sample, rtol=1e-6)
    np.testing.assert_allclose(ms.run(c, calls_max=1, zero_state=True).trace[:, 0, 1], zeroed, rtol=1e-6)


@pytest.mark.parametrize("name", ["tricks", "stale", "sd3"])
def test_pairings_agree_exactly_under_the_identity_permutation(name):
    c = ms.case(name)
    ident = np.broadcast_to(np.arange(c["horizon"]), ms.perms(c).shape).copy()
    a, b = ms.run(c, perm=ident), ms.run(dict(c, state_rows="sample"), perm=ident)
    assert np.array_equal(a.trace, b.trace) and np.array_equal(a.v_target, b.v_target)
    for i in range(len(c["dims"])):
        assert np.array_equal(mo.flat(c, "critic", a.critics[i]), mo.flat(c, "critic", b.critics[i]))
        assert np.array_equal(mo.flat(c, "actor", a.actors[i]), mo.flat(c, "actor", b.actors[i]))
    # ... and not under the case's own permutations
    assert not np.array_equal(ms.run(c).trace[:, :, 1], ms.run(dict(c, state_rows="sample")).trace[:, :, 1])


def test_sample_pairing_takes_short_minibatches_and_position_does_not():
    c = ms.case("plain", state_rows="sample", minibatch=16)
    o = ms.run(c)
    assert o.trace.shape == (3, 2 * 3, 2) and np.isfinite(o.trace).all()
    with pytest.raises(AssertionError, match="torch.cat raises"):
        ms.run(ms.case("plain", minibatch=16))


def test_case_conditions():
    """what the golden maker enforced at recording time, restated on the seeded inputs: the masks' and the stored actions' conditions, and
    states that are i.i.d. per row and equal to no observation"""
    for name in ms.CASES:
        c = ms.case(name)
        fill = c["horizon"] if c["fill"] is None else c["fill"]
        inp = ms.inputs(c)
        sets = [(inp["rows"], inp["state"], fill)]
        if c["second"]:
            rows, st = ms.second_rows(c)
            sets.append((rows, st, c["second"]))
        for rows, state, count in sets:
            assert state.shape[1] == c["state_dim"] and len(np.unique(state[:count], axis=0)) == count
            assert not any(np.isin(state[:count], r["obs"]).any() for r in rows)
            for (O, A), r in zip(c["dims"], rows):
                k = r["mask"][:count].sum(axis=1)
                assert ((k >= 2) & (k <= A - 1)).mean() >= 0.5
                if not c["cont"]:
                    assert r["mask"][np.arange(count), r["act"][:count, 0].astype(int)].all()
        assert not ms.ring_state(c, inp)[fill:].any()
    frac = dict(np.load(GOLDEN))["tricks/frac_small"]
    assert ((frac >= 0.1) & (frac <= 0.9)).all()


def test_toy_env_state_and_the_reference_loop():
    """ToyEnv.get_state() follows the step; the reference class's first episode (parameters not yet updated) from the recorded draws"""
    fx = dict(np.load(LOOP))
    c, env = ms.LOOP, ms.ToyEnv()
    assert env.get_state().shape == (c["state_dim"],) and np.array_equal(env.get_state(), env.state[0])
    env.step({a: 0 for a in env.agents}, False)
    assert np.array_equal(env.get_state(), env.state[1])
    env = ms.ToyEnv()
    inp = ms.inputs(c)
    assert float(fx["min_margin"]) >= 1e-3 and fx["actions"].shape == (sum(ms.LOOP_EPISODES), len(c["dims"]))
    for i, (O, A) in enumerate(c["dims"]):
        T = ms.LOOP_EPISODES[0]
        logits = mo.forward(inp["actors"][i], mo.ACTOR_D, env.obs[i][:T], c["trick"])[0]
        a, lp, margin = mm.sample(logits, env.mask[i][:T], fx["q/%d" % i][:T])
        assert np.array_equal(a, fx["actions"][:T, i])
        np.testing.assert_allclose(lp, fx["logp"][:T, i], rtol=1e-4, atol=1e-6)
