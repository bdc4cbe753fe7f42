"""CPU: the NumPy restatement of MAPPO_for_mask_action.py (tests/mappo_mask_oracle.py) against the reference's recorded outputs
(tests/golden/mappo_mask.npz, loop_mappo_mask.npz) on every case: advantages and value targets to rtol 1e-5 / atol 2e-6, the loss of
every step to rtol 1e-4 / atol 1e-6, final parameters by the project's parameter rule, Adam's moments and step counts, the recorded
permutations; the normalisation order that the `partial` case decides; the masked sample against the reference class's episode run."""
import os

import numpy as np
import pytest

from tests import mappo_mask_oracle as mm
from tests import mappo_oracle as mo

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mappo_mask.npz")
LOOP = os.path.join(HERE, "golden", "loop_mappo_mask.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", list(mm.CASES))
def test_oracle_against_reference(fx, name):
    c = mm.case(name)
    o = mm.run(c)
    n, steps = len(c["dims"]), c["k_epochs"] * mm.calls(c)
    assert np.array_equal(fx[name + "/perms"], mm.perms(c))
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


def test_partial_decides_the_normalisation_order(fx):
    """13 rows never written: all-closed masks.  torch's l = z' - (max + log sum) makes their logits exactly 0 (ratio 1); the other order
    gives -log A (ratio 1 / A) and another first actor loss, by more than 1e-3 relative (recorded by the maker on the reference's numbers)"""
    c = mm.case("partial")
    z = np.random.Generator(np.random.PCG64(3)).normal(0, 1, (4, 5)).astype(np.float32)
    closed = np.zeros((4, 5), bool)
    l, p, ent = mm.masked_dist(z, closed)
    assert np.all(l == 0) and np.all(p == np.float32(0.2)) and np.all(ent == 0)
    np.testing.assert_allclose(mm.masked_logits(z, closed, torch_order=False), -np.log(5.0), rtol=1e-6)
    ref = fx["partial/trace"][:, 0, 0]
    other = fx["partial/first_actor_loss_other_order"]
    assert (np.abs(ref - other) > 1e-3 * np.abs(ref)).all()
    ours = mm.run(c).trace[:, 0, 0]
    wrong = mm.run(c, torch_order=False).trace[:, 0, 0]
    np.testing.assert_allclose(ours, ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(wrong, other, rtol=1e-6)
    assert (np.abs(wrong - ref) > 1e-3 * np.abs(ref)).all()


def test_case_conditions():
    """what the golden maker enforced at recording time, restated on the seeded inputs"""
    for name in mm.CASES:
        c = mm.case(name)
        fill = c["horizon"] if c["fill"] is None else c["fill"]
        for rows, count in [(mm.inputs(c)["rows"], fill)] + ([(mm.second_rows(c), c["second"])] if c["second"] else []):
            for (O, A), r in zip(c["dims"], rows):
                k = r["mask"][:count].sum(axis=1)
                if c["edges"]:
                    assert (k == 1).any() and (k == A).any() and ((k == 1) | (k == A)).all()
                else:
                    assert ((k >= 2) & (k <= A - 1)).mean() >= 0.5
                if not c["cont"]:
                    assert r["mask"][np.arange(count), r["act"][:count, 0].astype(int)].all()


def test_edges_rows():
    """exactly one open action: p = 1, zero entropy, zero head delta whatever the advantage; the oracle's gradient is zero there"""
    z = np.array([[0.3, -1.0, 2.0, 0.5]], np.float32)
    mask = np.array([[False, True, False, False]])
    l, p, ent = mm.masked_dist(z, mask)
    assert l[0, 1] == 0 and p[0, 1] == 1 and ent[0, 0] == 0 and np.all(p[0, [0, 2, 3]] == 0)


def test_masked_sample_against_the_reference_loop():
    """the reference class's first episode (parameters not yet updated): actions and log-probs from the recorded Exp(1) draws"""
    fx = dict(np.load(LOOP))
    c, env = mm.LOOP, mm.ToyEnv()
    inp = mm.inputs(c)
    assert float(fx["min_margin"]) >= 1e-3 and fx["actions"].shape == (sum(mm.LOOP_EPISODES), len(c["dims"]))
    for i, (O, A) in enumerate(c["dims"]):
        T = mm.LOOP_EPISODES[0]
        logits = mo.forward(inp["actors"][i], mo.ACTOR_D, env.obs[i][:T], c["trick"])[0]
        a, lp, margin = mm.sample(logits, env.mask[i][:T], fx["q/%d" % i][:T])
        assert np.array_equal(a, fx["actions"][:T, i])
        np.testing.assert_allclose(lp, fx["logp"][:T, i], rtol=1e-4, atol=1e-6)
        assert env.mask[i][np.arange(T), a].all() and env.mask[i][:, A - 1].all()
