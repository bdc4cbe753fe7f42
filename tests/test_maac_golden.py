"""CPU: the NumPy oracle of MAAC (tests/maac_oracle.py) against the recording of the imported reference class (tests/golden/maac.npz, made
by tests/golden/make_maac_golden.py from MAAC_file/MAAC_discrete.py + Attention.py in float32 on the CPU): the cases pair, hetero, spread3
and spread5 after 1 and 3 learn() calls — both losses and both pre-clip norms per agent and call, every online and target net, Adam's
first moments, the critic optimisers' step counts.  Tolerances are the project's (maac_oracle.TOL).  And every other reading of the
reference that the oracle can switch to MISSES the recording: what the recording pins is the reference's, not one reading of it."""
import os

import numpy as np
import pytest

from tests import maac_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maac.npz")
CASES = ("pair", "hetero", "spread3", "spread5")
ACTOR_KEYS = [n + s for n in mo.ACTOR_NAMES for s in (".weight", ".bias")]


@pytest.fixture(scope="module")
def rec():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _m_check(m, keys, stats, sample, label):
    """Adam's first moments: within TOL['m'] of the tensor's largest recorded |m| (a tensor whose gradient is exactly zero stays zero)"""
    got_stats, got_sample = mo.digest_keys(m, keys)
    for t, k in enumerate(keys):
        scale = float(np.abs(sample[t]).max())
        if stats[t, 1] == 0.0:
            assert not np.asarray(m[k]).any(), label + " " + k
            continue
        assert np.max(np.abs(got_sample[t] - sample[t])) <= mo.TOL["m"] * scale, label + " " + k
        assert abs(got_stats[t, 1] - stats[t, 1]) <= mo.TOL["m"] * stats[t, 1], label + " " + k + " abs-sum"


def _hold(name, rec, dtype, **sw):
    """run the oracle on the case and hold it to the recording; raises AssertionError where it misses"""
    c = mo.case(name)
    inp = mo.inputs(c)
    n = len(c["dims"])
    assert np.array_equal(rec[name + "/idx"], np.stack(inp["idx"]))
    am = max(a for _, a in c["dims"])
    assert np.array_equal(rec[name + "/eps"], np.stack([mo.pad_eps(inp["eps"][k], n, c["batch"], am) for k in range(c["n_learn"])]))
    o = mo.make(c, inp, dtype, **sw)
    (lr, la), nr, (pr, pa) = mo.TOL["loss"], mo.TOL["norm"], mo.TOL["param"]
    for call in range(c["n_learn"]):
        out = o.learn_with(inp["idx"][call], inp["eps"][call], c["gamma"], c["tau"])
        lab = "%s call %d" % (name, call + 1)
        np.testing.assert_allclose(np.array(out["critic_loss"], np.float64), rec[name + "/critic_loss"][call], rtol=lr, atol=la, err_msg=lab + " critic loss")
        np.testing.assert_allclose(np.array(out["actor_loss"], np.float64), rec[name + "/actor_loss"][call], rtol=lr, atol=la, err_msg=lab + " actor loss")
        np.testing.assert_allclose(out["critic_norm"], rec[name + "/critic_norm"][call], rtol=nr, err_msg=lab + " critic norm")
        np.testing.assert_allclose(out["actor_norm"], rec[name + "/actor_norm"][call], rtol=nr, err_msg=lab + " actor norm")
        if call + 1 not in mo.RECORD_AFTER:
            continue
        for j in range(n):
            pre = "%s/after%d/%d/" % (name, call + 1, j)
            for key, p, keys in (("actor", o.actor[j], ACTOR_KEYS), ("actor_target", o.actor_t[j], ACTOR_KEYS),
                                 ("critic", o.critic(j), mo.CRITIC_KEYS), ("critic_target", o.critic(j, True), mo.CRITIC_KEYS)):
                mo.check_keys(p, keys, rec[pre + key + "/stats"], rec[pre + key + "/sample"], pr, pa, lab + " agent %d %s" % (j, key))
            _m_check(o.aopt[j].m, ACTOR_KEYS, rec[pre + "actor_m/stats"], rec[pre + "actor_m/sample"], lab + " agent %d actor m" % j)
            _m_check(o.copt[j].m, mo.TRAINED_KEYS, rec[pre + "critic_m/stats"], rec[pre + "critic_m/sample"], lab + " agent %d critic m" % j)
            # n optimisers on one block: after k calls every agent's reports step k for attention.query.weight
            assert int(rec[pre + "critic_step"]) == call + 1 == o.copt[j].t


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", CASES)
def test_oracle_against_the_recorded_reference(name, dtype, rec):
    _hold(name, rec, dtype)


def test_frozen_tensors_in_the_recording(rec):
    """the reference left encoder_fc_sa, encoder_fc_a, bias_fc1, bias_fc2 of every agent as loaded: their recorded digests after 3 calls are
    those of the inputs, bit for bit"""
    for name in CASES:
        c = mo.case(name)
        inp = mo.inputs(c)
        for j in range(len(c["dims"])):
            stats, sample = mo.digest_keys(mo.critic_params(inp, j), mo.CRITIC_KEYS)
            rs, rsm = rec["%s/after3/%d/critic/stats" % (name, j)], rec["%s/after3/%d/critic/sample" % (name, j)]
            # (pair: one other agent, the softmax is 1, so the query's and the key's gradients are exactly zero and Adam leaves them too)
            still = mo.FROZEN_KEYS + (["attention.query.weight", "attention.key.weight"] if len(c["dims"]) == 2 else [])
            for t, k in enumerate(mo.CRITIC_KEYS):
                same = np.array_equal(stats[t], rs[t]) and np.array_equal(sample[t], rsm[t])
                assert same == (k in still), (name, j, k)


@pytest.mark.parametrize("switch", ["own_attention", "final_attention", "one_draw", "stale_actors", "detach_probs"])
def test_other_readings_miss_the_recording(switch, rec):
    missed = []
    for name in ("hetero", "spread3"):
        try:
            _hold(name, rec, np.float64, **{switch: True})
        except AssertionError:
            missed.append(name)
    assert missed, "the recording does not tell %s from the reference" % switch
