"""CPU: the NumPy restatement of discrete SAC (tests/sacd_oracle.py) against the reference's outputs
(tests/golden/sac_discrete.npz, long_sac_discrete.npz: SAC_file/SAC_add_discrete.py run by make_sacd_golden.py)."""
import os

import numpy as np
import pytest

from tests import sacd_oracle as so
from tests.golden import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "sac_discrete.npz")))


@pytest.mark.parametrize("name", list(so.CASES))
def test_oracle_matches_reference(fx, name):
    c = so.case(name)
    o, losses, alphas = so.run(c, so.inputs(c))
    for k, col in (("loss_critic", 0), ("loss_actor", 1), ("loss_alpha", 2)):
        np.testing.assert_allclose(losses[:, col], fx[name + "/" + k], rtol=1e-4, atol=1e-7, err_msg=k)
    np.testing.assert_allclose(alphas, fx[name + "/alpha"], rtol=1e-5)
    assert np.float32(o.target_entropy) == fx[name + "/target_entropy"]
    for net, p in (("actor", o.actor), ("critic", o.critic), ("actor_target", o.actor_t), ("critic_target", o.critic_t)):
        synth.check_digest(name + "/" + net, p, fx, rtol=2e-4, atol=2e-6, label=name)
    # Adam's first moment: a bias gradient is a sum over the batch with cancellation, rounding shows at ~1e-2 of its scale
    # (seen: o11_a20 critic l4.bias, 5.8e-6 of an m of ~1e-3)
    for net, p in (("actor_m", o.actor_opt.m), ("critic_m", o.critic_opt.m)):
        synth.check_digest(name + "/" + net, p, fx, rtol=5e-3, atol=2e-5, label=name)
    assert int(fx[name + "/critic_step"]) == o.critic_opt.t == c["n_learn"]


def test_long_curve():
    """200 calls: the oracle stays with the reference's loss curve over all of it (measured: critic and actor losses within
    2.5e-7 relative at every call; float32 on both sides, summation orders differ), held here to 1e-5."""
    g = np.load(os.path.join(GOLDEN, "long_sac_discrete.npz"))
    c = so.case("long")
    _, losses, alphas = so.run(c, so.inputs(c))
    np.testing.assert_allclose(losses[:, 0], g["loss_critic"], rtol=1e-5)
    np.testing.assert_allclose(losses[:, 1], g["loss_actor"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(losses[:, 2], g["loss_alpha"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(alphas, g["alpha"], rtol=1e-6)
