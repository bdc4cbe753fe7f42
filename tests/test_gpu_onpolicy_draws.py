"""GPU: the draws of a `perms=None` on-policy learn call, held bit for bit.  tests/golden/onpolicy_draws.npz was recorded from the
library as it stood before the calls' host halves moved into csrc/onpolicy_plan.hpp (tests/golden/make_onpolicy_draws_golden.py); a call
must still take the same rng_counter values in the same order and hand the same permutations — ppo_perm_kernel's up to 8192 rows, the
host shuffle's past them, HAPPO's visiting order behind either — to the same kernels.

The cases (tests/onpolicy_draws_cases.py) are the smallest at which the draw path can go wrong: each entry point at horizon 40 in
minibatches of 16 (a ragged last one) and at horizon 8193 in one minibatch; hidden 32, two learners, two agents, K = 1.  Equality is
exact: same kernels, same inputs, same row order.  A second engine with another seed must differ, or the comparison would say nothing
about the draws."""
import os

import numpy as np
import pytest

from tests import onpolicy_draws_cases as oc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "onpolicy_draws.npz")


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def test_the_fixture_holds_every_case(fx):
    assert set(fx) == {oc.name(*c) for c in oc.CASES} and len(oc.CASES) == 8


@pytest.mark.parametrize("entry,T,mb", oc.CASES, ids=[oc.name(*c) for c in oc.CASES])
def test_draws_are_the_recorded_ones(N, fx, entry, T, mb):
    want = fx[oc.name(entry, T, mb)]
    got = oc.run(N, entry, T, mb)
    other = oc.run(N, entry, T, mb, seed=oc.OTHER_SEED)
    print("%s: %d of %d floats differ from the fixture; %d differ under seed %d" % (
        oc.name(entry, T, mb), np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)), want.size, np.count_nonzero(got != other), oc.OTHER_SEED))
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, other)


@pytest.mark.parametrize("entry", oc.ENTRIES)
def test_a_minibatch_of_zero_reaches_the_librarys_refusal(N, entry):
    """with the loss trace wanted, the wrapper sizes it from ceil(horizon / minibatch): a minibatch of 0 must get the library's refusal by
    name, not a ZeroDivisionError of the wrapper's own"""
    e = oc._engine(N, entry, 40, 16, oc.SEED)
    try:
        with pytest.raises(N.FrlError, match=r"minibatch 0 outside \[1,16\]"):
            if entry == "gail_ppo":
                e.gail_ppo_learn(40, 0, oc.K, lam=0.95, ent_weight=0.01, value_loss_coef=0.5, p_lr=3e-4, v_lr=3e-4, want=("trace",), **oc.HYPER)
            else:
                learn = dict(ppo=e.ppo_learn, mappo=e.mappo_learn, happo=e.happo_learn)[entry]
                learn(40, 0, oc.K, lmbda=0.95, ent_coef=0.01, actor_lr=3e-4, critic_lr=3e-4, want_trace=True, **oc.HYPER)
    finally:
        e.close()
