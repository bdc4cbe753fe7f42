"""GPU: three consecutive device-drawn calls of every off-policy entry point, held bit for bit.  tests/golden/offpolicy_calls.npz was
recorded from the library as it stood before the calls' host halves moved into csrc/learn_plan.hpp
(tests/golden/make_offpolicy_calls_golden.py); a call must still take the same rng_counter values in the same order, make the same
launches with the same arguments, and so train on the same rows, return the same numbers and leave the same bits in every net.

The cases (tests/offpolicy_calls_cases.py): every row of tests/test_gpu_learn_launches.py's CASES — one per kernel family and per host
decision — and the smallest call of frl_envelope_learn, frl_envelope_ddpg_learn, frl_gail_learn, frl_cem_gd3pg_learn and
frl_reinforce_learn.  Equality is exact: same kernels, same inputs, same row order; the recorder ran every case twice and found each
reproducible to the bit (the fixture's `notes` names any that was not, and what it keeps of it)."""
import os

import numpy as np
import pytest

from tests import offpolicy_calls_cases as oc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offpolicy_calls.npz")


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def test_the_fixture_holds_every_case_whole(fx):
    assert str(fx["notes"]) == "" and len(oc.NAMES) == 19
    want = {n + "/" + k for n in oc.NAMES for k in ("idx", "out", "digest")} - {"reinforce/idx"} | {"notes"}
    assert set(fx) == want


@pytest.mark.parametrize("name", oc.NAMES)
def test_calls_are_the_recorded_ones(N, fx, name):
    got = oc.run(N, name)
    keys = sorted(k.split("/")[1] for k in fx if k.startswith(name + "/"))
    assert keys == sorted(got)
    for k in keys:
        want = fx[name + "/" + k]
        print("%s/%s: %d of %d bytes differ" % (name, k, np.count_nonzero(np.frombuffer(got[k].tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))
                                               if got[k].shape == want.shape else -1, want.nbytes))
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert got[k].tobytes() == want.tobytes(), k
