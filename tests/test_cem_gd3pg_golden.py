"""CPU: the recording of the reference (tests/golden/cem_gd3pg.npz, written by tests/golden/make_cem_gd3pg_golden.py) against the NumPy
restatement of CEM_GD3PG.learn in float32 and float64, at the project's unwidened tolerances — losses and KL rtol 1e-4 / atol 1e-6,
pre-clip norms rtol 1e-3, parameters 5e-4 / 5e-6, Adam's m within 2e-3 of a tensor's largest —, each switched oracle missing it, and
freerl_amd.CEM_GD3PG.sepCEM against the recorded sepCEM to rtol 1e-12 with the same generator state afterwards."""
import os

import numpy as np
import pytest

from tests import cem_gd3pg_oracle as co

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NORM_COLS = (1, 3, 5)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "cem_gd3pg.npz")))


def _misses(ref, got):
    """-> the worst ratio of |got - ref| to the tolerance over the compared columns (losses, norms, KL): > 1 is a miss"""
    worst = 0.0
    for col in range(7):
        rtol, atol = (1e-3, 0.0) if col in NORM_COLS else (1e-4, 1e-6)
        worst = max(worst, float(np.max(np.abs(got[:, col] - ref[:, col]) / (atol + rtol * np.abs(ref[:, col])))))
    return worst


def _inputs(fx, name):
    c = co.case(name)
    inp = co.inputs(c, seed=int(fx[name + "/seed"]))
    inp["idx"] = list(fx[name + "/idx"])
    return c, inp


def _states(o):
    out = dict(actor_1=o.actor[0], actor_2=o.actor[1], critic=o.critic, actor_1_target=o.actor_t[0], actor_2_target=o.actor_t[1], critic_target=o.critic_t,
               actor_domain=o.domain)
    for key, opt in (("actor_1", o.aopt[0]), ("actor_2", o.aopt[1]), ("critic", o.copt)):
        out[key + "_m"], out[key + "_v"] = opt.m, opt.v
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("name", list(co.CASES))
def test_oracle_matches_the_recording(fx, name, dtype):
    c, inp = _inputs(fx, name)
    ref = fx[name + "/out"]
    assert ref.shape == (c["n_learn"], 8) and np.all(ref[:, 7] == 2 * (min(c["n1"], c["batch"]) // 2))
    for calls in (1, c["n_learn"]):          # the states the generator recorded: after call 1 and after the last
        o, got = co.run(c, inp, n_learn=calls, dtype=dtype)
        assert _misses(ref[:calls], got) <= 1.0, (name, calls, got, ref[:calls])
        for key, p in _states(o).items():
            sums, sample = co.digest(p)
            want, pre = fx["%s/call%d/%s/sample" % (name, calls, key)], "%s call %d %s" % (name, calls, key)
            if key.endswith("_m"):
                assert np.max(np.abs(sample - want)) <= 2e-3 * np.max(np.abs(want)), pre
            elif key.endswith("_v"):
                np.testing.assert_allclose(sample, want, rtol=5e-3, atol=1e-3 * np.max(np.abs(want)), err_msg=pre)
            else:
                np.testing.assert_allclose(sample, want, rtol=5e-4, atol=5e-6, err_msg=pre)
                np.testing.assert_allclose(sums[:, 0], fx["%s/call%d/%s/sums" % (name, calls, key)][:, 0], rtol=0,
                                           atol=5e-4 * np.max(fx["%s/call%d/%s/sums" % (name, calls, key)][:, 1]) + 5e-6 * sample.size, err_msg=pre)
        for key in ("actor_1", "actor_2", "critic"):
            assert int(fx["%s/call%d/%s_step" % (name, calls, key)]) == calls


# (kl_ba divides by B A instead of B: the same number on a one-column action, so `pend` cannot tell it apart and is not asked to)
SWITCHED = [(n, s) for n in co.CASES for s in co.SWITCHES if not (s == "kl_ba" and co.CASES[n]["act_dim"] == 1)]


@pytest.mark.parametrize("name,switch", SWITCHED)
def test_each_switched_oracle_misses_the_recording(fx, name, switch):
    c, inp = _inputs(fx, name)
    _, got = co.run(c, inp, switches=(switch,))
    assert _misses(fx[name + "/out"], got) >= 10.0, (name, switch)


def test_the_recording_covers_what_it_claims(fx):
    """both sides of the three clips, both values of is_F1_more, rows of `buffer` that were never written"""
    crit, guided, unguided = [], [], []
    for name in co.CASES:
        c, ref = co.case(name), fx[name + "/out"]
        g = 5 if c["f1_more"] else 3
        crit += list(ref[:, 1]); guided += list(ref[:, g]); unguided += list(ref[:, 8 - g])
        assert np.all(ref[:, 6] > 0)
    for v in (crit, guided, unguided):
        assert min(v) < 0.5 < max(v), v
    assert {co.case(n)["f1_more"] for n in co.CASES} == {True, False}
    assert fx["short/idx"][:, 0].max() >= co.case("short")["n0"] and fx["short/idx"].shape == (3, 2, 15)
    assert fx["odd/idx"].shape == (3, 2, 16)          # the odd batch of 33 loses a row


def test_bound_buffer_switch_draws_other_rows(fx):
    """the first draw's bound taken from len(buffer): another stream of rows on `walker` (600 against 560), an error on `short`"""
    c, inp = _inputs(fx, "walker")
    np.random.seed(int(fx["walker/seed"]))
    i0, i1 = co.CemGd3pg(inp, c).draw(c["batch"])
    assert np.array_equal(np.stack([i0, i1]), fx["walker/idx"][0])
    np.random.seed(int(fx["walker/seed"]))
    j0, _ = co.CemGd3pg(inp, c, switches=("bound_buffer",)).draw(c["batch"])
    assert not np.array_equal(j0, i0)


# ------------------------------------------------------------------------------------ sepCEM
@pytest.mark.parametrize("name", ["pop4", "pop10", "pop5"])
def test_sepcem_matches_the_recording(fx, name):
    from freerl_amd.CEM_GD3PG import sepCEM
    got = co.sepcem_script(sepCEM, co.SEPCEM[name], co.SEPCEM_SEED)
    keys = [k[len("sepcem/%s/" % name):] for k in fx if k.startswith("sepcem/%s/" % name)]
    assert sorted(keys) == sorted(got) and len(keys) == 4 + 6 * 3
    for k in keys:
        np.testing.assert_allclose(got[k], fx["sepcem/%s/%s" % (name, k)], rtol=1e-12, atol=0, err_msg=k)
    assert got["next_uniform"] == float(fx["sepcem/%s/next_uniform" % name])          # the same generator state afterwards
