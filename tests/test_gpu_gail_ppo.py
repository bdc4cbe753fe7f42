"""GPU: GAIL's policy side (GAIL_file/PPO2.py's PPO_learn) on kernels_gail_ppo.hip — an ALGO_GAIL_PPO engine through frl_gail_ppo_learn and
frl_act — against the NumPy float64 restatement (tests/gail_ppo_oracle.py) and the reference's own outputs (tests/golden/gail_ppo.npz).

Tolerances are tests/test_gpu_ppo_edges.py's for the same arithmetic, unchanged: ADV_TOL for adv_out / returns_out / logp_old_out,
ACTOR_TOL / CRITIC_TOL for the loss trace, PARAM_TOL for every parameter.  tests/test_gail_ppo_oracle.py shows on the CPU, from the
oracle alone, that every case meets the conditioning rules under which two float32 implementations stay inside them; no row or element
is left out of any comparison."""
import os

import numpy as np
import pytest

from tests import gail_ppo_oracle as go
from tests.golden import synth
from tests.hip_helpers import flat_params, unflat_params

pytestmark = pytest.mark.gpu

ACTOR_TOL = dict(rtol=2e-4, atol=5e-6)
CRITIC_TOL = dict(rtol=2e-4)
PARAM_TOL = dict(rtol=2e-3, atol=2e-5)
ADV_TOL = dict(rtol=1e-4, atol=1e-5)
NAMES = go.NAMES
H = go.HYPER
WANT = ("adv", "returns", "logp_old", "trace")


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gail_ppo.npz"))


def _engine(N, c, P=1, algo=None, hidden_act=None, **kw):
    from freerl_amd.engine import Engine
    act = {"LeakyReLU": N.ACT_LEAKY_RELU, "ReLU": N.ACT_RELU}[c["act"]] if hidden_act is None else hidden_act
    e = Engine(N.ALGO_GAIL_PPO if algo is None else algo, c["s"], c["a"], c["T"], n_learners=P, discrete=c["discrete"], hidden=c["H"], hidden_act=act,
               batch_max=c["mb"], **kw)
    if algo is None and tuple(c["rng"]) != (-10.0, 2.0):
        e.set_log_std_range(*c["rng"])
    return e


def _records(e, tab, rewards=None):
    lay = e.layout
    rec = np.zeros((len(tab["rewards"]), e.width), np.float32)
    rec[:, lay.obs_off[0]:lay.obs_off[0] + tab["states"].shape[1]] = tab["states"]
    rec[:, lay.act_off[0]:lay.act_off[0] + tab["actions"].shape[1]] = tab["actions"]
    rec[:, lay.rew_off] = tab["rewards"] if rewards is None else rewards
    rec[:, lay.done_off] = tab["done"]
    return rec


def _load(e, c, inputs_per_learner, rewards=None):
    extra = None if c["discrete"] else "log_std"
    for p, inp in enumerate(inputs_per_learner):
        e.set_params(0, flat_params(inp["params"]["actor"], NAMES, extra), learner=p)
        e.set_params(1, flat_params(inp["params"]["critic"], NAMES), learner=p)
    e.add_batch(np.concatenate([_records(e, inp["table"], rewards) for inp in inputs_per_learner]),
                learners=np.repeat(np.arange(len(inputs_per_learner)), c["T"]) if len(inputs_per_learner) > 1 else None)
    e.flush()


def _learn(e, c, perms, last_value, **kw):
    return e.gail_ppo_learn(c["T"], c["mb"], c["K"], gamma=H["gamma"], lam=H["lam"], clip=H["clip"], ent_weight=H["ent_weight"],
                            value_loss_coef=H["value_loss_coef"], p_lr=H["p_lr"], v_lr=H["v_lr"], clip_norm=H["clip_norm"], perms=perms,
                            last_value=last_value, want=WANT, **kw)


def _nets(e, c, p=0, kind=0):
    inp = go.inputs(c)["params"]
    extra = None if c["discrete"] else "log_std"
    return dict(actor=unflat_params(e.get_params(0, kind, p), inp["actor"], NAMES, extra), critic=unflat_params(e.get_params(1, kind, p), inp["critic"], NAMES))


def _check_call(got, want, p, label):
    np.testing.assert_allclose(got["adv"][p], want["adv"], err_msg=label + " adv", **ADV_TOL)
    np.testing.assert_allclose(got["returns"][p], want["returns"], err_msg=label + " returns", **ADV_TOL)
    np.testing.assert_allclose(got["logp_old"][p], want["logp_old"], err_msg=label + " logp_old", **ADV_TOL)


def _check_learner(e, c, outs, p, fx, label):
    """Learner p of engine e after the case's calls (outs: what each call returned) against the case's oracle and fixture record."""
    r = go.oracle_run(c)
    n = go.n_steps(c)
    trace = np.concatenate([o["trace"][p] for o in outs])
    for call, (o, w) in enumerate(zip(outs, r["outs"])):
        _check_call(o, w, p, "%s call %d" % (label, call))
        print("%s call %d: max |adv - oracle| %.3g, |returns - oracle| %.3g" % (label, call, np.abs(o["adv"][p] - w["adv"]).max(), np.abs(o["returns"][p] - w["returns"]).max()))
    np.testing.assert_allclose(trace[:, 0], r["actor_losses"], err_msg=label + " actor loss", **ACTOR_TOL)
    np.testing.assert_allclose(trace[:, 1], r["critic_losses"], err_msg=label + " critic loss", **CRITIC_TOL)
    assert len(trace) == c["calls"] * n
    got = _nets(e, c, p)
    for net, ref in (("actor", r["orc"].actor), ("critic", r["orc"].critic)):
        for k in ref:
            np.testing.assert_allclose(got[net][k], ref[k].reshape(got[net][k].shape), err_msg="%s %s %s" % (label, net, k), **PARAM_TOL)
    assert e.opt_step(0, p) == e.opt_step(1, p) == c["calls"] * n             # one optimiser: one count
    # ... and the reference's own record
    name = c["name"]
    np.testing.assert_allclose(np.stack([o["returns"][p] for o in outs]), fx[name + "/returns"], err_msg=label + " fixture returns", **ADV_TOL)
    np.testing.assert_allclose(trace[:, 0], fx[name + "/actor_losses"], err_msg=label + " fixture actor loss", **ACTOR_TOL)
    np.testing.assert_allclose(trace[:, 1], fx[name + "/critic_losses"], err_msg=label + " fixture critic loss", **CRITIC_TOL)
    for net in ("actor", "critic"):
        synth.check_digest("%s/%s" % (name, net), got[net], fx, PARAM_TOL["rtol"], PARAM_TOL["atol"], label)
    assert int(fx[name + "/step"]) == c["calls"] * n


def _run_case(N, c, fx, **kw):
    go.assert_conditions(c)
    inp = go.inputs(c)
    e = _engine(N, c)
    _load(e, c, [inp])
    outs = [_learn(e, c, inp["perms"][call][None], c["last_value"], **kw) for call in range(c["calls"])]
    _check_learner(e, c, outs, 0, fx, c["name"])
    return e, outs


@pytest.mark.parametrize("c", [c for c in go.CASES if c["name"] not in ("clamp", "range-wide", "range-narrow")], ids=lambda c: c["name"])
def test_cases_against_oracle_and_fixture(N, c, fx):
    e, outs = _run_case(N, c, fx)
    assert e.cursor(0) == (c["T"] % e.capacity, c["T"])                       # the call leaves the ring's cursors alone
    e.close()


def test_clamp_gate_is_closed_past_the_bounds_and_open_on_them(N, fx):
    c = go.BY_NAME["clamp"]
    raw = np.array(c["log_std"], np.float32)
    # the first step alone: the on-bound columns move by Adam's first step (lr g / (|g| + 1e-8), see tests/test_gail_ppo_oracle.py)
    inp = go.inputs(c)
    e = _engine(N, c)
    _load(e, c, [inp])
    e.gail_ppo_learn(c["mb"], c["mb"], 1, gamma=H["gamma"], lam=H["lam"], clip=H["clip"], ent_weight=H["ent_weight"], value_loss_coef=H["value_loss_coef"],
                     p_lr=H["p_lr"], v_lr=H["v_lr"], perms=np.arange(c["mb"])[None, None])
    ls = _nets(e, c)["actor"]["log_std"].reshape(-1)
    np.testing.assert_allclose(np.abs(ls - raw)[[0, 2]], H["p_lr"], rtol=1e-3)
    assert (ls[[1, 3]] == raw[[1, 3]]).all()
    e.close()
    # the whole case, and after every call: the past-bound columns bit-unchanged, their Adam moments exactly 0
    e, outs = _run_case(N, c, fx)
    for kind, want in ((N.PARAM_ONLINE, raw[[1, 3]]), (N.PARAM_ADAM_M, np.zeros(2, np.float32)), (N.PARAM_ADAM_V, np.zeros(2, np.float32))):
        got = _nets(e, c, kind=kind)["actor"]["log_std"].reshape(-1)[[1, 3]]
        assert (got == want).all(), (kind, got)
    e.close()


def test_log_std_range_is_engine_state(N, fx):
    wide, narrow = go.BY_NAME["range-wide"], go.BY_NAME["range-narrow"]
    ew, ow = _run_case(N, wide, fx)
    en, on = _run_case(N, narrow, fx)
    assert ew.log_std_range() == (-10.0, 2.0) and en.log_std_range() == (-5.0, 0.5)
    assert np.abs(ow[0]["trace"][0, :, 0] - on[0]["trace"][0, :, 0]).max() > 1e-3      # the same net, another range: other losses
    # ... and the act path reads the same range: raw log_std -7 samples with std e^-7 under [-10, 2] and e^-5 under [-5, 0.5]
    probe = go.inputs(wide)["probe"]
    eps = np.random.default_rng(5).standard_normal((len(probe), 2)).astype(np.float32)
    for e, c in ((ew, wide), (en, narrow)):
        raw = _nets(e, c)["actor"]["log_std"].reshape(-1)          # (the update has moved the open columns by a few p_lr)
        std = np.exp(np.clip(raw, *c["rng"]).astype(np.float64))
        assert (std[0] < 1.1 * np.exp(-7.0)) == (c is wide) and (abs(std[0] - np.exp(-5.0)) < 1e-9) == (c is narrow)
        mean = e.act(0, N.ACT_TANHHEAD, probe, out_dim=2)[0]
        a = e.act(0, N.ACT_PPO_SAMPLE, probe, eps=eps, out_dim=2)[0]
        # a = mean + std eps in float32: the difference carries the rounding of a value of order |mean| <= 1
        np.testing.assert_allclose(a - mean, std * eps, rtol=1e-5, atol=2.5e-7)
    ew.close()
    en.close()


def test_population_of_three_against_their_oracles(N, fx):
    cs = go.POPULATION
    for c in cs:
        go.assert_conditions(c)
    c0, inps = cs[0], [go.inputs(c) for c in cs]
    e = _engine(N, c0, P=3)
    _load(e, c0, inps)
    outs = [_learn(e, c0, np.stack([inp["perms"][0] for inp in inps]), np.array([c["last_value"] for c in cs], np.float32))]
    for p, c in enumerate(cs):
        _check_learner(e, c, outs, p, fx, c["name"])
    e.close()


def test_gae_bootstraps_from_the_next_row_across_an_episode_end(N):
    c = go.BY_NAME["leaky-3-1"]
    inp = go.inputs(c)
    tab = inp["table"]
    # from the oracle, before any engine: on the done rows the two recurrences are far apart
    orc = go.Oracle(c, inp["params"])
    vs = orc.value(tab["states"])
    r64, d64 = tab["rewards"].astype(np.float64), tab["done"].astype(np.float64)
    kept = orc.gae(r64, vs, d64, c["last_value"])[0]
    other = orc.gae(r64, vs, d64, c["last_value"], bootstrap_done=True)[0]
    rows = np.nonzero(tab["done"])[0]
    assert list(rows) == [17, 39]
    margin = np.abs(kept - other)[rows] / (ADV_TOL["atol"] + ADV_TOL["rtol"] * np.abs(kept[rows]))
    assert margin.min() > 1000, margin
    e = _engine(N, c)
    _load(e, c, [inp])
    got = _learn(e, c, inp["perms"][0][None], c["last_value"])
    np.testing.assert_allclose(got["adv"][0], kept, **ADV_TOL)
    assert (np.abs(got["adv"][0] - other)[rows] > 500 * (ADV_TOL["atol"] + ADV_TOL["rtol"] * np.abs(other[rows]))).all()
    e.close()


def test_rewards_argument_overrides_the_ring_column_bit_for_bit(N):
    c = go.BY_NAME["leaky-3-1"]
    inp = go.inputs(c)
    other = np.random.default_rng(77).standard_normal(c["T"]).astype(np.float32)
    res = []
    for in_ring in (True, False):
        e = _engine(N, c)
        _load(e, c, [inp], rewards=other if in_ring else None)
        out = _learn(e, c, inp["perms"][0][None], c["last_value"], rewards=None if in_ring else other[None])
        res.append((out, e.get_params(0), e.get_params(1)))
        e.close()
    (a, a0, a1), (b, b0, b1) = res
    for k in WANT:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
    assert not np.allclose(a["adv"][0], go.oracle_run(c)["outs"][0]["adv"], **ADV_TOL)      # (and they are not the table's rewards)


def test_act_modes_on_this_engine(N, fx):
    c = go.BY_NAME["leaky-3-1"]
    inp = go.inputs(c)
    e = _engine(N, c)
    _load(e, c, [inp])
    probe = inp["probe"]
    # raw log_std -15 under [-10, 2]: FRL_ACT_PPO_SAMPLE with injected eps returns mean + e^-10 eps
    p = {k: v.copy() for k, v in inp["params"]["actor"].items()}
    p["log_std"][:] = -15.0
    e.set_params(0, flat_params(p, NAMES, "log_std"))
    eps = np.random.default_rng(3).standard_normal((len(probe), 1)).astype(np.float32)
    mean = e.act(0, N.ACT_TANHHEAD, probe, out_dim=1)[0]
    a, lp = e.act(0, N.ACT_PPO_SAMPLE, probe, eps=eps, out_dim=1, want_logp=True)
    np.testing.assert_allclose(a[0], mean + np.exp(np.float32(-10.0)) * eps, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(lp[0], -0.5 * eps.astype(np.float64) ** 2 + 10.0 - 0.5 * np.log(2 * np.pi), rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(mean, np.tanh(go.Oracle(c, inp["params"]).head(probe)[0]), rtol=1e-4, atol=1e-5)
    # without eps the launch draws its own: finite, not the mean, another draw the next time
    d1, d2 = e.act(0, N.ACT_PPO_SAMPLE, probe, out_dim=1)[0], e.act(0, N.ACT_PPO_SAMPLE, probe, out_dim=1)[0]
    assert np.isfinite(d1).all() and not np.array_equal(d1, mean) and not np.array_equal(d1, d2)
    # after the case's calls: pi(return_mean=True) and value against the fixture's probes
    e.set_params(0, flat_params(inp["params"]["actor"], NAMES, "log_std"))
    for call in range(c["calls"]):
        _learn(e, c, inp["perms"][call][None], c["last_value"])
    np.testing.assert_allclose(e.act(0, N.ACT_TANHHEAD, probe, out_dim=1)[0], fx[c["name"] + "/probe_pi"], rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(e.act(1, N.ACT_RAW, probe, out_dim=1)[0, :, 0], fx[c["name"] + "/probe_value"], rtol=1e-3, atol=1e-4)
    e.close()
    # discrete: argmax against the fixture, samples are class indices with the log-softmax as their log-prob
    c = go.BY_NAME["cat-4-5"]
    inp = go.inputs(c)
    e = _engine(N, c)
    _load(e, c, [inp])
    logits = e.act(0, N.ACT_RAW, inp["probe"], out_dim=5)[0]
    np.testing.assert_allclose(logits, go.Oracle(c, inp["params"]).head(inp["probe"])[0], rtol=1e-4, atol=1e-5)
    assert np.array_equal(e.act(0, N.ACT_ARGMAX, inp["probe"])[0, :, 0], np.argmax(logits, axis=1))
    q = np.random.default_rng(4).exponential(size=(len(inp["probe"]), 5)).astype(np.float32)
    idx, lp = e.act(0, N.ACT_CAT_SAMPLE, inp["probe"], eps=q, want_logp=True)
    want = np.argmax(np.exp(go.log_softmax(logits.astype(np.float64))) / q, axis=1)
    assert np.array_equal(idx[0, :, 0], want)
    np.testing.assert_allclose(lp[0, :, 0], go.log_softmax(logits.astype(np.float64))[np.arange(len(want)), want], rtol=1e-5, atol=1e-6)
    for call in range(c["calls"]):
        _learn(e, c, inp["perms"][call][None], c["last_value"])
    assert np.array_equal(e.act(0, N.ACT_ARGMAX, inp["probe"])[0, :, 0], fx[c["name"] + "/probe_pi"])
    e.close()


def test_refusals(N):
    from freerl_amd.engine import Engine
    c = go.BY_NAME["leaky-3-1"]
    kw = dict(gamma=0.99, lam=0.95, clip=0.2, ent_weight=0.01, value_loss_coef=1.0, p_lr=1e-3, v_lr=1e-3)
    e = _engine(N, c)
    for name, call in (("frl_learn", lambda: e.learn(4, gamma=0.99, tau=0.005)),
                       ("frl_ppo_learn", lambda: e.ppo_learn(8, 4, 1, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.0, actor_lr=1e-3, critic_lr=1e-3)),
                       ("frl_act_explore", lambda: e.act_explore(N.ACT_TANHHEAD, np.zeros((1, 1, 3), np.float32), kind=N.EXPLORE_NONE))):
        with pytest.raises(N.FrlError, match="error 4.*%s does not serve GAIL-PPO" % name):
            call()
    with pytest.raises(N.FrlError, match="error 1.*horizon 1 < 2"):
        e.gail_ppo_learn(1, 1, 1, **kw)
    with pytest.raises(N.FrlError, match="error 1.*horizon 41 > capacity"):
        e.gail_ppo_learn(41, 16, 1, **kw)
    with pytest.raises(N.FrlError, match="error 1.*minibatch 17 outside"):
        e.gail_ppo_learn(40, 17, 1, **kw)
    with pytest.raises(N.FrlError, match="error 1.*k_epochs"):
        e.gail_ppo_learn(40, 16, 0, **kw)
    bad = np.arange(40)[None, None].copy()
    bad[0, 0, 7] = 40
    with pytest.raises(N.FrlError, match="error 1.*permutation entry 40 outside"):
        e.gail_ppo_learn(40, 16, 1, perms=bad, **kw)
    with pytest.raises(N.FrlError, match="error 1.*lo < hi"):
        e.set_log_std_range(2.0, -10.0)
    e.close()
    # the wrong engine on the other side, and Tanh at create
    ppo = Engine(N.ALGO_PPO, 3, 1, 40, batch_max=16, extra_cols=2)
    with pytest.raises(N.FrlError, match="error 4.*frl_gail_ppo_learn does not serve PPO"):
        ppo.gail_ppo_learn(40, 16, 1, **kw)
    with pytest.raises(N.FrlError, match="error 4.*frl_log_std_range_set does not serve PPO"):
        ppo.set_log_std_range(-10.0, 2.0)
    ppo.close()
    with pytest.raises(N.FrlError, match="error 1.*GAIL-PPO: hidden_act FRL_ACT_TANH is refused"):
        _engine(N, c, hidden_act=N.ACT_TANH)
