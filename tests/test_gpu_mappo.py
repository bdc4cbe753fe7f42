"""GPU: MAPPO and IPPO (MAPPO_file/MAPPO.py, IPPO.py) on kernels_mappo.hip, against the reference's recorded outputs
(tests/golden/mappo.npz) and the NumPy restatement (tests/mappo_oracle.py), at the smallest shapes at which each part can go wrong:
three agents of unequal dims (5, 3), (4, 2), (5, 3), hidden 32, horizon 40 in minibatches of 16 (the last one has 8 rows), K 2.

Tolerances are the project's: advantages and value targets rtol 1e-5 (atol 2e-6: an advantage near zero is a sum of TD errors of size
~1 and has no relative accuracy), losses rtol 1e-4 / atol 1e-6, parameters and Adam's first moment by tests/test_gpu_envelope.py's
rule (tests/mappo_oracle.py: assert_net / assert_m)."""
import os

import numpy as np
import pytest

from tests import mappo_oracle as mo
from tests.hip_helpers import records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mappo.npz")
F32 = np.float32


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def runs():
    """the oracle's run of a case, computed once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mo.run(mo.case(name))
        return cache[name]
    return get


def _extra_cols(c):
    return sum(a if c["cont"] else 1 for _, a in c["dims"]) + len(c["dims"])


def _engine(N, c, P=1, **kw):
    from freerl_amd.engine import Engine
    args = dict(n_learners=P, discrete=not c["cont"], hidden=c["hidden"], batch_max=c["minibatch"], extra_cols=_extra_cols(c))
    args.update(kw)
    e = Engine(N.ALGO_MAPPO if c["kind"] == "mappo" else N.ALGO_IPPO, [o for o, _ in c["dims"]], [a for _, a in c["dims"]], c["horizon"], **args)
    e.net_norm_set(c["trick"]["feature_norm"], c["trick"]["LayerNorm"])
    return e


def _records(inp):
    rows = inp["rows"]
    extra = np.concatenate([r["logp"] for r in rows] + [r["adv_done"] for r in rows], axis=1)      # log-prob blocks, then one adv_done column per agent
    return records(rows, extra)


def _load(e, c, inp, p=0):
    for i in range(len(c["dims"])):
        e.set_params(2 * i, mo.flat(c, "actor", inp["actors"][i]), learner=p)
        e.set_params(2 * i + 1, mo.flat(c, "critic", inp["critics"][i]), learner=p)


def _hyper(c):
    """what the Python classes pass: MAPPO's one Adam is lr = actor_lr, eps 1e-5, no clip (MAPPO.py:229-230); IPPO's two are clipped at 0.5"""
    t = c["trick"]
    kw = dict(gamma=c["gamma"], lmbda=c["lmbda"], clip=c["clip"], ent_coef=c["ent_coef"], actor_lr=c["actor_lr"], adv_norm=t["adv_norm"],
              value_clip=t["ValueClip"], huber_delta=c["huber_delta"] if t["huber_loss"] else None)
    if c["kind"] == "mappo":
        kw.update(critic_lr=c["actor_lr"], adam_eps=1e-5, clip_norm=0.0)
    else:
        kw.update(critic_lr=c["critic_lr"], adam_eps=1e-5 if t["adam_eps"] else 1e-8, clip_norm=0.5)
    return kw


def _learn(e, c, perms):
    return e.mappo_learn(c["horizon"], c["minibatch"], c["k_epochs"], perms=perms, want_trace=True, want_adv=True, **_hyper(c))


def _prepared(N, c, inp):
    e = _engine(N, c)
    _load(e, c, inp)
    e.add_batch(_records(inp))
    return e


def _steps(c):
    return c["k_epochs"] * -(-c["horizon"] // c["minibatch"])


def _check_against(e, c, o, fx, name, out, p=0):
    """adv, v_target and the loss trace against the reference and the oracle; parameters against the reference where the golden holds them
    in full and against the oracle; Adam m against the oracle; the step counts"""
    n, steps = len(c["dims"]), _steps(c)
    print("%s: first losses kernel %s reference %s oracle %s" % (name, out["trace"][p, 0, 0], fx[name + "/trace"][0, 0], o.trace[0, 0]))
    for want, who in ((fx[name + "/adv"], "reference"), (o.adv_raw, "oracle")):
        np.testing.assert_allclose(out["adv"][p], want, rtol=1e-5, atol=2e-6, err_msg="adv vs " + who)
    for want, who in ((fx[name + "/v_target"], "reference"), (o.v_target, "oracle")):
        np.testing.assert_allclose(out["v_target"][p], want, rtol=1e-5, atol=2e-6, err_msg="v_target vs " + who)
    for want, who in ((fx[name + "/trace"], "reference"), (o.trace, "oracle")):
        np.testing.assert_allclose(out["trace"][p], want, rtol=1e-4, atol=1e-6, err_msg="loss trace vs " + who)
    for i in range(n):
        for net, tag, want, opt, lr in ((2 * i, "actor", o.actors[i], o.aopt[i], c["actor_lr"]), (2 * i + 1, "critic", o.critics[i], o.copt[i], o.critic_lr)):
            key = "%s/%d/%s" % (name, i, tag)
            got = e.get_params(net, 0, p)
            if key + "/p" in fx:
                mo.assert_net(got, fx[key + "/p"], lr, steps, key + " vs reference")
            mo.assert_net(got, mo.flat(c, tag, want), lr, steps, key + " vs oracle")
            mo.assert_m(e.get_params(net, 2, p), mo.flat(c, tag, opt.m), key)
            assert e.opt_step(net, learner=p) == steps == int(fx[key + "/step"])
            assert e.pad_max(net, 0, p) == 0.0


MATRIX = [k for k in mo.CASES if k.endswith(("_plain", "_tricks"))]


@pytest.mark.parametrize("name", MATRIX)
def test_golden_and_oracle(N, fx, runs, name):
    """each engine kind x {continuous, discrete} x {no tricks + MSE, all tricks + Huber 10}"""
    c = mo.case(name)
    e = _prepared(N, c, mo.inputs(c))
    out = _learn(e, c, fx[name + "/perms"][None])
    _check_against(e, c, runs(name), fx, name, out)
    assert e.cursor(0) == (0, 0)              # Buffer_for_PPO.clear


@pytest.mark.parametrize("name", ["mappo_c_chunk", "ippo_d_chunk"])
def test_minibatch_longer_than_a_row_chunk(N, fx, runs, name):
    """horizon = the engine's row chunk + 6 in ONE minibatch: the second chunk adds its gradient to the first's"""
    c = mo.case(name)
    e = _prepared(N, c, mo.inputs(c))
    assert c["horizon"] == c["minibatch"] == e.lds_bytes()[1] + 6
    _check_against(e, c, runs(name), fx, name, _learn(e, c, fx[name + "/perms"][None]))


@pytest.mark.parametrize("name", ["mappo_c_wide", "ippo_d_wide"])
def test_the_scripts_widths(N, fx, runs, name):
    """3 x (18, 5), hidden 128, tricks on; a MAPPO critic's first layer is 54 wide"""
    c = mo.case(name)
    e = _prepared(N, c, mo.inputs(c))
    assert e.num_params(1) == (54 if c["kind"] == "mappo" else 18) * 128 + 128 + 128 * 128 + 128 + 128 + 1
    _check_against(e, c, runs(name), fx, name, _learn(e, c, fx[name + "/perms"][None]))


@pytest.mark.parametrize("name", ["ippo_c_huber", "mappo_d_huber"])
def test_both_huber_branches(N, fx, runs, name):
    """huber_delta 0.5: in the reference's run 10 % .. 90 % of every agent's first critic errors lie inside delta (recorded by the maker)"""
    c = mo.case(name)
    assert ((fx[name + "/frac_small"] >= 0.1) & (fx[name + "/frac_small"] <= 0.9)).all()
    e = _prepared(N, c, mo.inputs(c))
    _check_against(e, c, runs(name), fx, name, _learn(e, c, fx[name + "/perms"][None]))


@pytest.mark.parametrize("name", ["mappo_c_vclip", "ippo_c_vclip"])
def test_value_clip_takes_the_unclipped_step(N, fx, runs, name):
    """>= 25 % of the first step's rows are clamped in the reference's run, and the step is the value_clip = 0 step of the same case, to
    the bit; against the golden as ever"""
    c = mo.case(name)
    assert (fx[name + "/frac_clamped"] >= 0.25).all()
    inp = mo.inputs(c)
    e = _prepared(N, c, inp)
    out = _learn(e, c, fx[name + "/perms"][None])
    _check_against(e, c, runs(name), fx, name, out)
    e0 = _prepared(N, c, inp)
    out0 = e0.mappo_learn(c["horizon"], c["minibatch"], c["k_epochs"], perms=fx[name + "/perms"][None], want_trace=True, **dict(_hyper(c), value_clip=False))
    assert np.array_equal(out["trace"], out0["trace"])
    for net in range(e.n_nets):
        assert np.array_equal(e.get_params(net), e0.get_params(net))


@pytest.mark.parametrize("name", ["mappo_c_dead", "ippo_d_dead"])
def test_dead_hidden_layer(N, fx, runs, name):
    """l1.bias = -10 on agent 1's actor and critic: its LayerNorm rows have zero variance; finite, and still the golden"""
    c = mo.case(name)
    e = _prepared(N, c, mo.inputs(c))
    out = _learn(e, c, fx[name + "/perms"][None])
    assert np.isfinite(out["trace"]).all()
    for net in range(e.n_nets):
        assert np.isfinite(e.get_params(net)).all() and np.isfinite(e.get_params(net, 2)).all()
    _check_against(e, c, runs(name), fx, name, out)


@pytest.mark.parametrize("name", ["mappo_c_plain", "mappo_c_tricks", "ippo_d_plain", "ippo_d_tricks"])
def test_act_against_the_oracles_forward(N, name):
    """every served mode through the normalised forward, norms off and on, both kinds; a MAPPO critic takes the concatenated row"""
    c = mo.case(name)
    inp = mo.inputs(c)
    e = _prepared(N, c, inp)
    rng = np.random.Generator(np.random.PCG64(5))
    rows = 70                                    # more than one row chunk
    for i, (O, A) in enumerate(c["dims"]):
        obs = rng.normal(0, 1, (rows, O)).astype(F32)
        head = mo.act_forward(c, inp["actors"][i], obs)
        if c["cont"]:
            np.testing.assert_allclose(e.act(2 * i, N.ACT_TANHHEAD, obs, out_dim=A)[0], head, rtol=2e-5, atol=2e-6)
            eps = rng.normal(0, 1, (rows, A)).astype(F32)
            got, logp = e.act(2 * i, N.ACT_PPO_SAMPLE, obs, eps=eps, out_dim=A, want_logp=True)
            ls = np.clip(inp["actors"][i]["log_std"], -20, 2).astype(F32)
            np.testing.assert_allclose(got[0], head + np.exp(ls) * eps, rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(logp[0], -(eps * eps) / 2 - ls - F32(mo.LOG_SQRT_2PI), rtol=2e-5, atol=2e-5)
        else:
            np.testing.assert_allclose(e.act(2 * i, N.ACT_RAW, obs, out_dim=A)[0], head, rtol=2e-5, atol=2e-6)
            p = mo.softmax(head)
            top2 = np.sort(p, axis=1)[:, -2:]
            sure = top2[:, 1] - top2[:, 0] > 1e-4              # (a tie within rounding may go either way)
            assert np.array_equal(e.act(2 * i, N.ACT_ARGMAX, obs)[0, sure, 0], np.argmax(p, axis=1)[sure])
            q = rng.exponential(1.0, (rows, A)).astype(F32)
            got, logp = e.act(2 * i, N.ACT_CAT_SAMPLE, obs, eps=q, want_logp=True)
            r2 = np.sort(p / q, axis=1)[:, -2:]
            sure = (r2[:, 1] - r2[:, 0]) > 1e-4 * r2[:, 1]
            want = np.argmax(p / q, axis=1)
            assert np.array_equal(got[0, sure, 0], want[sure])
            np.testing.assert_allclose(logp[0, sure, 0], np.log(p[np.arange(rows), want])[sure], rtol=2e-5, atol=2e-5)
        cobs = rng.normal(0, 1, (rows, mo.critic_in(c, i))).astype(F32)
        np.testing.assert_allclose(e.act(2 * i + 1, N.ACT_RAW, cobs, out_dim=1)[0], mo.value(inp["critics"][i], cobs, c["trick"]), rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("name", ["mappo_c_tricks", "ippo_d_plain"])
def test_population(N, fx, name):
    """two learners with different parameters and rows: each one's result is bit-identical to the same learner run alone, and to a
    second run from the same state"""
    c = mo.case(name)
    inps = [mo.inputs(c), mo.inputs(c, seed=c["seed"] + 500)]
    perms = np.stack([fx[name + "/perms"], mo.perms(c, seed=c["seed"] + 500)])

    def pair():
        e = _engine(N, c, P=2)
        for p in range(2):
            _load(e, c, inps[p], p)
        e.add_batch(np.concatenate([_records(inps[0]), _records(inps[1])]), learners=np.repeat(np.arange(2), c["horizon"]).astype(np.int32))
        return e, _learn(e, c, perms)
    e2, out2 = pair()
    e2b, out2b = pair()
    for p in range(2):
        e1 = _prepared(N, c, inps[p])
        out1 = _learn(e1, c, perms[p][None])
        for k in ("adv", "v_target", "trace"):
            assert np.array_equal(out2[k][p], out1[k][0]) and np.array_equal(out2[k][p], out2b[k][p]), k
        for net in range(e2.n_nets):
            for kind in (0, 2, 3):
                a = e2.get_params(net, kind, p)
                assert np.array_equal(a, e1.get_params(net, kind, 0)) and np.array_equal(a, e2b.get_params(net, kind, p))
            assert e2.opt_step(net, learner=p) == e1.opt_step(net) == _steps(c)


@pytest.mark.parametrize("name", ["ippo_c_single", "ippo_d_single"])
def test_one_agent_is_the_ppo_engines_step(N, fx, runs, name):
    """one agent, no tricks: IPPO.py:281-317 and PPO_with_tricks.py:324-351 are the same expressions, so an IPPO engine takes the step
    the existing PPO engine takes on the same rows, permutations and hyper-parameters (two kernels: the parameter rule)"""
    from freerl_amd.engine import Engine
    c = mo.case(name)
    inp = mo.inputs(c)
    e = _prepared(N, c, inp)
    out = _learn(e, c, fx[name + "/perms"][None])
    _check_against(e, c, runs(name), fx, name, out)
    (O, A), T = c["dims"][0], c["horizon"]
    ppo = Engine(N.ALGO_PPO, O, A, T, discrete=not c["cont"], hidden=c["hidden"], batch_max=c["minibatch"], extra_cols=_extra_cols(c))
    ppo.set_params(0, mo.flat(c, "actor", inp["actors"][0]))
    ppo.set_params(1, mo.flat(c, "critic", inp["critics"][0]))
    ppo.add_batch(_records(inp))
    h = _hyper(c)
    pout = ppo.ppo_learn(T, c["minibatch"], c["k_epochs"], gamma=h["gamma"], lmbda=h["lmbda"], clip=h["clip"], ent_coef=h["ent_coef"],
                         actor_lr=h["actor_lr"], critic_lr=h["critic_lr"], adam_eps=h["adam_eps"], clip_norm=h["clip_norm"],
                         perms=fx[name + "/perms"][0][None], want_trace=True, want_adv=True)
    np.testing.assert_allclose(out["adv"][0, :, 0], pout["adv"][0], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out["v_target"][0, :, 0], pout["v_target"][0], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out["trace"][0, 0], pout["trace"][0], rtol=1e-4, atol=1e-6)
    for net, lr in ((0, c["actor_lr"]), (1, c["critic_lr"])):
        mo.assert_net(e.get_params(net), ppo.get_params(net), lr, _steps(c), "net %d vs the PPO engine" % net)
        mo.assert_m(e.get_params(net, 2), ppo.get_params(net, 2), "net %d vs the PPO engine" % net)
        assert e.opt_step(net) == ppo.opt_step(net)


def _state(e):
    return [e.get_params(net, kind) for net in range(e.n_nets) for kind in (0, 2, 3)] + [e.opt_step(net) for net in range(e.n_nets)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_create_time_refusals(N):
    from freerl_amd.engine import Engine
    dims = dict(obs_dim=[5, 4], act_dim=[3, 2], capacity=40)

    def refused(match, algo=None, **kw):
        args = dict(dims, hidden=32, batch_max=16, extra_cols=7)
        args.update(kw)
        pos = [args.pop(k) for k in ("obs_dim", "act_dim", "capacity")]
        for a in ((N.ALGO_MAPPO, N.ALGO_IPPO) if algo is None else (algo,)):
            with pytest.raises(N.FrlError, match=match):
                Engine(a, *pos, **args)
    refused("multiple of 16", hidden=40)
    refused("hidden 272 > 256", hidden=272)
    refused("65 actions > 64", act_dim=[65, 2], discrete=True, extra_cols=4)
    refused("of LDS per row chunk", algo=N.ALGO_MAPPO, obs_dim=[1500, 1500], hidden=256)
    refused("of LDS per row chunk", algo=N.ALGO_IPPO, obs_dim=[2600, 4], hidden=256)
    refused("hidden_act", hidden_act=N.ACT_TANH)
    refused("must be 0", twin_critic=True)
    refused("must be 0", dueling=True)
    refused("must be 0", noisy=True)
    refused("must be 0", c51=(51, -10.0, 10.0))
    refused("must be 0", actor_dist=1)
    refused("extra_cols", extra_cols=3)


def test_wrong_engine_refusals_change_nothing(N):
    """frl_net_norm_set on a PPO engine, frl_mappo_learn on a MADDPG engine, and the other learn / explore entry points on these
    engines: refused through the one helper, parameters and step counts unchanged"""
    from freerl_amd.engine import Engine
    ppo = Engine(N.ALGO_PPO, 5, 3, 40, hidden=32, batch_max=16, extra_cols=4)
    before = _state(ppo)
    with pytest.raises(N.FrlError, match=r"frl_net_norm_set does not serve PPO engines \(updates: frl_ppo_learn\)"):
        ppo.net_norm_set(True, True)
    with pytest.raises(N.FrlError, match="frl_mappo_learn does not serve PPO engines"):
        ppo.mappo_learn(40, 16, 1, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3)
    assert _same(before, _state(ppo))
    mad = Engine(N.ALGO_MADDPG, [5, 4], [3, 2], 64, hidden=32, batch_max=16)
    before = _state(mad)
    with pytest.raises(N.FrlError, match=r"frl_mappo_learn does not serve MADDPG engines \(updates: frl_learn\)"):
        mad.mappo_learn(40, 16, 1, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3)
    assert _same(before, _state(mad))
    for name in ("ippo_c_plain", "mappo_c_plain"):
        c = mo.case(name)
        e = _prepared(N, c, mo.inputs(c))
        before = _state(e)
        with pytest.raises(N.FrlError, match="frl_learn does not serve %s engines \\(updates: frl_mappo_learn\\)" % c["kind"].upper()):
            e.learn(16, gamma=0.99, tau=0.01)
        with pytest.raises(N.FrlError, match="frl_ppo_learn does not serve"):
            e.ppo_learn(40, 16, 1, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3)
        with pytest.raises(N.FrlError, match="frl_act_explore does not serve"):
            e.act_explore(N.ACT_TANHHEAD, np.zeros((1, 1, 5), F32), kind=N.EXPLORE_NONE)
        with pytest.raises(N.FrlError, match="frl_obsnorm_enable does not serve"):
            e.obsnorm_enable(True)
        for bad, match in ((dict(horizon=41), "horizon"), (dict(minibatch=17), "minibatch"), (dict(k_epochs=0), "k_epochs"), (dict(huber_delta=0.0), "huber_delta")):
            kw = dict(horizon=40, minibatch=16, k_epochs=1, huber_delta=None)
            kw.update(bad)
            with pytest.raises(N.FrlError, match=match):
                e.mappo_learn(kw["horizon"], kw["minibatch"], kw["k_epochs"], gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3,
                              critic_lr=1e-3, huber_delta=kw["huber_delta"])
        bad_perm = np.full((1, 3, 1, 40), 40, np.int64)
        with pytest.raises(N.FrlError, match="permutation entry"):
            e.mappo_learn(40, 16, 1, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3, perms=bad_perm)
        assert _same(before, _state(e))
        assert e.cursor(0) == (0, 40)             # a refused call does not clear the ring either


def test_device_permutations(N):
    """perms = NULL: every (agent, epoch) gets a permutation of the horizon drawn on the device; the run is finite and steps every net"""
    c = mo.case("mappo_d_tricks")
    e = _prepared(N, c, mo.inputs(c))
    out = _learn(e, c, None)
    assert np.isfinite(out["trace"]).all()
    assert all(e.opt_step(net) == _steps(c) for net in range(e.n_nets))
