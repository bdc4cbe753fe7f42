"""GPU: HAPPO (MAPPO_file/HAPPO.py) on kernels_happo.hip, against the reference's recorded outputs (tests/golden/happo.npz) and the
NumPy restatement (tests/happo_oracle.py), at the smallest shapes at which each part can go wrong: three agents of unequal dims
(5, 3), (4, 2), (5, 3), hidden 32, horizon 40 in minibatches of 16 (the last one has 8 rows), K 2; a horizon of one row chunk + 6.

Tolerances are the project's (tests/test_gpu_mappo.py), the factors take the loss tolerance, and happo_c_hot's are derived in
tests/happo_oracle.py.  The two discrete cases with real minibatches have no reference values: the reference raises there."""
import os

import numpy as np
import pytest

from tests import happo_oracle as ho
from tests import mappo_oracle as mo
from tests.test_gpu_mappo import _extra_cols, _load, _records, _same, _state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "happo.npz")
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
def runs(fx):
    """the oracle's run of a case under the recorded order, computed once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = ho.run(ho.case(name), fx[name + "/order"])
        return cache[name]
    return get


def _engine(N, c, P=1, algo=None, **kw):
    from freerl_amd.engine import Engine
    args = dict(n_learners=P, discrete=not c["cont"], hidden=c["hidden"], batch_max=c["minibatch"], extra_cols=_extra_cols(c))
    args.update(kw)
    e = Engine(N.ALGO_HAPPO if algo is None else algo, [o for o, _ in c["dims"]], [a for _, a in c["dims"]], c["horizon"], **args)
    e.net_norm_set(c["trick"]["feature_norm"], c["trick"]["LayerNorm"])
    return e


def _hyper(c):
    """what freerl_amd.HAPPO passes: two Adams per agent behind clip_grad_norm_(..., 0.5) (HAPPO.py:237-254)"""
    t = c["trick"]
    return dict(gamma=c["gamma"], lmbda=c["lmbda"], clip=c["clip"], ent_coef=c["ent_coef"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"],
                adam_eps=1e-5 if t["adam_eps"] else 1e-8, clip_norm=0.5, adv_norm=t["adv_norm"], value_clip=t["ValueClip"],
                huber_delta=c["huber_delta"] if t["huber_loss"] else None)


def _learn(e, c, order, perms):
    return e.happo_learn(c["horizon"], c["minibatch"], c["k_epochs"], agent_order=order, perms=perms, want_trace=True, want_adv=True,
                         want_factor=True, **_hyper(c))


def _prepared(N, c, inp, **kw):
    e = _engine(N, c, **kw)
    _load(e, c, inp)
    e.add_batch(_records(inp))
    return e


def _steps(c):
    return c["k_epochs"] * -(-c["horizon"] // c["minibatch"])


def _check_against(e, c, o, fx, name, out, p=0):
    n, steps = len(c["dims"]), _steps(c)
    ref = name + "/trace" in fx
    first = int(o.order[0])
    print("%s: first losses kernel %s oracle %s; last factor kernel %.4g..%.4g oracle %.4g..%.4g; worst factor |diff| %.3g" % (
        name, out["trace"][p, first, 0], o.trace[first, 0], out["factor"][p, -1].min(), out["factor"][p, -1].max(), o.factors[-1].min(),
        o.factors[-1].max(), np.abs(out["factor"][p] - o.factors).max()))
    wants = lambda key, mine: ([(fx[name + "/" + key], "reference")] if ref else []) + [(mine, "oracle")]
    for want, who in wants("adv", o.adv_raw):
        np.testing.assert_allclose(out["adv"][p], want, rtol=1e-5, atol=2e-6, err_msg="adv vs " + who)
    for want, who in wants("v_target", o.v_target):
        np.testing.assert_allclose(out["v_target"][p], want, rtol=1e-5, atol=2e-6, err_msg="v_target vs " + who)
    rt, at = ho.tol(name, "trace")
    for want, who in wants("trace", o.trace):
        np.testing.assert_allclose(out["trace"][p], want, rtol=rt, atol=at, err_msg="loss trace vs " + who)
    rt, at = ho.tol(name, "factor")
    assert np.all(out["factor"][p, 0] == 1.0)
    for want, who in wants("factor", o.factors):
        np.testing.assert_allclose(out["factor"][p], want, rtol=rt, atol=at, err_msg="factors vs " + who)
    rt, at = ho.tol(name, "param")
    for i in range(n):
        for net, tag, want, opt, lr in ((2 * i, "actor", o.actors[i], o.aopt[i], c["actor_lr"]), (2 * i + 1, "critic", o.critics[i], o.copt[i], c["critic_lr"])):
            key = "%s/%d/%s" % (name, i, tag)
            got = e.get_params(net, 0, p)
            if key + "/p" in fx:
                mo.assert_net(got, fx[key + "/p"], lr, steps, key + " vs reference", rtol=rt, atol=at)
            if ref:
                mo.assert_digest(got, fx[key + "/digest"][0], key + " vs the reference's digest", rtol=rt, atol=at)
                assert int(fx[key + "/step"]) == steps
            mo.assert_net(got, mo.flat(c, tag, want), lr, steps, key + " vs oracle", rtol=rt, atol=at)
            mo.assert_m(e.get_params(net, 2, p), mo.flat(c, tag, opt.m), key)
            assert e.opt_step(net, learner=p) == steps
            assert e.pad_max(net, 0, p) == 0.0
    assert e.cursor(p) == (0, 0)               # Buffer_for_PPO.clear


@pytest.mark.parametrize("name", list(ho.CASES))
def test_golden_and_oracle(N, fx, runs, name):
    """every case of tests/happo_oracle.py: the whole chain against the reference's run (where it runs) and the oracle's"""
    c, o = ho.case(name), runs(name)
    e = _prepared(N, c, ho.inputs(c))
    rc = e.lds_bytes()[1]
    if name in ("happo_c_chunk", "happo_c_ragged"):
        assert c["horizon"] == rc + 6 == ho.RC + 6          # the horizon pass's second chunk has 6 rows
    assert bool(fx[name + "/ref_raises"]) == c["ref_raises"] == (name + "/trace" not in fx)
    order = fx[name + "/order"]
    out = _learn(e, c, order[None], ho.perms(c, order)[None])
    _check_against(e, c, o, fx, name, out)


def test_first_visited_agent_and_every_critic_are_mappos(N, fx, runs):
    """happo_c_plain's inputs on an ALGO_MAPPO engine through frl_mappo_learn with HAPPO's lrs, eps, clip_norm and permutations: every
    critic and the actor of the first visited agent take the same steps (two kernels: the parameter rule); the later actors do not"""
    name = "happo_c_plain"
    c, o = ho.case(name), runs(name)
    inp, order = ho.inputs(c), fx[name + "/order"]
    perms = ho.perms(c, order)[None]
    e = _prepared(N, c, inp)
    out = _learn(e, c, order[None], perms)
    m = _prepared(N, c, inp, algo=N.ALGO_MAPPO)
    mout = m.mappo_learn(c["horizon"], c["minibatch"], c["k_epochs"], perms=perms, want_trace=True, want_adv=True, **_hyper(c))
    np.testing.assert_allclose(out["adv"], mout["adv"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out["v_target"], mout["v_target"], rtol=1e-5, atol=2e-6)
    first, steps = int(order[0]), _steps(c)
    np.testing.assert_allclose(out["trace"][0, first, :, 0], mout["trace"][0, first, :, 0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(out["trace"][0, :, :, 1], mout["trace"][0, :, :, 1], rtol=1e-4, atol=1e-6)
    for i in range(3):
        mo.assert_net(e.get_params(2 * i + 1), m.get_params(2 * i + 1), c["critic_lr"], steps, "critic %d vs the MAPPO engine" % i)
        mo.assert_m(e.get_params(2 * i + 1, 2), m.get_params(2 * i + 1, 2), "critic %d vs the MAPPO engine" % i)
    mo.assert_net(e.get_params(2 * first), m.get_params(2 * first), c["actor_lr"], steps, "first visited actor vs the MAPPO engine")
    mo.assert_m(e.get_params(2 * first, 2), m.get_params(2 * first, 2), "first visited actor vs the MAPPO engine")
    for i in (int(j) for j in order[1:]):
        d = np.abs(e.get_params(2 * i) - m.get_params(2 * i))
        assert (d > 5e-6 + 5e-4 * np.abs(m.get_params(2 * i))).mean() > 0.01, "actor %d: the factor left no trace" % i
        assert not np.allclose(out["trace"][0, i, :, 0], mout["trace"][0, i, :, 0], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", ["happo_c_tricks", "happo_d_plain"])
def test_population(N, fx, name):
    """two learners with different parameters, rows AND orders in one engine: each one's result is bit-identical to the same learner
    run alone, and to a second run from the same state"""
    c = ho.case(name)
    inps = [ho.inputs(c), ho.inputs(c, seed=c["seed"] + 500)]
    orders = np.stack([fx[name + "/order"], fx[name + "/order"][::-1]])
    assert not np.array_equal(orders[0], orders[1])
    perms = np.stack([ho.perms(c, orders[0]), ho.perms(c, orders[1], seed=c["seed"] + 500)])

    def pair():
        e = _engine(N, c, P=2)
        for p in range(2):
            _load(e, c, inps[p], p)
        e.add_batch(np.concatenate([_records(inps[0]), _records(inps[1])]), learners=np.repeat(np.arange(2), c["horizon"]).astype(np.int32))
        return e, _learn(e, c, orders, perms)
    e2, out2 = pair()
    e2b, out2b = pair()
    for p in range(2):
        e1 = _prepared(N, c, inps[p])
        out1 = _learn(e1, c, orders[p][None], perms[p][None])
        for k in ("adv", "v_target", "trace", "factor"):
            assert np.array_equal(out2[k][p], out1[k][0]) and np.array_equal(out2[k][p], out2b[k][p]), k
        assert np.all(out2["factor"][p, 0] == 1.0) and np.isfinite(out2["factor"][p]).all()
        for net in range(e2.n_nets):
            for kind in (0, 2, 3):
                a = e2.get_params(net, kind, p)
                assert np.array_equal(a, e1.get_params(net, kind, 0)) and np.array_equal(a, e2b.get_params(net, kind, p))
            assert e2.opt_step(net, learner=p) == e1.opt_step(net) == _steps(c)
    assert not np.array_equal(out2["factor"][0], out2["factor"][1])


KW = dict(gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3)


def test_refusals_change_nothing(N):
    """frl_mappo_learn on a HAPPO engine, frl_happo_learn on MAPPO, PPO and MADDPG engines, the other learn / explore entry points on a
    HAPPO engine, a visiting order that is no permutation, frl_mappo_learn's argument refusals: state and ring as they were"""
    from freerl_amd.engine import Engine
    c = ho.case("happo_c_plain")
    others = [(Engine(N.ALGO_PPO, 5, 3, 40, hidden=32, batch_max=16, extra_cols=4), r"PPO engines \(updates: frl_ppo_learn\)"),
              (Engine(N.ALGO_MADDPG, [5, 4], [3, 2], 64, hidden=32, batch_max=16), r"MADDPG engines \(updates: frl_learn\)"),
              (_prepared(N, c, ho.inputs(c), algo=N.ALGO_MAPPO), r"MAPPO engines \(updates: frl_mappo_learn\)")]
    for eng, match in others:
        before = _state(eng)
        with pytest.raises(N.FrlError, match="frl_happo_learn does not serve " + match):
            eng.happo_learn(40, 16, 1, **KW)
        assert _same(before, _state(eng))
    assert others[2][0].cursor(0) == (0, 40)
    e = _prepared(N, c, ho.inputs(c))
    before = _state(e)
    with pytest.raises(N.FrlError, match=r"frl_mappo_learn does not serve HAPPO engines \(updates: frl_happo_learn\)"):
        e.mappo_learn(40, 16, 1, **KW)
    with pytest.raises(N.FrlError, match=r"frl_learn does not serve HAPPO engines \(updates: frl_happo_learn\)"):
        e.learn(16, gamma=0.99, tau=0.01)
    with pytest.raises(N.FrlError, match="frl_ppo_learn does not serve HAPPO"):
        e.ppo_learn(40, 16, 1, **KW)
    with pytest.raises(N.FrlError, match="frl_act_explore does not serve HAPPO"):
        e.act_explore(N.ACT_TANHHEAD, np.zeros((1, 1, 5), F32), kind=N.EXPLORE_NONE)
    with pytest.raises(N.FrlError, match="frl_obsnorm_enable does not serve HAPPO"):
        e.obsnorm_enable(True)
    for order in ([0, 1, 1], [0, 1, 3], [-1, 0, 1]):
        with pytest.raises(N.FrlError, match="agent_order of learner 0 is not a permutation"):
            e.happo_learn(40, 16, 1, agent_order=np.array([order]), **KW)
    for bad, match in ((dict(horizon=41), "horizon"), (dict(horizon=1), "horizon"), (dict(minibatch=17), "minibatch"), (dict(minibatch=0), "minibatch"),
                       (dict(k_epochs=0), "k_epochs"), (dict(huber_delta=0.0), "huber_delta")):
        kw = dict(horizon=40, minibatch=16, k_epochs=1, huber_delta=None)
        kw.update(bad)
        with pytest.raises(N.FrlError, match=match):
            e.happo_learn(kw["horizon"], kw["minibatch"], kw["k_epochs"], huber_delta=kw["huber_delta"], **KW)
    with pytest.raises(N.FrlError, match="permutation entry"):
        e.happo_learn(40, 16, 1, perms=np.full((1, 3, 1, 40), 40, np.int64), **KW)
    assert _same(before, _state(e))
    assert e.cursor(0) == (0, 40)             # a refused call does not clear the ring either


def test_order_and_permutations_drawn_by_the_engine(N):
    """agent_order = NULL and perms = NULL: the order is drawn on the host from the engine's seed, the permutations on the device; the
    run is finite, steps every net, and slice 0 of the factors is ones"""
    c = ho.case("happo_d_tricks")
    e = _prepared(N, c, ho.inputs(c))
    out = _learn(e, c, None, None)
    assert np.isfinite(out["trace"]).all() and np.isfinite(out["factor"]).all()
    assert np.all(out["factor"][0, 0] == 1.0) and (out["factor"][0, -1] != 1.0).any()
    assert all(e.opt_step(net) == _steps(c) for net in range(e.n_nets))
    assert e.cursor(0) == (0, 0)


@pytest.mark.parametrize("name", ["happo_c_tricks", "happo_d_tricks"])
def test_act_against_the_oracles_forward(N, name):
    """frl_act serves a HAPPO engine as it serves a MAPPO engine: the normalised forward, norms on; a critic takes the concatenated row"""
    c = ho.case(name)
    inp = ho.inputs(c)
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
        cobs = rng.normal(0, 1, (rows, sum(o for o, _ in c["dims"]))).astype(F32)
        np.testing.assert_allclose(e.act(2 * i + 1, N.ACT_RAW, cobs, out_dim=1)[0], mo.value(inp["critics"][i], cobs, c["trick"]), rtol=2e-5, atol=2e-6)
