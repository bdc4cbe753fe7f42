"""GPU: ATT-MADDPG (MADDPG_file/MADDPG_simple_with_tricks.py with trick['ATT']) on kernels_att.hip, against the reference's outputs
(tests/golden/att_maddpg.npz) and the NumPy restatement (tests/att_oracle.py) on exactly the reference's rows.

Tolerances are tests/test_gpu_envelope_ddpg.py's, unchanged: losses rtol 1e-4 / atol 1e-6, norms rtol 1e-3, its _assert_net rule for
parameters (>= 99 % of a tensor within rtol 5e-4 / atol 5e-6, none further than 2 lr calls) and its rule for Adam's first moment.
tests/test_att_oracle.py shows on the CPU that float32 against float64 uses under 2 % of each on the golden inputs."""
import os

import numpy as np
import pytest
import torch

from tests import att_oracle as ao
from tests.hip_helpers import flat_params, records
from tests.test_gpu_envelope_ddpg import _assert_m, _assert_net

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ST_CRITIC_LOSS, ST_ACTOR_LOSS, ST_CRITIC_GNORM, ST_ACTOR_GNORM = 0, 1, 4, 5          # enum frl_stat


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "att_maddpg.npz")))


def _engine(N, c, P=1, batch_max=None, seed=0, algo=None):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_MADDPG_ATT if algo is None else algo, [o for o, _ in c["dims"]], [a for _, a in c["dims"]], c["n_table"], n_learners=P,
                  hidden=c["hidden"], batch_max=batch_max or c["batch"], seed=seed)


def _load(e, inp, p=0):
    for j in range(len(inp["actor"])):
        for kind in (0, 1):
            e.set_params(2 * j, flat_params(inp["actor"][j], ao.ACTOR_NAMES), kind, learner=p)
            e.set_params(2 * j + 1, flat_params(ao.to_engine(inp["critic"][j]), ao.ENGINE_NAMES), kind, learner=p)


def _learn(e, c, idx, **kw):
    """idx [P, n, B] -> stats [P, n, 8]"""
    return e.learn(np.asarray(idx).shape[-1], gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], idx=idx,
                   want_stats=True, **kw)


def _check_state(e, o, c, calls, label, p=0, agents=None, actor_calls=None):
    for j in (range(len(c["dims"])) if agents is None else agents):
        acalls = calls if actor_calls is None else actor_calls
        for net, online, target, opt, lr, names, n_calls in (
                (2 * j, o.actor[j], o.actor_t[j], o.aopt[j], c["actor_lr"], ao.ACTOR_NAMES, acalls),
                (2 * j + 1, ao.to_engine(o.critic[j]), ao.to_engine(o.critic_t[j]), o.copt[j], c["critic_lr"], ao.ENGINE_NAMES, calls)):
            tag = "%s agent %d %s" % (label, j, "actor" if net % 2 == 0 else "critic")
            _assert_net(e.get_params(net, 0, p), online, names, 5e-4, 5e-6, lr, max(n_calls, 1), tag)
            _assert_net(e.get_params(net, 1, p), target, names, 5e-4, 5e-6, lr, max(n_calls, 1), tag + " target")
            m = opt.m if net % 2 == 0 else ao.to_engine(opt.m)
            if n_calls:
                _assert_m(e.get_params(net, 2, p), m, names, tag)
            assert e.opt_step(net, learner=p) == n_calls == opt.t, tag


def _assert_call(st, want, label):
    np.testing.assert_allclose(st[:, ST_CRITIC_LOSS], want["critic_loss"], rtol=1e-4, atol=1e-6, err_msg="critic loss, " + label)
    np.testing.assert_allclose(st[:, ST_ACTOR_LOSS], want["actor_loss"], rtol=1e-4, atol=1e-6, err_msg="actor loss, " + label)
    np.testing.assert_allclose(st[:, ST_CRITIC_GNORM], want["critic_norm"], rtol=1e-3, err_msg="critic norm, " + label)
    np.testing.assert_allclose(st[:, ST_ACTOR_GNORM], want["actor_norm"], rtol=1e-3, err_msg="actor norm, " + label)


def _rows(c, t, rows):
    """[all obs | all actions] of ring rows `rows`"""
    return np.concatenate([x["obs"][rows] for x in t] + [x["act"][rows] for x in t], axis=1)


@pytest.mark.parametrize("name", list(ao.CASES))
def test_golden_and_oracle(N, fx, name):
    """Every case, every call, on the rows the reference drew: frl_act RAW on each critic and its target against first_q, both losses
    and both pre-clip norms per agent against the reference and the oracle, then every net, target and Adam m against the oracle."""
    c = ao.case(name)
    inp = ao.inputs(c)
    n = len(c["dims"])
    e = _engine(N, c)
    assert e.n_nets == 2 * n and e.lds_bytes()[0] <= 160 * 1024 and e.lds_bytes()[1] == 16
    _load(e, inp)
    e.add_batch(records(inp["table"]))
    for j in range(n):
        x = _rows(c, inp["table"], fx[name + "/idx"][0][j])
        np.testing.assert_allclose(e.act(2 * j + 1, N.ACT_RAW, x[None], out_dim=1)[0, :, 0], fx[name + "/first_q"][j], rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(e.act(2 * j + 1, N.ACT_RAW, x[None], out_dim=1, use_target=True)[0, :, 0], fx[name + "/first_q_target"][j],
                                   rtol=1e-4, atol=1e-6)
    o = ao.make(c, inp)
    for k in range(c["n_learn"]):
        idx = fx[name + "/idx"][k]
        st = _learn(e, c, idx[None])[0]
        want = o.learn_with(idx, c["gamma"], c["tau"])
        print("%s call %d: critic loss %s reference %s | actor loss %s reference %s | norms %s %s reference %s %s" %
              (name, k, st[:, 0], fx[name + "/critic_loss"][k], st[:, 1], fx[name + "/actor_loss"][k], st[:, 4], st[:, 5],
               fx[name + "/critic_norm"][k], fx[name + "/actor_norm"][k]))
        ref = {key: fx["%s/%s" % (name, key)][k] for key in ("critic_loss", "actor_loss", "critic_norm", "actor_norm")}
        _assert_call(st, ref, "call %d vs reference" % k)
        _assert_call(st, want, "call %d vs oracle" % k)
    _check_state(e, o, c, c["n_learn"], name)
    for net in range(2 * n):
        assert e.pad_max(net) == 0.0 and e.pad_max(net, 1) == 0.0 and e.pad_max(net, 2) == 0.0
    e.close()


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_ragged_rows(N, B):
    """batches that fill no 16-row tile, one exactly, one and a row, two and a row, on the heterogeneous agents"""
    c = ao.case("hetero")
    inp = ao.inputs(c, n_learn=2, batch=B)
    e = _engine(N, c, batch_max=64)
    _load(e, inp)
    e.add_batch(records(inp["table"]))
    o = ao.make(c, inp)
    for k in range(2):
        st = _learn(e, c, inp["idx"][k][None])[0]
        _assert_call(st, o.learn_with(inp["idx"][k], c["gamma"], c["tau"]), "B %d call %d" % (B, k))
    _check_state(e, o, c, 2, "B%d" % B)
    e.close()


@pytest.mark.parametrize("B", [33, 64])
def test_two_chunks_per_workgroup(N, B, monkeypatch):
    """FRL_CPS=2 (the create-time knob the other row-chunk tests use): a workgroup walks two chunks of 16 rows and its second chunk
    ADDS to the slab its first one stored; 33 rows leave the second workgroup one ragged chunk.  (The plan picks two chunks per
    workgroup by itself from 5 agents x 64 chunks up, e.g. the class's default batch_max of 1024.)"""
    monkeypatch.setenv("FRL_CPS", "2")
    c = ao.case("hetero")
    inp = ao.inputs(c, n_learn=2, batch=B, seed=7700)
    e = _engine(N, c, batch_max=64)
    _load(e, inp)
    e.add_batch(records(inp["table"]))
    o = ao.make(c, inp)
    for k in range(2):
        st = _learn(e, c, inp["idx"][k][None])[0]
        _assert_call(st, o.learn_with(inp["idx"][k], c["gamma"], c["tau"]), "B %d call %d" % (B, k))
    _check_state(e, o, c, 2, "two chunks, B%d" % B)
    e.close()


@pytest.mark.parametrize("i", [0, 1, 2])
def test_each_updating_agent(N, i):
    """agent i = first, middle, last held to the oracle on its own: its rows differ from the others', its x_d joins other slices"""
    c = ao.case("hetero")
    inp = ao.inputs(c, n_learn=1, seed=7600 + i)
    e = _engine(N, c)
    _load(e, inp)
    e.add_batch(records(inp["table"]))
    o = ao.make(c, inp)
    st = _learn(e, c, inp["idx"][0][None])[0]
    want = o.learn_with(inp["idx"][0], c["gamma"], c["tau"])
    for key, col in (("critic_loss", 0), ("actor_loss", 1)):
        np.testing.assert_allclose(st[i, col], want[key][i], rtol=1e-4, atol=1e-6, err_msg="%s of agent %d" % (key, i))
    np.testing.assert_allclose(st[i, ST_CRITIC_GNORM], want["critic_norm"][i], rtol=1e-3)
    np.testing.assert_allclose(st[i, ST_ACTOR_GNORM], want["actor_norm"][i], rtol=1e-3)
    _check_state(e, o, c, 1, "agent %d" % i, agents=[i])
    e.close()


POP = dict(ao.COMMON, dims=[(5, 2), (4, 1), (6, 3)], hidden=32, batch=9, n_table=40, n_learn=2)


@pytest.mark.parametrize("P", [1, 3, 9])
def test_population(N, P):
    """every learner has its own parameters and ring; learners 0 and P - 1 against oracles of their own (9 learners x 3 agents = 27 units
    cross the launch's rounding of the unit count to a multiple of 8)"""
    cs = [dict(POP, seed=8000 + 50 * p) for p in range(P)]
    inps = [ao.inputs(c) for c in cs]
    e = _engine(N, cs[0], P=P)
    for p in range(P):
        _load(e, inps[p], p)
    e.add_batch(np.concatenate([records(i["table"]) for i in inps]), learners=np.repeat(np.arange(P), POP["n_table"]))
    check = sorted({0, P - 1})
    orc = {p: ao.make(cs[p], inps[p]) for p in check}
    for k in range(2):
        st = _learn(e, cs[0], np.stack([i["idx"][k] for i in inps]))
        assert np.all(np.isfinite(st[:, :, :2]))
        for p in check:
            _assert_call(st[p], orc[p].learn_with(inps[p]["idx"][k], POP["gamma"], POP["tau"]), "learner %d call %d" % (p, k))
    for p in check:
        _check_state(e, orc[p], cs[p], 2, "P%d learner %d" % (P, p), p)
    e.close()


def test_do_actor_zero(N):
    """do_actor = 0: the critics step, the actors and ALL targets stay, as on FRL_ALGO_MADDPG engines"""
    c = ao.case("hetero")
    inp = ao.inputs(c, n_learn=1)
    e = _engine(N, c)
    _load(e, inp)
    e.add_batch(records(inp["table"]))
    o = ao.make(c, inp)
    before = [(e.get_params(net), e.get_params(net, 1)) for net in range(e.n_nets)]
    st = _learn(e, c, inp["idx"][0][None], do_actor=False)[0]
    want = o.learn_with(inp["idx"][0], c["gamma"], c["tau"], do_actor=False)
    np.testing.assert_allclose(st[:, ST_CRITIC_LOSS], want["critic_loss"], rtol=1e-4, atol=1e-6)
    for net in range(e.n_nets):
        assert np.array_equal(e.get_params(net, 1), before[net][1]), "target %d moved" % net
        assert np.array_equal(e.get_params(net), before[net][0]) == (net % 2 == 0), "net %d" % net
    _check_state(e, o, c, 1, "do_actor 0", actor_calls=0)
    e.close()


def test_device_indices(N):
    c = ao.case("hetero")
    inp = ao.inputs(c, n_learn=1)
    e = _engine(N, c, batch_max=64, seed=11)
    _load(e, inp)
    e.add_batch(records(inp["table"]))
    st = e.learn(33, gamma=c["gamma"], tau=c["tau"], actor_lr=1e-3, critic_lr=1e-3, want_stats=True)
    assert np.all(np.isfinite(st[0, :, :2]))
    rows = e.last_indices(33)[0]
    for j in range(3):
        assert len(set(rows[j].tolist())) == 33 and rows[j].min() >= 0 and rows[j].max() < c["n_table"]
    assert not np.array_equal(rows[0], rows[1])
    e.close()


def test_refusals_and_other_entry_points(N):
    from freerl_amd.engine import Engine
    for kw, msg in ((dict(obs=[4], act=[2]), "n_agents 1 < 2"), (dict(twin_critic=True), "twin_critic"), (dict(discrete=True), "discrete"),
                    (dict(hidden=40), "hidden"), (dict(hidden=256), "hidden 256"), (dict(obs=[9000, 4]), "LDS")):
        obs, act = kw.pop("obs", [4, 5]), kw.pop("act", [2, 3])
        with pytest.raises(N.FrlError, match=msg):
            Engine(N.ALGO_MADDPG_ATT, obs, act[:len(obs)], 64, batch_max=16, **kw)
    e = Engine(N.ALGO_MADDPG_ATT, [4, 5], [2, 3], 64, hidden=32, batch_max=16)
    assert e.learn_path(8) == (False, e.lds_bytes()[0], 16)
    for call in (lambda: e.ppo_learn(8, 8, 1, gamma=0.9, lmbda=0.9, clip=0.2, ent_coef=0.0, actor_lr=1e-3, critic_lr=1e-3),
                 lambda: e.reinforce_learn(gamma=0.99, lr=1e-3),
                 lambda: e.envelope_learn(8, 2, gamma=0.99, tau=0.01, lr=1e-3, beta=0.5),
                 lambda: e.envelope_ddpg_learn(8, 2, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, beta=0.5),
                 lambda: e.mappo_learn(8, 8, 1, gamma=0.9, lmbda=0.9, clip=0.2, ent_coef=0.0, actor_lr=1e-3, critic_lr=1e-3),
                 lambda: e.happo_learn(8, 8, 1, gamma=0.9, lmbda=0.9, clip=0.2, ent_coef=0.0, actor_lr=1e-3, critic_lr=1e-3),
                 lambda: e.gail_learn(np.zeros((1, 4, 6), np.float32), gp=False, lr=1e-3, beta1=0.9, beta2=0.999, n_expert=4)):
        with pytest.raises(N.FrlError, match="error 4.*ATT-MADDPG.*frl_learn"):
            call()
    with pytest.raises(N.FrlError, match="FRL_ACT_RAW"):
        e.act(1, N.ACT_TANHHEAD, np.zeros((1, 2, 14), np.float32), out_dim=1)
    with pytest.raises(N.FrlError, match="in_dim"):
        e.act(1, N.ACT_RAW, np.zeros((1, 2, 11), np.float32), out_dim=1)
    with pytest.raises(N.FrlError, match="Batch_ObsNorm"):
        e.obsnorm_enable(True)
    assert e.act(0, N.ACT_TANHHEAD, np.zeros((1, 2, 4), np.float32), out_dim=2).shape == (1, 2, 2)
    e.close()


def _dim_info(c):
    return {"agent_%d" % j: list(d) for j, d in enumerate(c["dims"])}


def test_class(N, fx, tmp_path):
    """freerl_amd.MADDPG_simple_with_tricks.MADDPG: the torch RNG order at construction (initial parameters against the reference's
    digests), select_action / add / learn against the reference's record, the state_dict keys, load(), and a SECOND instance in the
    same process (the reference's class counter raises IndexError there)."""
    from freerl_amd.MADDPG_simple_with_tricks import MADDPG
    c = ao.case("class")
    inp = ao.inputs(c)
    t = inp["table"]
    ids = list(_dim_info(c))
    for instance in range(2):
        torch.manual_seed(c["seed"])
        np.random.seed(c["seed"])
        pol = MADDPG(_dim_info(c), True, c["actor_lr"], c["critic_lr"], c["capacity"], "cpu", {"ATT": True}, rng="host", batch_max=16)
        pol.track_loss = True
        for j, a in enumerate(ids):
            for key, names in (("actor", ao.ACTOR_NAMES), ("critic", ao.CRITIC_NAMES)):
                sd = {k: v.numpy() for k, v in getattr(pol.agents[a], key).state_dict().items()}
                pre = "class/init/%d/%s" % (j, key)
                ao.check_digest(sd, names, fx[pre + "/stats"], fx[pre + "/sample"], 0, 0, pre)
        assert list(pol.agents[ids[0]].critic.state_dict()) == [n + s for n in ao.CRITIC_NAMES for s in (".weight", ".bias")]
        learn_at, k = ao.class_schedule(c), 0
        for i in range(c["n_steps"]):
            act = pol.select_action({a: t[j]["obs"][i] for j, a in enumerate(ids)})
            np.testing.assert_allclose(np.concatenate([act[a] for a in ids]), fx["class/action"][i], rtol=1e-4, atol=1e-6, err_msg="step %d" % i)
            pol.add({a: t[j]["obs"][i] for j, a in enumerate(ids)}, {a: t[j]["act"][i] for j, a in enumerate(ids)},
                    {a: float(t[j]["rew"][i]) for j, a in enumerate(ids)}, {a: t[j]["next_obs"][i] for j, a in enumerate(ids)},
                    {a: bool(t[j]["done"][i]) for j, a in enumerate(ids)})
            if i in learn_at:
                pol.learn(c["batch"], c["gamma"], c["tau"])
                np.testing.assert_array_equal(pol._e.last_indices(c["batch"])[0], fx["class/idx"][k])
                got = np.array([pol.last_losses[a] for a in ids])
                np.testing.assert_allclose(got[:, 0], fx["class/critic_loss"][k], rtol=1e-4, atol=1e-6, err_msg="critic loss, learn() %d" % k)
                np.testing.assert_allclose(got[:, 1], fx["class/actor_loss"][k], rtol=1e-4, atol=1e-6, err_msg="actor loss, learn() %d" % k)
                k += 1
        assert k == c["n_learn"]
    # critic(obs_list, act_list) as the reference's module is called
    rows = np.arange(5)
    q = pol.agents[ids[1]].critic([x["obs"][rows] for x in t], [x["act"][rows] for x in t])
    assert tuple(q.shape) == (5, 1) and torch.isfinite(q).all()
    pol.save(str(tmp_path))
    back = MADDPG.load(_dim_info(c), True, str(tmp_path))
    for a in ids:
        for k2, v in back.agents[a].actor.state_dict().items():
            assert torch.equal(v, pol.agents[a].actor.state_dict()[k2])
    with pytest.raises(TypeError):
        MADDPG(_dim_info(c), True, 1e-3, 1e-3, 8, "cpu")            # `trick` is required, as in the reference


def test_trick_false_is_the_plain_engine(N):
    """trick = {'ATT': False}: freerl_amd.MADDPG.MADDPG's results bit for bit"""
    from freerl_amd.MADDPG import MADDPG as Plain
    from freerl_amd.MADDPG_simple_with_tricks import MADDPG
    c = ao.case("class")
    t = ao.inputs(c)["table"]
    ids = list(_dim_info(c))
    sds = []
    for make in (lambda: Plain(_dim_info(c), True, 1e-3, 1e-3, 64, "cpu", rng="host", batch_max=16),
                 lambda: MADDPG(_dim_info(c), True, 1e-3, 1e-3, 64, "cpu", {"ATT": False}, rng="host", batch_max=16)):
        torch.manual_seed(3)
        np.random.seed(3)
        pol = make()
        for i in range(24):
            pol.add({a: t[j]["obs"][i] for j, a in enumerate(ids)}, {a: t[j]["act"][i] for j, a in enumerate(ids)},
                    {a: float(t[j]["rew"][i]) for j, a in enumerate(ids)}, {a: t[j]["next_obs"][i] for j, a in enumerate(ids)},
                    {a: bool(t[j]["done"][i]) for j, a in enumerate(ids)})
        for _ in range(2):
            pol.learn(8, 0.95, 0.01)
        sds.append([pol._e.get_params(net, kind) for net in range(pol._e.n_nets) for kind in (0, 1)])
    assert all(np.array_equal(x, y) for x, y in zip(*sds))
    assert list(pol.agents[ids[0]].critic.state_dict()) == ["l1.weight", "l1.bias", "l2.weight", "l2.bias", "l3.weight", "l3.bias"]
