"""GPU: CEM_GD3PG.learn (CEM_GD3PG_file/CEM_GD3PG.py) on kernels_cem_gd3pg.hip, against the reference's outputs
(tests/golden/cem_gd3pg.npz) and the NumPy restatement (tests/cem_gd3pg_oracle.py).

Every engine shape and call size used here is a row of tests/test_cem_gd3pg_plan.py's SHAPES, whose offsets the CPU probe walks.
Tolerances are tests/test_gpu_envelope_ddpg.py's, unchanged: losses rtol 1e-4 / atol 1e-6, norms rtol 1e-3, parameters 5e-4 / 5e-6 on
>= 99 % of a net's elements and none further than Adam can move it, Adam's m within 2e-3 of a tensor's largest."""
import os

import numpy as np
import pytest
import torch

from tests import cem_gd3pg_oracle as co
from tests.hip_helpers import flat_params
from tests.test_cem_gd3pg_plan import POPULATIONS, RAGGED_DIMS, RAGGED_ROWS, SPLIT_ROWS, shapes
from tests.test_gpu_envelope_ddpg import _assert_m, _assert_net

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = co.NAMES
NETS = (("actor_1", 0), ("actor_2", 1), ("critic", 2))


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "cem_gd3pg.npz")))


def _engine(N, shape, seed=0):
    from freerl_amd.engine import Engine
    O, A, H, P, cap, bm = shape[:6]
    return Engine(N.ALGO_CEM_GD3PG, O, A, cap, n_learners=P, hidden=H, hidden_act=N.ACT_TANH, batch_max=bm, seed=seed)


def _case_engine(N, c, P=1, cap=None, batch_max=None, seed=0):
    return _engine(N, (c["obs_dim"], c["act_dim"], c["hidden"], P, cap or c["cap"], batch_max or max(c["batch"], 2)), seed)


def _records(e, t):
    lay, n = e.layout, len(t["done"])
    rec = np.zeros((n, e.width), np.float32)
    O, A = t["obs"].shape[1], t["act"].shape[1]
    rec[:, lay.obs_off[0]:lay.obs_off[0] + O] = t["obs"]
    rec[:, lay.act_off[0]:lay.act_off[0] + A] = t["act"]
    rec[:, lay.rew_off] = t["rew"]
    rec[:, lay.done_off] = t["done"]
    rec[:, lay.next_obs_off[0]:lay.next_obs_off[0] + O] = t["next_obs"]
    return rec


def _load(e, inp, p=0):
    for key, net in NETS:
        e.set_params(net, flat_params(inp[key], NAMES), 0, learner=p)
        e.set_params(net, flat_params(inp.get(key + "_target", inp[key]), NAMES), 1, learner=p)
    e.set_params(3, flat_params(inp["actor_domain"], NAMES), 0, learner=p)
    for r, key in ((0, "table0"), (1, "table1")):
        if len(inp[key]["done"]):
            e.ring_add_batch(r, _records(e, inp[key]), learners=np.full(len(inp[key]["done"]), p, np.int32))


def _learn(e, c, idx, f1=None, delta=None, batch=None):
    return e.cem_gd3pg_learn(batch or c["batch"], gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"],
                             f1_more=c["f1_more"] if f1 is None else f1, delta=c["delta"] if delta is None else delta, lam=co.LAMBDA, idx=idx)


def _assert_out(got, want, msg):
    """[8] in the oracle's OUT order: losses and KL at the loss tolerance, norms at rtol 1e-3, the row count exactly"""
    for col, key in enumerate(co.OUT):
        if key == "rows":
            assert got[col] == want[col], "%s: rows %r != %r" % (msg, got[col], want[col])
        elif key.endswith("norm"):
            np.testing.assert_allclose(got[col], want[col], rtol=1e-3, err_msg="%s, %s" % (key, msg))
        else:
            np.testing.assert_allclose(got[col], want[col], rtol=1e-4, atol=1e-6, err_msg="%s, %s" % (key, msg))


def _check_state(e, o, c, calls, label, p=0):
    for key, net in NETS:
        online, target, opt = ((o.actor[net], o.actor_t[net], o.aopt[net]) if net < 2 else (o.critic, o.critic_t, o.copt))
        lr = c["actor_lr"] if net < 2 else c["critic_lr"]
        tag = "%s %s" % (label, key)
        _assert_net(e.get_params(net, 0, p), online, NAMES, 5e-4, 5e-6, lr, calls, tag)
        _assert_net(e.get_params(net, 1, p), target, NAMES, 5e-4, 5e-6, lr, calls, tag + " target")
        _assert_m(e.get_params(net, 2, p), opt.m, NAMES, tag)
        assert e.opt_step(net, learner=p) == calls == opt.t
    assert e.opt_step(3, learner=p) == 0


@pytest.mark.parametrize("name", list(co.CASES))
def test_golden_and_oracle(N, fx, name):
    """Every case, every call, on the rows the reference drew: the three losses, the three pre-clip norms and KL against the reference
    and the oracle; the six nets and Adam's m element-wise against the oracle."""
    c = co.case(name)
    inp = co.inputs(c, seed=int(fx[name + "/seed"]))
    e = _case_engine(N, c)
    _load(e, inp)
    o = co.CemGd3pg(inp, c)
    for k in range(c["n_learn"]):
        idx = fx[name + "/idx"][k]
        got = _learn(e, c, idx[None])[0]
        w = o.learn_with(idx, c["gamma"], c["tau"], c["f1_more"], c["delta"])
        want = [w[key] for key in co.OUT]
        print("%s call %d\n  engine    %s\n  reference %s\n  oracle    %s" % (name, k, got, fx[name + "/out"][k], np.array(want)))
        _assert_out(got, fx[name + "/out"][k], "%s call %d vs reference" % (name, k))
        _assert_out(got, want, "%s call %d vs oracle" % (name, k))
        st = e.stats()[0, 0]
        assert (st[0], st[4], st[1], st[5]) == (got[0], got[1], got[2], got[3])          # FRL_STAT_* carry the same values
    _check_state(e, o, c, c["n_learn"], name)
    e.close()


def _ragged_case(O, A, rows, seed, hidden=32):
    """a case whose ring 1 holds exactly `rows` rows, so that batch = rows uses all of them twice over"""
    return dict(co.COMMON, obs_dim=O, act_dim=A, hidden=hidden, batch=rows, cap=80, n0=80, n1=max(rows, 2), f1_more=bool(rows % 4), delta=0.4,
                reward_scale=1.0, seed=seed)


@pytest.mark.parametrize("O,A", RAGGED_DIMS)
def test_ragged_rows(N, O, A, monkeypatch):
    """2 half of 2, 10, 30, 32, 34 and 70 at 16-row chunks: the seam between ring 0's and ring 1's halves inside a chunk and on a chunk
    boundary, a last chunk of 2 rows; A of 1, 4 and 16 (a head of more than 4 columns leaves the fused narrow-head path); obs of 3, 33."""
    monkeypatch.setenv("FRL_RC", "16")
    shape = shapes()["ragged_o%d_a%d" % (O, A)]
    for rows in RAGGED_ROWS:
        c = _ragged_case(O, A, rows, 9000 + 100 * O + 10 * A + rows)
        inp = co.inputs(c, n_learn=2)
        e = _engine(N, shape)
        assert e.lds_bytes()[1] == 16
        _load(e, inp)
        o = co.CemGd3pg(inp, c)
        for k in range(2):
            got = _learn(e, c, inp["idx"][k][None])[0]
            w = o.learn_with(inp["idx"][k], c["gamma"], c["tau"], c["f1_more"], c["delta"])
            _assert_out(got, [w[key] for key in co.OUT], "O %d A %d rows %d call %d" % (O, A, rows, k))
        _check_state(e, o, c, 2, "O%d A%d rows%d" % (O, A, rows))
        e.close()


@pytest.mark.parametrize("rows", SPLIT_ROWS)
def test_chunk_splits(N, rows, monkeypatch):
    """FRL_RC=16 with FRL_CPS 2 and 3: a workgroup's later chunks ADD to the slab its first one stored, in the critic and in the actor
    launch (whose spill block and parked domain rows follow the chunk) — against the oracle, and against the FRL_CPS=1 engine."""
    monkeypatch.setenv("FRL_RC", "16")
    c = dict(_ragged_case(5, 2, rows, 9700 + rows), cap=80)
    inp = co.inputs(c, n_learn=2)
    res = {}
    for cps in (1, 2, 3):
        monkeypatch.setenv("FRL_CPS", str(cps))
        e = _engine(N, shapes()["split_cps%d" % cps])
        assert e.lds_bytes()[1] == 16
        _load(e, inp)
        o = co.CemGd3pg(inp, c)
        outs = []
        for k in range(2):
            outs.append(_learn(e, c, inp["idx"][k][None])[0])
            w = o.learn_with(inp["idx"][k], c["gamma"], c["tau"], c["f1_more"], c["delta"])
            _assert_out(outs[-1], [w[key] for key in co.OUT], "cps %d rows %d call %d" % (cps, rows, k))
        _check_state(e, o, c, 2, "cps%d rows%d" % (cps, rows))
        res[cps] = (np.array(outs), [e.get_params(net) for net in (0, 1, 2)])
        e.close()
    for cps in (2, 3):          # the same sums in another order: rounding apart
        np.testing.assert_allclose(res[cps][0], res[1][0], rtol=1e-4, atol=1e-6)
        for a, b in zip(res[cps][1], res[1][1]):
            np.testing.assert_allclose(a, b, rtol=5e-4, atol=5e-6)


POP = dict(obs_dim=4, act_dim=3, hidden=32, batch=16, cap=40, n0=40, n1=40, reward_scale=1.0)


def pop_inputs(p):
    # every learner its own nets, rings, flag and weight; learner 1: delta = 0; learner 2: the domain actor IS its guided actor (sum c^2 = 0)
    c = dict(co.COMMON, **POP, seed=9500 + 10 * p, f1_more=bool(p % 2), delta=0.0 if p == 1 else 0.1 + 0.05 * (p % 7))
    inp = co.inputs(c, n_learn=2)
    if p == 2:
        inp["actor_domain"] = {k: v.copy() for k, v in inp["actor_1"].items()}       # f1_more false: actor_1 is the guided one
    return c, inp


@pytest.mark.parametrize("P", POPULATIONS)
def test_population(N, P):
    e = _engine(N, shapes()["population_%d" % P])
    cs, inps = zip(*[pop_inputs(p) for p in range(P)])
    for p in range(P):
        _load(e, inps[p], p)
    check = sorted({0, 1, 2, P // 2, P - 1})
    orc = {p: co.CemGd3pg(inps[p], cs[p]) for p in check}
    c0 = cs[0]
    for k in range(2):
        got = e.cem_gd3pg_learn(16, gamma=c0["gamma"], tau=c0["tau"], actor_lr=c0["actor_lr"], critic_lr=c0["critic_lr"],
                                f1_more=[c["f1_more"] for c in cs], delta=[c["delta"] for c in cs], idx=np.stack([i["idx"][k] for i in inps]))
        assert np.all(np.isfinite(got))
        for p in check:
            w = orc[p].learn_with(inps[p]["idx"][k], c0["gamma"], c0["tau"], cs[p]["f1_more"], cs[p]["delta"])
            _assert_out(got[p], [w[key] for key in co.OUT], "learner %d call %d" % (p, k))
        if k == 0:
            assert got[2][6] == 0.0          # sum c^2 == 0: KL reported as 0
    for p in check:
        _check_state(e, orc[p], cs[p], 2, "P%d learner %d" % (P, p), p)
    # sum c^2 == 0 gives finite parameters, equal to the same step without the penalty
    e2 = _engine(N, shapes()["population_%d" % P])
    for p in range(P):
        _load(e2, inps[p], p)
    delta0 = [0.0 if p == 2 else cs[p]["delta"] for p in range(P)]
    e2.cem_gd3pg_learn(16, gamma=c0["gamma"], tau=c0["tau"], actor_lr=c0["actor_lr"], critic_lr=c0["critic_lr"], f1_more=[c["f1_more"] for c in cs],
                       delta=delta0, idx=np.stack([i["idx"][0] for i in inps]))
    e3 = _engine(N, shapes()["population_%d" % P])
    for p in range(P):
        _load(e3, inps[p], p)
    e3.cem_gd3pg_learn(16, gamma=c0["gamma"], tau=c0["tau"], actor_lr=c0["actor_lr"], critic_lr=c0["critic_lr"], f1_more=[c["f1_more"] for c in cs],
                       delta=[c["delta"] for c in cs], idx=np.stack([i["idx"][0] for i in inps]))
    for net in (0, 1, 2):
        a, b = e3.get_params(net, 0, 2), e2.get_params(net, 0, 2)
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), net
    e.close(); e2.close(); e3.close()


def test_device_draw(N):
    """idx = NULL: no repeats within a half, both halves below ring 1's size, the second half offset into ring 1."""
    c = dict(co.COMMON, **dict(POP, cap=64, n0=64, n1=40, batch=64), seed=9800, f1_more=True, delta=0.3)
    inp = co.inputs(c, n_learn=1)
    e = _engine(N, (4, 3, 32, 2, 64, 64), seed=11)
    for p in range(2):
        _load(e, inp, p)
    before = [e.get_params(net) for net in (0, 1, 2)]
    seen = []
    for k in range(3):
        out = _learn(e, c, None)
        assert np.all(np.isfinite(out)) and np.all(out[:, 7] == 40)          # half = min(40, 64) // 2 = 20
        rows = e.last_indices(40)[:, 0]
        for p in range(2):
            h0, h1 = rows[p, :20], rows[p, 20:]
            assert len(set(h0.tolist())) == 20 and len(set(h1.tolist())) == 20
            assert h0.min() >= 0 and h0.max() < 40 and h1.min() >= 64 and h1.max() < 64 + 40
        assert not np.array_equal(rows[0], rows[1])
        seen.append(rows.copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    for net in (0, 1, 2):
        after = e.get_params(net)
        assert np.all(np.isfinite(after)) and not np.array_equal(before[net], after) and e.opt_step(net) == 3
    e.close()


def test_frozen_state(N):
    """actor_domain's parameters and every padded slot bit-unchanged after 3 calls; net 3's target, Adam state and step never touched."""
    c = co.case("odd")
    inp = co.inputs(c)
    e = _case_engine(N, c)
    _load(e, inp)
    dom = e.get_params(3, 0).copy()
    marks = {kind: np.full(e.num_params(3), 0.25 * (kind + 1), np.float32) for kind in (1, 2, 3)}
    for kind, v in marks.items():
        e.set_params(3, v, kind)
    for k in range(3):
        _learn(e, c, inp["idx"][k][None])
    assert np.array_equal(e.get_params(3, 0), dom) and e.opt_step(3) == 0
    for kind, v in marks.items():
        assert np.array_equal(e.get_params(3, kind), v), kind
    for net in range(4):
        for kind in (0, 1, 2, 3):
            assert e.pad_max(net, kind) == 0.0, (net, kind)
    e.close()


def test_class(N, tmp_path):
    """freerl_amd.CEM_GD3PG.CEM_GD3PG: select_action, the get_params / set_params round trip, rings that wrap, a host-drawn learn() against
    the oracle on the same NumPy stream, save / load."""
    from freerl_amd.CEM_GD3PG import CEM_GD3PG
    c = dict(co.COMMON, obs_dim=5, act_dim=2, hidden=32, batch=16, cap=24, n0=24, n1=24, f1_more=False, delta=0.2, reward_scale=1.0, seed=9900)
    inp = co.inputs(c, n_learn=1)
    torch.manual_seed(3)
    pol = CEM_GD3PG([5, 2], True, c["actor_lr"], c["critic_lr"], 24, "cpu", hidden=32, batch_max=16, rng="host")
    ag = pol.agent
    # the constructor's nets: actor_domain starts as a copy of actor_2, the targets as copies of their nets
    assert np.array_equal(ag.actor_domain.get_params(), ag.actor_2.get_params()) and not np.array_equal(ag.actor_1.get_params(), ag.actor_2.get_params())
    assert np.array_equal(ag.actor_1_target.get_params(), ag.actor_1.get_params())
    assert list(ag.actor_1.state_dict()) == ["l1.weight", "l1.bias", "l2.weight", "l2.bias", "l3.weight", "l3.bias"]
    assert {k: tuple(v.shape) for k, v in ag.critic.state_dict().items()}["l1.weight"] == (32, 7)
    for key, net in (("actor_1", ag.actor_1), ("actor_2", ag.actor_2), ("critic", ag.critic), ("actor_domain", ag.actor_domain),
                     ("actor_1_target", ag.actor_1_target), ("actor_2_target", ag.actor_2_target), ("critic_target", ag.critic_target)):
        net.load_state_dict({k: torch.as_tensor(v) for k, v in inp[key].items()})
    flat = ag.actor_1.get_params()
    assert flat.dtype == np.float32 and flat.size == ag.actor_1.get_size() == 5 * 32 + 32 + 32 * 32 + 32 + 32 * 2 + 2
    np.testing.assert_array_equal(flat, flat_params(inp["actor_1"], NAMES))          # torch's parameters() order
    ag.actor_domain.set_params(flat.astype(np.float64) * 0.5)
    np.testing.assert_array_equal(ag.actor_domain.get_params(), (flat.astype(np.float64) * 0.5).astype(np.float32))
    ag.actor_domain.set_params(flat_params(inp["actor_domain"], NAMES))
    o = co.CemGd3pg(dict(inp, table0=None, table1=None), c)
    # rings that wrap: 30 rows into ring 0 of 24, 27 into ring 1
    t0, t1 = co.table(1, 30, c), co.table(2, 27, c)
    for r, (buf, t) in enumerate(((pol.buffer, t0), (pol.buffer_domain, t1))):
        for i in range(len(t["done"])):
            pol.add(buf, t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]))
            o.add(r, t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]))
    assert len(pol.buffer) == len(pol.buffer_domain) == 24 and pol.buffer._index == 6 and pol.buffer_domain._index == 3
    np.testing.assert_array_equal(pol.buffer_domain.obs, o.ring[1]["obs"])
    np.testing.assert_array_equal(pol.buffer.rewards, o.ring[0]["rew"])
    act = pol.select_action(t0["obs"][0], ag.actor_1)
    np.testing.assert_allclose(act, o.pi(o.actor[0], t0["obs"][:1])[0][0], rtol=1e-4, atol=1e-6)
    np.testing.assert_array_equal(pol.evaluate_action(t0["obs"][0], ag.actor_1), act)
    np.random.seed(77)
    obs, a, r, nobs, d = pol.sample(16)
    assert obs.shape == (16, 5) and a.shape == (16, 2) and r.shape == (16, 1) and d.shape == (16, 1)
    np.random.seed(77)
    i0, i1 = o.draw(16)
    np.testing.assert_array_equal(obs.numpy(), np.concatenate([o.ring[0]["obs"][i0], o.ring[1]["obs"][i1]]))
    np.random.seed(78)
    pol.learn(16, c["gamma"], c["tau"], False, 0.2, ag.actor_domain)
    np.random.seed(78)
    idx = o.draw(16)
    np.testing.assert_array_equal(np.stack(pol.last_indices), np.stack(idx))
    after = np.random.rand()
    w = o.learn_with(idx, c["gamma"], c["tau"], False, 0.2)
    _assert_out(pol.last_out, [w[key] for key in co.OUT], "learn()")
    np.random.seed(78)
    o.draw(16)
    assert after == np.random.rand()          # two choice() calls per learn, nothing else
    with pytest.raises(ValueError):
        pol.learn(16, c["gamma"], c["tau"], False, 0.2, ag.actor_1)
    pol.save(str(tmp_path), ag.actor_domain)
    back = CEM_GD3PG.load([5, 2], str(tmp_path), hidden=32)
    np.testing.assert_array_equal(back.agent.actor_domain.get_params(), ag.actor_domain.get_params())
    with pytest.raises(ValueError):
        CEM_GD3PG([5, 2], False, 1e-3, 1e-3, 24, "cpu")


def test_rejections(N):
    import ctypes as C
    from freerl_amd.engine import Engine
    kw = dict(hidden=32, batch_max=16)
    with pytest.raises(N.FrlError, match="hidden_act"):
        Engine(N.ALGO_CEM_GD3PG, 4, 3, 40, **kw)                                        # FRL_ACT_RELU
    with pytest.raises(N.FrlError, match="discrete"):
        Engine(N.ALGO_CEM_GD3PG, 4, 3, 40, hidden_act=N.ACT_TANH, discrete=True, **kw)
    with pytest.raises(N.FrlError, match="twin_critic"):
        Engine(N.ALGO_CEM_GD3PG, 4, 3, 40, hidden_act=N.ACT_TANH, twin_critic=True, **kw)
    with pytest.raises(N.FrlError, match="n_agents"):
        Engine(N.ALGO_CEM_GD3PG, [4, 4], [3, 3], 40, hidden_act=N.ACT_TANH, **kw)
    c = dict(co.COMMON, **POP, seed=9950, f1_more=True, delta=0.3)
    inp = co.inputs(c, n_learn=1)
    e = _engine(N, (4, 3, 32, 1, 40, 16))
    assert e.n_nets == 4
    ok = dict(gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, f1_more=True, delta=0.3)
    with pytest.raises(N.FrlError, match="error 4.*ring 1"):                            # nothing in buffer_domain yet
        e.cem_gd3pg_learn(16, **ok)
    _load(e, dict(inp, table1=dict((k, v[:9]) for k, v in inp["table1"].items())))      # 9 rows in ring 1: half = 4
    before = [e.get_params(net) for net in (0, 1, 2)]
    idx = inp["idx"][0][:, :4] % 9
    for batch, kw2, ix, msg in ((1, {}, None, "batch"), (16, dict(gamma=float("nan")), idx, "NaN"), (16, dict(tau=float("nan")), idx, "NaN"),
                                (16, dict(actor_lr=float("nan")), idx, "NaN"), (16, dict(critic_lr=float("nan")), idx, "NaN"),
                                (16, dict(lam=float("nan")), idx, "NaN"), (16, dict(delta=float("nan")), idx, "NaN"),
                                (16, {}, np.array([[0, 1, 2, 40], [0, 1, 2, 3]]), "ring 0"), (16, {}, np.array([[0, 1, 2, 39], [0, 1, 2, 9]]), "ring 1"),
                                (16, {}, np.array([[0, 1, 2, -1], [0, 1, 2, 3]]), "ring 0")):
        with pytest.raises(N.FrlError, match="error 1.*" + msg):
            e.cem_gd3pg_learn(batch, **dict(ok, **kw2), idx=None if ix is None else ix[None])
    with pytest.raises(N.FrlError, match="ring 2"):
        e.ring_add(2, np.zeros(e.width, np.float32))
    e2 = _engine(N, (4, 3, 32, 1, 40, 4))
    _load(e2, inp)
    with pytest.raises(N.FrlError, match="error 1.*batch_max"):
        e2.cem_gd3pg_learn(16, **ok)
    e2.close()
    for call in (lambda: e.learn(8, gamma=0.99, tau=0.01, critic_lr=1e-3), lambda: e.learn_path(8), lambda: e.learn_work(8),
                 lambda: e.envelope_ddpg_learn(8, 1, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, beta=0.5),
                 lambda: e.reinforce_learn(gamma=0.99, lr=1e-3), lambda: e.ppo_learn(8, 8, 1, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.0, actor_lr=1e-3, critic_lr=1e-3),
                 lambda: e.act_explore(N.ACT_TANHHEAD, np.zeros((1, 1, 4), np.float32), kind=N.EXPLORE_GAUSS)):
        with pytest.raises(N.FrlError, match="error 4.*frl_cem_gd3pg_learn"):           # FRL_ERR_STATE, naming the entry point to use
            call()
    ra, st = N.RolloutArgs(), N.RolloutStats()
    assert e._L.frl_rollout(e._h, None, C.byref(ra), C.byref(st)) == 4 and b"frl_cem_gd3pg_learn" in e._L.frl_last_error()
    with pytest.raises(N.FrlError, match="FRL_ACT"):
        e.act(2, N.ACT_TANHHEAD, np.zeros((1, 1, 7), np.float32), out_dim=1)
    for net in (0, 1, 2):
        assert np.array_equal(before[net], e.get_params(net)) and e.opt_step(net) == 0  # nothing was launched
    # frl_act: the target critic's Q on [obs | act], the domain actor and an actor's target on obs
    o = co.CemGd3pg(inp, c)
    x = np.concatenate([inp["table0"]["obs"][:5], inp["table0"]["act"][:5]], 1)
    np.testing.assert_allclose(e.act(2, N.ACT_RAW, x[None], out_dim=1, use_target=True)[0], o.q(o.critic_t, x[:, :4], x[:, 4:])[0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(e.act(3, N.ACT_TANHHEAD, x[None, :, :4], out_dim=3)[0], o.pi(o.domain, x[:, :4])[0], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(e.act(1, N.ACT_TANHHEAD, x[None, :, :4], out_dim=3, use_target=True)[0], o.pi(o.actor_t[1], x[:, :4])[0], rtol=1e-4, atol=1e-6)
    out = e.cem_gd3pg_learn(16, **ok, idx=idx[None])
    assert np.all(np.isfinite(out)) and out[0, 7] == 8                                  # ... and the engine still works
    e.close()
    d = Engine(N.ALGO_DDPG, 4, 3, 40, batch_max=32)
    with pytest.raises(N.FrlError, match="error 4.*frl_learn"):
        d.cem_gd3pg_learn(16, **ok)
    with pytest.raises(N.FrlError, match="ring 1"):
        d.ring_add(1, np.zeros(d.width, np.float32))
    d.close()
