"""GPU: envelope multi-objective DDPG (ENVELOPE_MORL_file/ENVELOPE_DDPG.py) on kernels_envelope_ddpg.hip, against the reference's
outputs (tests/golden/envelope_ddpg.npz) and the NumPy restatement (tests/envelope_ddpg_oracle.py).

The algorithm has no argmax, so there is no margin condition: every row of every call is compared.  Tolerances are
tests/test_gpu_envelope.py's, unchanged; tests/test_envelope_ddpg_oracle.py shows on the CPU that float32 against float64 needs
none of the 1 % allowance on the golden inputs."""
import os

import numpy as np
import pytest
import torch

from tests import envelope_ddpg_oracle as eo
from tests.hip_helpers import flat_params, unflat_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = eo.NAMES
ST_CRITIC_GNORM, ST_ACTOR_GNORM = 4, 5          # enum frl_stat


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "envelope_ddpg.npz")))


def _engine(N, c, P=1, cap=None, batch_max=None, seed=0):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_ENVELOPE_DDPG, c["obs_dim"], c["act_dim"], cap or c["n_table"], n_learners=P, hidden=c["hidden"],
                  batch_max=batch_max or c["batch"] * c["weight_num"], reward_dim=c["rdim"], seed=seed)


def _records(e, t):
    lay, n = e.layout, len(t["done"])
    rec = np.zeros((n, e.width), np.float32)
    O, A, R = t["obs"].shape[1], t["act"].shape[1], t["rew"].shape[1]
    assert lay.done_off - lay.rew_off == R == e.reward_dim and lay.act_dim[0] == A
    rec[:, lay.obs_off[0]:lay.obs_off[0] + O] = t["obs"]
    rec[:, lay.act_off[0]:lay.act_off[0] + A] = t["act"]
    rec[:, lay.rew_off:lay.rew_off + R] = t["rew"]
    rec[:, lay.done_off] = t["done"]
    rec[:, lay.next_obs_off[0]:lay.next_obs_off[0] + O] = t["next_obs"]
    return rec


def _load(e, inp, p=0):
    for net, key in ((0, "actor"), (1, "critic")):
        for kind in (0, 1):
            e.set_params(net, flat_params(inp[key], NAMES), kind, learner=p)


def _learn(e, c, idx, w, beta=None, **kw):
    """-> (critic loss [P], actor loss [P])"""
    out = e.envelope_ddpg_learn(np.asarray(idx).shape[-1], np.asarray(w).shape[-2], gamma=c["gamma"], tau=c["tau"],
                                actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], beta=c["beta"] if beta is None else beta, idx=idx,
                                weights=w, want_loss=True, **kw)
    return out["critic_loss"], out["actor_loss"]


# Parameter tolerances: tests/test_gpu_envelope.py's rules, unchanged (two fp32 implementations of one update differ by rounding in
# every gradient element, and a ReLU unit within rounding of zero may be open in one and shut in the other): >= 99 % of a net's
# elements within (rtol, atol), none further than Adam can move an element in `calls` steps; the first moment within 2e-3 of its
# largest on >= 99 % of a matrix, within 5e-2 everywhere (2e-2 for bias vectors).
def _assert_net(got_flat, want, names, rtol, atol, lr, calls, label):
    got = unflat_params(got_flat, want, names)
    for k in want:
        d = np.abs(got[k] - want[k])
        bad = d > atol + rtol * np.abs(want[k])
        assert bad.mean() <= 0.01, "%s/%s: %d of %d elements outside (max |diff| %.3g)" % (label, k, bad.sum(), bad.size, d.max())
        assert d.max() <= 2 * lr * calls, "%s/%s: max |diff| %.3g" % (label, k, d.max())


def _assert_m(got_flat, want, names, label):
    got = unflat_params(got_flat, want, names)
    for k in want:
        scale = float(np.abs(want[k]).max())
        d = np.abs(got[k] - want[k]).reshape(-1)
        if d.size < 2048:
            assert d.max() <= 2e-2 * scale, "adam m %s/%s: %.3g of max |m| %.3g" % (label, k, d.max(), scale)
            continue
        assert np.quantile(d, 0.99) <= 2e-3 * scale, "adam m %s/%s: 99th percentile" % (label, k)
        assert d.max() <= 5e-2 * scale, "adam m %s/%s: max %.3g of %.3g" % (label, k, d.max(), scale)


def _check_state(e, o, c, calls, label, p=0):
    for net, online, target, opt, lr in ((0, o.actor, o.actor_t, o.aopt, c["actor_lr"]), (1, o.critic, o.critic_t, o.copt, c["critic_lr"])):
        tag = "%s %s" % (label, "actor" if net == 0 else "critic")
        _assert_net(e.get_params(net, 0, p), online, NAMES, 5e-4, 5e-6, lr, calls, tag)
        _assert_net(e.get_params(net, 1, p), target, NAMES, 5e-4, 5e-6, lr, calls, tag + " target")
        _assert_m(e.get_params(net, 2, p), opt.m, NAMES, tag)
        assert e.opt_step(net, learner=p) == calls == opt.t


def _assert_losses(got, want, msg):
    np.testing.assert_allclose(got[0], want[0], rtol=1e-4, atol=1e-6, err_msg="critic loss, " + msg)
    np.testing.assert_allclose(got[1], want[1], rtol=1e-4, atol=1e-6, err_msg="actor loss, " + msg)


@pytest.mark.parametrize("name", list(eo.CASES))
def test_golden_and_oracle(N, fx, name):
    """Every case, every call, on the rows and preferences the reference drew: both losses against the reference and the oracle;
    the four nets and both Adam m element-wise against the oracle; the step counts.  The pre-clip gradient norms (the statistics
    the clip coefficient is computed from) against the reference's at rtol 1e-3: a norm is the root of a sum of squares of
    gradient elements that each carry fp32 rounding of relative size ~1e-6 x the row count's root, far inside that."""
    c = eo.case(name)
    inp = eo.inputs(c, seed=int(fx[name + "/seed"]))
    e = _engine(N, c)
    _load(e, inp)
    e.add_batch(_records(e, inp["table"]))
    o = eo.make(c, inp)
    for k in range(c["n_learn"]):
        idx, w = fx[name + "/idx"][k], fx[name + "/weights"][k]
        got = _learn(e, c, idx[None], w[None])
        want = o.learn_with(idx, w, c["gamma"], c["tau"], c["beta"])
        st = e.stats()[0, 0]
        print("%s call %d: critic %.8g reference %.8g oracle %.8g | actor %.8g reference %.8g oracle %.8g | norms %.6g %.6g reference %.6g %.6g"
              % (name, k, got[0][0], fx[name + "/critic_loss"][k], want[0], got[1][0], fx[name + "/actor_loss"][k], want[1],
                 st[ST_CRITIC_GNORM], st[ST_ACTOR_GNORM], fx[name + "/critic_norm"][k], fx[name + "/actor_norm"][k]))
        _assert_losses((got[0][0], got[1][0]), (fx[name + "/critic_loss"][k], fx[name + "/actor_loss"][k]), "call %d vs reference" % k)
        _assert_losses((got[0][0], got[1][0]), want, "call %d vs oracle" % k)
        np.testing.assert_allclose(st[ST_CRITIC_GNORM], fx[name + "/critic_norm"][k], rtol=1e-3, err_msg="critic norm, call %d" % k)
        np.testing.assert_allclose(st[ST_ACTOR_GNORM], fx[name + "/actor_norm"][k], rtol=1e-3, err_msg="actor norm, call %d" % k)
    _check_state(e, o, c, c["n_learn"], name)
    e.close()


# one row; one sample under seven weights (a chunk that ends mid-way); chunks that straddle both a sample wrap and a weight boundary;
# 4096 rows over many chunks; R = 3 is no multiple of 2 (the device draw's pairs); and a one-column action
RAGGED = dict(obs_dim=5, act_dim=3, rdim=3, hidden=32, n_table=300)
# ... and hidden 64, where both heads (<= 4 columns behind a 64-wide layer) take the fused narrow-head path of device/net.hpp
RAGGED_CASES = [(1, 1, 3, 32), (1, 7, 3, 32), (37, 5, 3, 32), (256, 16, 3, 32), (16, 4, 1, 32), (37, 5, 3, 64)]


@pytest.mark.parametrize("B,W,A,H", RAGGED_CASES)
def test_ragged_rows(N, B, W, A, H):
    c = dict(eo.COMMON, **RAGGED, batch=B, weight_num=W, seed=9000 + 10 * B + W)
    c["act_dim"], c["hidden"] = A, H
    inp = eo.inputs(c, n_learn=3)
    e = _engine(N, c, batch_max=4096)
    _load(e, inp)
    e.add_batch(_records(e, inp["table"]))
    o = eo.make(c, inp)
    for k in range(3):
        got = _learn(e, c, inp["idx"][k][None], inp["weights"][k][None])
        want = o.learn_with(inp["idx"][k], inp["weights"][k], c["gamma"], c["tau"], c["beta"])
        print("B %d W %d A %d call %d: critic %.8g oracle %.8g | actor %.8g oracle %.8g" % (B, W, A, k, got[0][0], want[0], got[1][0], want[1]))
        _assert_losses((got[0][0], got[1][0]), want, "call %d" % k)
    _check_state(e, o, c, 3, "B%d W%d A%d H%d" % (B, W, A, H))
    e.close()


@pytest.mark.parametrize("B,W", [(16, 2), (37, 1)])
def test_two_chunks_per_workgroup(N, B, W, monkeypatch):
    """FRL_RC=16, FRL_CPS=2, one learner: a workgroup walks two row chunks and its second chunk ADDS to the slab its first one stored,
    in the critic and in the actor launch (whose parked activations follow the chunk).  16 x 2 = 32 rows: one workgroup, two full
    chunks; 37 rows: a second workgroup with the ragged 5-row chunk."""
    monkeypatch.setenv("FRL_RC", "16")
    monkeypatch.setenv("FRL_CPS", "2")
    c = dict(eo.COMMON, **RAGGED, batch=B, weight_num=W, seed=9700 + 10 * B + W)
    inp = eo.inputs(c, n_learn=2)
    e = _engine(N, c, batch_max=64)
    # rc from the engine; its cps (no getter in the C ABI) is pinned for exactly this engine by the plan on the CPU:
    # tests/test_engine_plan.py::test_rowchunk_addresses_stay_inside_the_plans_buffers ("rc 16 cps 2 S 2")
    assert e.lds_bytes()[1] == 16
    _load(e, inp)
    e.add_batch(_records(e, inp["table"]))
    o = eo.make(c, inp)
    for k in range(2):
        got = _learn(e, c, inp["idx"][k][None], inp["weights"][k][None])
        want = o.learn_with(inp["idx"][k], inp["weights"][k], c["gamma"], c["tau"], c["beta"])
        _assert_losses((got[0][0], got[1][0]), want, "cps2 B %d W %d call %d" % (B, W, k))
    _check_state(e, o, c, 2, "cps2 B%d W%d" % (B, W))
    e.close()


POP = dict(obs_dim=4, act_dim=3, rdim=2, hidden=32, batch=16, weight_num=4, n_table=40)


def pop_inputs(p):
    c = dict(eo.COMMON, **POP, seed=9500 + 10 * p)
    return c, eo.inputs(c, n_learn=2)


@pytest.mark.parametrize("P", [1, 40, 512])
def test_population(N, P):
    """Every learner has its own parameters, table, rows and preferences; learner 0, the two middle ones and the last are held
    to oracles of their own."""
    c = pop_inputs(0)[0]
    e = _engine(N, c, P=P, cap=c["n_table"])
    inps = [pop_inputs(p)[1] for p in range(P)]
    for p in range(P):
        _load(e, inps[p], p)
    e.add_batch(np.concatenate([_records(e, i["table"]) for i in inps]), learners=np.repeat(np.arange(P), c["n_table"]))
    check = sorted({0, max(P // 2 - 1, 0), P // 2, P - 1})
    orc = {p: eo.make(c, inps[p]) for p in check}
    for k in range(2):
        got = _learn(e, c, np.stack([i["idx"][k] for i in inps]), np.stack([i["weights"][k] for i in inps]))
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
        for p in check:
            want = orc[p].learn_with(inps[p]["idx"][k], inps[p]["weights"][k], c["gamma"], c["tau"], c["beta"])
            _assert_losses((got[0][p], got[1][p]), want, "learner %d call %d" % (p, k))
    for p in check:
        _check_state(e, orc[p], c, 2, "P%d learner %d" % (P, p), p)
    e.close()


def test_device_weights(N):
    """weights = NULL: |N(0,1)| / L1 norm from the engine's Philox stream, returned in weights_out."""
    c = dict(eo.COMMON, obs_dim=4, act_dim=3, rdim=2, hidden=32, batch=1, weight_num=2048, n_table=40, seed=9700)
    inp = eo.inputs(c, n_learn=2)
    idx = np.array([[3], [17]], np.int64)

    def fresh():
        e = _engine(N, c, P=2, cap=c["n_table"], seed=5)
        for p in range(2):
            _load(e, inp, p)
        e.add_batch(np.concatenate([_records(e, inp["table"])] * 2), learners=np.repeat(np.arange(2), c["n_table"]))
        return e
    e = fresh()
    kw = dict(gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], beta=c["beta"], idx=idx)
    out1 = e.envelope_ddpg_learn(1, 2048, want_loss=True, want_weights=True, **kw)
    out2 = e.envelope_ddpg_learn(1, 2048, want_loss=True, want_weights=True, **kw)
    for w in (out1["weights"], out2["weights"]):
        assert w.shape == (2, 2048, 2) and np.all(np.isfinite(w)) and np.all(w >= 0)
        np.testing.assert_allclose(w.sum(axis=2), 1.0, rtol=0, atol=1e-6)
        assert not np.array_equal(w[0], w[1])                       # learners draw their own
    assert not np.array_equal(out1["weights"], out2["weights"])     # ... and so does every call
    e.close()
    e2 = fresh()
    back = e2.envelope_ddpg_learn(1, 2048, weights=out1["weights"], want_loss=True, **kw)
    for key in ("critic_loss", "actor_loss"):
        assert np.array_equal(back[key], out1[key]) and np.all(np.isfinite(back[key])), key      # bit for bit
    e2.close()


def test_device_indices(N):
    c = dict(eo.COMMON, obs_dim=4, act_dim=3, rdim=2, hidden=32, batch=16, weight_num=4, n_table=40, seed=9800)
    inp = eo.inputs(c, n_learn=1)
    e = _engine(N, c, cap=c["n_table"])
    _load(e, inp)
    e.add_batch(_records(e, inp["table"]))
    before = [e.get_params(0), e.get_params(1)]
    kw = dict(gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], beta=c["beta"])
    out = e.envelope_ddpg_learn(16, 4, weights=inp["weights"][0][None], want_loss=True, **kw)
    assert np.isfinite(out["critic_loss"][0]) and out["critic_loss"][0] > 0 and np.isfinite(out["actor_loss"][0])
    rows = e.last_indices(16)[0, 0]
    assert len(set(rows.tolist())) == 16 and rows.min() >= 0 and rows.max() < c["n_table"]
    for net in (0, 1):
        after = e.get_params(net)
        assert np.all(np.isfinite(after)) and not np.array_equal(before[net], after)
    out = e.envelope_ddpg_learn(16, 4, want_loss=True, **kw)      # both drawn on the device
    assert np.isfinite(out["critic_loss"][0]) and e.opt_step(0) == 2 and e.opt_step(1) == 2
    e.close()


def test_class(N, fx, tmp_path):
    """freerl_amd.ENVELOPE_DDPG.ENVELOPE_DDPG through the class case's script (ring of 40 rows that wraps): select_action's
    actions, the priorities, the homotopy on beta, the prioritised draws and every call's losses against the reference's record."""
    from freerl_amd.ENVELOPE_DDPG import ENVELOPE_DDPG
    c = eo.case("class")
    seed = int(fx["class/seed"])
    inp = eo.inputs(c, seed=seed)
    t = inp["table"]
    dims = [c["obs_dim"], c["act_dim"], c["rdim"]]
    kw = dict(hidden=c["hidden"], max_rows=c["batch"] * c["weight_num"])
    pol = ENVELOPE_DDPG(dims, True, c["actor_lr"], c["critic_lr"], c["capacity"], "cpu", c["beta"], c["max_episodes"], **kw)
    for net, tgt, key in ((pol.agent.actor, pol.agent.actor_target, "actor"), (pol.agent.critic, pol.agent.critic_target, "critic")):
        sd = {k: torch.as_tensor(v) for k, v in inp[key].items()}
        net.load_state_dict(sd)
        tgt.load_state_dict(sd)
    np.random.seed(seed)
    torch.manual_seed(seed)
    learn_at, k = eo.class_schedule(c), 0
    for i in range(c["n_steps"]):
        act = pol.select_action(t["obs"][i])
        assert act.shape == (c["act_dim"],)
        np.testing.assert_allclose(act, fx["class/action"][i], rtol=1e-4, atol=1e-6, err_msg="select_action at step %d" % i)
        pol.add(t["obs"][i], t["act"][i], t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"])
        np.testing.assert_allclose(float(pol.priority_mem[-1]), fx["class/priority"][i], rtol=1e-4, err_msg="priority at step %d" % i)
        assert abs(pol.beta - float(fx["class/beta"][i])) <= 1e-12
        if i in learn_at:
            pol.learn(c["batch"], c["gamma"], c["tau"], c["weight_num"], 1)
            np.testing.assert_array_equal(pol.last_indices, fx["class/idx"][k])
            np.testing.assert_array_equal(pol.last_weights, fx["class/weights"][k])
            _assert_losses((pol.loss.item(), pol.actor_loss.item()), (fx["class/critic_loss"][k], fx["class/actor_loss"][k]), "learn() call %d" % k)
            k += 1
    assert k == c["n_learn"] and len(pol.buffer) == c["capacity"] == len(pol.priority_mem)
    np.testing.assert_allclose(np.array(pol.priority_mem, np.float64), fx["class/final_priority"], rtol=1e-4)
    obs, act, rew, nobs, done = pol.sample(5)
    assert rew.shape == (5, c["rdim"]) and done.shape == (5, 1) and act.shape == (5, c["act_dim"]) and obs.shape == nobs.shape == (5, c["obs_dim"])
    # checkpoint: the reference's keys and shapes (the actor's state_dict), and a round trip
    want = pol.agent.actor.state_dict()
    H, O, A, R = c["hidden"], c["obs_dim"], c["act_dim"], c["rdim"]
    assert {k2: tuple(v.shape) for k2, v in want.items()} == {"l1.weight": (H, O + R), "l1.bias": (H,), "l2.weight": (H, H), "l2.bias": (H,),
                                                            "l3.weight": (A, H), "l3.bias": (A,)}
    assert {k2: tuple(v.shape) for k2, v in pol.agent.critic_target.state_dict().items()}["l1.weight"] == (H, O + A + R)
    pol.save(str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "ENVELOPE_DDPG.pt"))
    back = ENVELOPE_DDPG.load(dims, True, str(tmp_path), **kw)
    for k2, v in back.agent.actor.state_dict().items():
        assert torch.equal(v, want[k2]), k2
    np.testing.assert_array_equal(back.evaluate_action(t["obs"][0], [0.5, 0.5]), pol.evaluate_action(t["obs"][0], [0.5, 0.5]))
    with pytest.raises(ValueError):
        ENVELOPE_DDPG(dims, False, c["actor_lr"], c["critic_lr"], c["capacity"], "cpu", c["beta"], c["max_episodes"], **kw)


def test_rejections(N):
    import ctypes as C
    from freerl_amd.engine import Engine
    c = dict(eo.COMMON, obs_dim=4, act_dim=3, rdim=2, hidden=32, batch=8, weight_num=4, n_table=40, seed=9900)
    with pytest.raises(N.FrlError, match="hidden"):
        Engine(N.ALGO_ENVELOPE_DDPG, 4, 3, 40, hidden=512, batch_max=32, reward_dim=2)
    with pytest.raises(N.FrlError, match="hidden"):
        Engine(N.ALGO_ENVELOPE_DDPG, 4, 3, 40, hidden=40, batch_max=32, reward_dim=2)
    with pytest.raises(N.FrlError, match="reward_dim"):
        Engine(N.ALGO_ENVELOPE_DDPG, 4, 3, 40, hidden=32, batch_max=32, reward_dim=-1)
    with pytest.raises(N.FrlError, match="80 KB"):                      # 1000 observation columns at hidden 256: no two workgroups per CU
        Engine(N.ALGO_ENVELOPE_DDPG, 1000, 3, 40, hidden=256, batch_max=32, reward_dim=2)
    inp = eo.inputs(c, n_learn=1)
    e = _engine(N, c, cap=64)
    assert e.reward_dim == 2 and e.layout.done_off == e.layout.rew_off + 2 and e.n_nets == 2
    _load(e, inp)
    e.add_batch(_records(e, inp["table"])[:20])
    before = [e.get_params(0), e.get_params(1)]
    ok = dict(gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, beta=0.5)
    idx, w = inp["idx"][0][None] % 20, inp["weights"][0][None]
    for B, W, kw, msg in ((0, 4, {}, "batch"), (8, 0, {}, "weight_num"), (8, 5, {}, "batch_max"), (21, 1, {}, "rows"),
                          (8, 4, dict(gamma=float("nan")), "NaN"), (8, 4, dict(tau=float("nan")), "NaN"),
                          (8, 4, dict(actor_lr=float("nan")), "NaN"), (8, 4, dict(critic_lr=float("nan")), "NaN"),
                          (8, 4, dict(beta=float("nan")), "NaN"), (8, 4, dict(beta=1.5), "beta"), (8, 4, dict(beta=-0.1), "beta")):
        with pytest.raises(N.FrlError, match=msg):
            e.envelope_ddpg_learn(B, W, **dict(ok, **kw), idx=idx[:, :B] if 0 < B <= 8 else None, weights=w[:, :W] if 0 < W <= 4 else None)
    with pytest.raises(N.FrlError, match="2\\*batch"):                  # the device draw needs twice the batch in the ring
        e.envelope_ddpg_learn(12, 1, **ok)
    for call in (lambda: e.learn(8, gamma=0.99, tau=0.01, critic_lr=1e-3), lambda: e.learn_path(8), lambda: e.learn_work(8),
                 lambda: e.learn_work_executed(8), lambda: e.envelope_learn(8, 4, gamma=0.99, tau=0.01, lr=1e-3, beta=0.5),
                 lambda: e.reinforce_learn(gamma=0.99, lr=1e-3),
                 lambda: e.act_explore(N.ACT_TANHHEAD, np.zeros((1, 1, 4), np.float32), kind=N.EXPLORE_GAUSS)):
        with pytest.raises(N.FrlError, match="error 4.*frl_envelope_ddpg_learn"):      # FRL_ERR_STATE, and the message names the entry point to use
            call()
    ra, st = N.RolloutArgs(), N.RolloutStats()
    assert e._L.frl_rollout(e._h, None, C.byref(ra), C.byref(st)) == 4 and b"frl_envelope_ddpg_learn" in e._L.frl_last_error()
    for net in (0, 1):
        assert np.array_equal(before[net], e.get_params(net)) and e.opt_step(net) == 0      # nothing was launched
    got = _learn(e, c, idx, w)
    assert np.isfinite(got[0][0]) and np.isfinite(got[1][0])                                # ... and the engine still works
    e.close()
    # the other direction: an envelope-DQN engine and a DDPG engine refuse frl_envelope_ddpg_learn, a DDPG engine frl_envelope_learn
    q = Engine(N.ALGO_ENVELOPE_DQN, 4, 3, 40, discrete=True, hidden=32, batch_max=32, reward_dim=2)
    with pytest.raises(N.FrlError, match="error 4.*frl_envelope_learn"):
        q.envelope_ddpg_learn(8, 4, **ok)
    q.close()
    d = Engine(N.ALGO_DDPG, 4, 3, 40, batch_max=32)
    with pytest.raises(N.FrlError, match="error 4.*frl_envelope_ddpg_learn"):
        d.envelope_ddpg_learn(8, 4, **ok)
    with pytest.raises(N.FrlError, match="error 4.*frl_envelope_learn"):
        d.envelope_learn(8, 4, gamma=0.99, tau=0.01, lr=1e-3, beta=0.5)
    d.close()
