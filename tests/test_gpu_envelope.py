"""GPU: envelope multi-objective DQN (ENVELOPE_MORL_file/ENVELOPE_DQN.py) on kernels_envelope.hip, against the reference's
outputs (tests/golden/envelope_dqn.npz) and the NumPy restatement (tests/envelope_oracle.py).

a' is an argmax, so every comparison runs on inputs whose margin — the gap between the two largest w . Q_online(s') of a row — is
at least envelope_oracle.MARGIN on the oracle's values (asserted); no row is masked out of any comparison."""
import os

import numpy as np
import pytest
import torch

from tests import envelope_oracle as eo
from tests.hip_helpers import flat_params, unflat_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["l1", "l2", "l3"]


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "envelope_dqn.npz")))


def _engine(N, c, P=1, cap=None, batch_max=None, **kw):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_ENVELOPE_DQN, kw.get("obs_dim", c["obs_dim"]), kw.get("n_act", c["n_act"]), cap or c["n_table"], n_learners=P,
                  discrete=True, hidden=kw.get("hidden", c["hidden"]), batch_max=batch_max or c["batch"] * c["weight_num"],
                  reward_dim=kw.get("rdim", c["rdim"]), seed=kw.get("seed", 0))


def _records(e, t):
    lay, n = e.layout, len(t["done"])
    rec = np.zeros((n, e.width), np.float32)
    O, R = t["obs"].shape[1], t["rew"].shape[1]
    assert lay.done_off - lay.rew_off == R == e.reward_dim
    rec[:, lay.obs_off[0]:lay.obs_off[0] + O] = t["obs"]
    rec[:, lay.act_off[0]] = t["act"][:, 0]
    rec[:, lay.rew_off:lay.rew_off + R] = t["rew"]
    rec[:, lay.done_off] = t["done"]
    rec[:, lay.next_obs_off[0]:lay.next_obs_off[0] + O] = t["next_obs"]
    return rec


def _load(e, params, p=0):
    for kind in (0, 1):
        e.set_params(0, flat_params(params, NAMES), kind, learner=p)


def _learn(e, c, idx, w, beta=None, **kw):
    return e.envelope_learn(np.asarray(idx).shape[-1], np.asarray(w).shape[-2], gamma=c["gamma"], tau=c["tau"], lr=c["lr"],
                            beta=c["beta"] if beta is None else beta, idx=idx, weights=w, want_loss=True, **kw)["loss"]


# Parameter tolerances: test_gpu_sac_discrete.py's rules (two fp32 implementations of one update differ by rounding in every
# gradient element, and a ReLU unit within rounding of zero may be open in one and shut in the other): >= 99 % of a net's elements
# within (rtol, atol), none further than Adam can move an element in `calls` steps; the first moment within 2e-3 of its largest on
# >= 99 % of a matrix, within 5e-2 everywhere (2e-2 for bias vectors).
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
    _assert_net(e.get_params(0, 0, p), o.q, NAMES, 5e-4, 5e-6, c["lr"], calls, label + " net")
    _assert_net(e.get_params(0, 1, p), o.q_t, NAMES, 5e-4, 5e-6, c["lr"], calls, label + " target")
    _assert_m(e.get_params(0, 2, p), o.opt.m, NAMES, label)
    assert e.opt_step(0, learner=p) == calls == o.opt.t


@pytest.mark.parametrize("name", list(eo.CASES))
def test_golden_and_oracle(N, fx, name):
    """Every case, every call, on the rows and preferences the reference drew: the loss against the reference and the oracle;
    net, target and Adam m element-wise against the oracle; the step count."""
    c = eo.case(name)
    inp = eo.inputs(c, seed=int(fx[name + "/seed"]))
    e = _engine(N, c)
    _load(e, inp["params"])
    e.add_batch(_records(e, inp["table"]))
    o = eo.make(c, inp)
    for k in range(c["n_learn"]):
        idx, w = fx[name + "/idx"][k], fx[name + "/weights"][k]
        got = _learn(e, c, idx[None], w[None])[0]
        want = o.learn_with(idx, w, c["gamma"], c["tau"], c["beta"])
        print("%s call %d: loss %.8g reference %.8g oracle %.8g" % (name, k, got, fx[name + "/loss"][k], want))
        np.testing.assert_allclose(got, fx[name + "/loss"][k], rtol=1e-4, atol=1e-6, err_msg="call %d vs reference" % k)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg="call %d vs oracle" % k)
    assert o.min_gap >= 0.5 * eo.MARGIN and float(fx[name + "/min_gap"]) >= eo.MARGIN
    _check_state(e, o, c, c["n_learn"], name)
    e.close()


# (B, W) -> the first seed from 9000 up whose inputs meet the margin on the oracle's values over the test's 3 calls (found on the CPU
# with the oracle; the test asserts the margin again).  Two actions and head weights scaled by 8 (no head bias) keep near-ties rare
# enough at 4096 rows x 3 calls while both actions are chosen.
RAGGED = dict(obs_dim=5, n_act=2, rdim=2, hidden=32, n_table=300, head_scale=8.0)
RAGGED_SEEDS = {(1, 1): 9000, (1, 7): 9000, (37, 5): 9000, (256, 16): 9000}


def ragged_inputs(B, W, seed, calls=3):
    c = dict(eo.COMMON, **RAGGED, batch=B, weight_num=W, seed=seed)
    inp = eo.inputs(c, n_learn=calls)
    inp["params"]["l3.weight"] = (inp["params"]["l3.weight"] * np.float32(RAGGED["head_scale"])).astype(np.float32)
    inp["params"]["l3.bias"] = np.zeros_like(inp["params"]["l3.bias"])        # (a bias gap would decide every row's a' alone)
    return c, inp


@pytest.mark.parametrize("B,W", list(RAGGED_SEEDS))
def test_ragged_rows(N, B, W):
    """Row counts that end inside a chunk, one row, one sample under seven weights, chunks that straddle both boundaries, and 4096
    rows over many chunks, on an engine whose batch_max (4096) is not the call's row count."""
    c, inp = ragged_inputs(B, W, RAGGED_SEEDS[(B, W)])
    e = _engine(N, c, batch_max=4096)
    _load(e, inp["params"])
    e.add_batch(_records(e, inp["table"]))
    o = eo.make(c, inp)
    for k in range(3):
        got = _learn(e, c, inp["idx"][k][None], inp["weights"][k][None])[0]
        want = o.learn_with(inp["idx"][k], inp["weights"][k], c["gamma"], c["tau"], c["beta"])
        print("B %d W %d call %d: loss %.8g oracle %.8g" % (B, W, k, got, want))
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg="call %d" % k)
    assert o.min_gap >= eo.MARGIN, "the inputs' argmax margin %.3g" % o.min_gap
    _check_state(e, o, c, 3, "B%d W%d" % (B, W))
    e.close()


@pytest.mark.parametrize("B,W", [(16, 2), (37, 1)])
def test_two_chunks_per_workgroup(N, B, W, monkeypatch):
    """FRL_RC=16, FRL_CPS=2, one learner: a workgroup walks two row chunks and its second chunk ADDS to the slab its first one stored.
    16 x 2 = 32 rows: one workgroup, two full chunks; 37 rows: a second workgroup with the ragged 5-row chunk."""
    monkeypatch.setenv("FRL_RC", "16")
    monkeypatch.setenv("FRL_CPS", "2")
    c, inp = ragged_inputs(B, W, 9100, calls=2)
    e = _engine(N, c, batch_max=64)
    # rc from the engine; its cps (no getter in the C ABI) is pinned for exactly this engine by the plan on the CPU:
    # tests/test_engine_plan.py::test_rowchunk_addresses_stay_inside_the_plans_buffers ("rc 16 cps 2 S 2")
    assert e.lds_bytes()[1] == 16
    _load(e, inp["params"])
    e.add_batch(_records(e, inp["table"]))
    o = eo.make(c, inp)
    for k in range(2):
        got = _learn(e, c, inp["idx"][k][None], inp["weights"][k][None])[0]
        want = o.learn_with(inp["idx"][k], inp["weights"][k], c["gamma"], c["tau"], c["beta"])
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg="cps2 B %d W %d call %d" % (B, W, k))
    assert o.min_gap >= eo.MARGIN, "the inputs' argmax margin %.3g" % o.min_gap
    _check_state(e, o, c, 2, "cps2 B%d W%d" % (B, W))
    e.close()


POP = dict(obs_dim=4, n_act=3, rdim=2, hidden=32, batch=16, weight_num=4, n_table=40)
POP_SEED = 9503      # the first base from 9500 up whose checked learners (all three populations) meet the margin


def pop_inputs(p):
    c = dict(eo.COMMON, **POP, seed=POP_SEED + 10 * p)
    return c, eo.inputs(c, n_learn=2)


@pytest.mark.parametrize("P", [1, 40, 512])
def test_population(N, P):
    """Every learner has its own parameters, table, rows and preferences; learner 0, the two middle ones and the last are held
    to oracles of their own."""
    c = pop_inputs(0)[0]
    e = _engine(N, c, P=P, cap=c["n_table"])
    inps = [pop_inputs(p)[1] for p in range(P)]
    for p in range(P):
        _load(e, inps[p]["params"], p)
    e.add_batch(np.concatenate([_records(e, i["table"]) for i in inps]), learners=np.repeat(np.arange(P), c["n_table"]))
    check = sorted({0, max(P // 2 - 1, 0), P // 2, P - 1})
    orc = {p: eo.make(c, inps[p]) for p in check}
    for k in range(2):
        got = _learn(e, c, np.stack([i["idx"][k] for i in inps]), np.stack([i["weights"][k] for i in inps]))
        assert np.all(np.isfinite(got))
        for p in check:
            want = orc[p].learn_with(inps[p]["idx"][k], inps[p]["weights"][k], c["gamma"], c["tau"], c["beta"])
            np.testing.assert_allclose(got[p], want, rtol=1e-4, atol=1e-6, err_msg="learner %d call %d" % (p, k))
    for p in check:
        assert orc[p].min_gap >= eo.MARGIN, "learner %d: argmax margin %.3g" % (p, orc[p].min_gap)
        _check_state(e, orc[p], c, 2, "P%d learner %d" % (P, p), p)
    e.close()


def test_device_weights(N):
    """weights = NULL: |N(0,1)| / L1 norm from the engine's Philox stream, returned in weights_out."""
    c = dict(eo.COMMON, obs_dim=4, n_act=3, rdim=2, hidden=32, batch=1, weight_num=2048, n_table=40, seed=9700)
    inp = eo.inputs(c, n_learn=2)
    idx = np.array([[3], [17]], np.int64)

    def fresh():
        e = _engine(N, c, P=2, cap=c["n_table"], seed=5)
        for p in range(2):
            _load(e, inp["params"], p)
        e.add_batch(np.concatenate([_records(e, inp["table"])] * 2), learners=np.repeat(np.arange(2), c["n_table"]))
        return e
    e = fresh()
    kw = dict(gamma=c["gamma"], tau=c["tau"], lr=c["lr"], beta=c["beta"], idx=idx)
    out1 = e.envelope_learn(1, 2048, want_loss=True, want_weights=True, **kw)
    out2 = e.envelope_learn(1, 2048, want_loss=True, want_weights=True, **kw)
    for w in (out1["weights"], out2["weights"]):
        assert w.shape == (2, 2048, 2) and np.all(np.isfinite(w)) and np.all(w >= 0)
        np.testing.assert_allclose(w.sum(axis=2), 1.0, rtol=0, atol=1e-6)
        assert not np.array_equal(w[0], w[1])                       # learners draw their own
    assert not np.array_equal(out1["weights"], out2["weights"])     # ... and so does every call
    # 4096 drawn rows: by symmetry the first component's mean is 0.5, its standard deviation at that count under 0.006
    assert abs(float(out1["weights"][:, :, 0].mean()) - 0.5) <= 0.02
    e.close()
    e2 = fresh()
    back = e2.envelope_learn(1, 2048, weights=out1["weights"], want_loss=True, **kw)
    assert np.array_equal(back["loss"], out1["loss"]) and np.all(np.isfinite(back["loss"]))      # bit for bit
    e2.close()


def test_device_indices(N):
    c = dict(eo.COMMON, obs_dim=4, n_act=3, rdim=2, hidden=32, batch=16, weight_num=4, n_table=40, seed=9800)
    inp = eo.inputs(c, n_learn=1)
    e = _engine(N, c, cap=c["n_table"])
    _load(e, inp["params"])
    e.add_batch(_records(e, inp["table"]))
    before = e.get_params(0)
    out = e.envelope_learn(16, 4, gamma=c["gamma"], tau=c["tau"], lr=c["lr"], beta=c["beta"], weights=inp["weights"][0][None], want_loss=True)
    assert np.isfinite(out["loss"][0]) and out["loss"][0] > 0
    rows = e.last_indices(16)[0, 0]
    assert len(set(rows.tolist())) == 16 and rows.min() >= 0 and rows.max() < c["n_table"]
    after = e.get_params(0)
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)
    out = e.envelope_learn(16, 4, gamma=c["gamma"], tau=c["tau"], lr=c["lr"], beta=c["beta"], want_loss=True)      # both drawn on the device
    assert np.isfinite(out["loss"][0]) and e.opt_step(0) == 2
    e.close()


def test_class(N, fx, tmp_path):
    """freerl_amd.ENVELOPE_DQN.ENVELOPE through the class case's script (ring of 40 rows that wraps): the priorities, the homotopy
    on beta, the prioritised draws, select_action's choices and every call's loss against the reference's record."""
    from freerl_amd.ENVELOPE_DQN import ENVELOPE
    c = eo.case("class")
    seed = int(fx["class/seed"])
    inp = eo.inputs(c, seed=seed)
    t = inp["table"]
    dims = [c["obs_dim"], c["n_act"], c["rdim"]]
    kw = dict(hidden=c["hidden"], max_rows=c["batch"] * c["weight_num"])
    pol = ENVELOPE(dims, False, c["lr"], c["capacity"], "cpu", c["beta"], c["max_episodes"], **kw)
    sd = {k: torch.as_tensor(v) for k, v in inp["params"].items()}
    pol.agent.Qnet.load_state_dict(sd)
    pol.agent.Qnet_target.load_state_dict(sd)
    np.random.seed(seed)
    torch.manual_seed(seed)
    learn_at, k = eo.class_schedule(c), 0
    for i in range(c["n_steps"]):
        assert int(pol.select_action(t["obs"][i])) == int(fx["class/choice"][i]), "select_action at step %d" % i
        pol.add(t["obs"][i], int(t["act"][i, 0]), t["rew"][i], t["next_obs"][i], bool(t["done"][i]), c["gamma"])
        np.testing.assert_allclose(float(pol.priority_mem[-1]), fx["class/priority"][i], rtol=1e-4, err_msg="priority at step %d" % i)
        assert abs(pol.beta - float(fx["class/beta"][i])) <= 1e-12
        if i in learn_at:
            pol.learn(c["batch"], c["gamma"], c["tau"], c["weight_num"], 1)
            np.testing.assert_array_equal(pol.last_indices, fx["class/idx"][k])
            np.testing.assert_array_equal(pol.last_weights, fx["class/weights"][k])
            np.testing.assert_allclose(pol.loss.item(), fx["class/loss"][k], rtol=1e-4, atol=1e-6, err_msg="learn() call %d" % k)
            k += 1
    assert k == c["n_learn"] and len(pol.buffer) == c["capacity"] == len(pol.priority_mem)
    np.testing.assert_allclose(np.array(pol.priority_mem, np.float64), fx["class/final_priority"], rtol=1e-4)
    obs, act, rew, nobs, done = pol.sample(5)
    assert rew.shape == (5, c["rdim"]) and done.shape == (5, 1) and rew.dtype == done.dtype == torch.float32 and obs.shape == nobs.shape == (5, c["obs_dim"])
    # checkpoint: the reference's keys and shapes, and a round trip
    want = pol.agent.Qnet.state_dict()
    H, O, A, R = c["hidden"], c["obs_dim"], c["n_act"], c["rdim"]
    assert {k2: tuple(v.shape) for k2, v in want.items()} == {"l1.weight": (H, O + R), "l1.bias": (H,), "l2.weight": (H, H), "l2.bias": (H,),
                                                            "l3.weight": (A * R, H), "l3.bias": (A * R,)}
    pol.save(str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "ENVELOPE_DQN.pt"))
    back = ENVELOPE.load(dims, False, str(tmp_path), **kw)
    for k2, v in back.agent.Qnet.state_dict().items():
        assert torch.equal(v, want[k2]), k2
    assert int(back.evaluate_action(t["obs"][0], [0.5, 0.5])) == int(pol.evaluate_action(t["obs"][0], [0.5, 0.5]))
    with pytest.raises(ValueError):
        ENVELOPE(dims, True, c["lr"], c["capacity"], "cpu", c["beta"], c["max_episodes"], **kw)


def test_rejections(N):
    from freerl_amd.engine import Engine
    c = dict(eo.COMMON, obs_dim=4, n_act=3, rdim=2, hidden=32, batch=8, weight_num=4, n_table=40, seed=9900)
    with pytest.raises(N.FrlError, match="65|head columns"):
        Engine(N.ALGO_ENVELOPE_DQN, 4, 13, 40, discrete=True, hidden=32, batch_max=32, reward_dim=5)
    with pytest.raises(N.FrlError, match="hidden"):
        Engine(N.ALGO_ENVELOPE_DQN, 4, 3, 40, discrete=True, hidden=512, batch_max=32, reward_dim=2)
    with pytest.raises(N.FrlError, match="hidden"):
        Engine(N.ALGO_ENVELOPE_DQN, 4, 3, 40, discrete=True, hidden=40, batch_max=32, reward_dim=2)
    inp = eo.inputs(c, n_learn=1)
    e = _engine(N, c, cap=64)
    assert e.reward_dim == 2 and e.layout.done_off == e.layout.rew_off + 2
    _load(e, inp["params"])
    e.add_batch(_records(e, inp["table"])[:20])
    before = e.get_params(0)
    ok = dict(gamma=0.99, tau=0.01, lr=1e-3, beta=0.5)
    idx, w = inp["idx"][0][None] % 20, inp["weights"][0][None]
    for B, W, kw, msg in ((0, 4, {}, "batch"), (8, 0, {}, "weight_num"), (8, 5, {}, "batch_max"), (21, 1, {}, "rows"),
                          (8, 4, dict(gamma=float("nan")), "NaN"), (8, 4, dict(tau=float("nan")), "NaN"), (8, 4, dict(lr=float("nan")), "NaN"),
                          (8, 4, dict(beta=float("nan")), "NaN"), (8, 4, dict(beta=1.5), "beta"), (8, 4, dict(beta=-0.1), "beta")):
        with pytest.raises(N.FrlError, match=msg):
            e.envelope_learn(B, W, **dict(ok, **kw), idx=idx[:, :B] if 0 < B <= 8 else None,
                             weights=w[:, :W] if 0 < W <= 4 else None)
    with pytest.raises(N.FrlError, match="2\\*batch"):                  # the device draw needs twice the batch in the ring
        e.envelope_learn(12, 1, **ok)
    for call, name in ((lambda: e.learn(8, gamma=0.99, tau=0.01, critic_lr=1e-3), "frl_envelope_learn"),
                       (lambda: e.learn_path(8), "frl_envelope_learn"), (lambda: e.learn_work(8), "frl_envelope_learn"),
                       (lambda: e.learn_work_executed(8), "frl_envelope_learn"),
                       (lambda: e.act_explore(N.ACT_ARGMAX, np.zeros((1, 1, 4), np.float32), kind=N.EXPLORE_EPS_GREEDY), "frl_act")):
        with pytest.raises(N.FrlError, match="error 4.*" + name):      # FRL_ERR_STATE, and the message names the entry point to use
            call()
    import ctypes as C
    ra, st = N.RolloutArgs(), N.RolloutStats()
    assert e._L.frl_rollout(e._h, None, C.byref(ra), C.byref(st)) == 4 and b"frl_envelope_learn" in e._L.frl_last_error()
    assert np.array_equal(before, e.get_params(0)) and e.opt_step(0) == 0      # nothing was launched
    assert np.isfinite(_learn(e, c, idx, w)[0])                                # ... and the engine still works
    e.close()
    d = Engine(N.ALGO_DQN, 4, 3, 40, discrete=True, batch_max=32)
    with pytest.raises(N.FrlError, match="error 4.*frl_envelope_learn"):
        d.envelope_learn(8, 4, **ok)
    d.close()
