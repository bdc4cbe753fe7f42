"""GPU: REINFORCE (REINFORCE_file/REINFORCE.py) on kernels_reinforce.hip, against the reference's outputs
(tests/golden/reinforce.npz, long_reinforce.npz, loop_reinforce_cartpole.npz) and the NumPy restatement
(tests/reinforce_oracle.py).

Loss tolerances are stated against s = sum_t |log pi_t * g_t| (the loss is a signed sum with cancellation): four times the
figure tests/test_reinforce_oracle.py records per case — the kernel's tile-order sum and torch's sequential sum are two float32
roundings of one sum.  Normalised returns: four times the recorded float32-vs-float64 figure, of max |g|.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import reinforce_oracle as ro
from tests.golden import synth
from tests.hip_helpers import flat_params, records
from tests.test_gpu_sac_discrete import _assert_m, _assert_net
from tests.test_reinforce_oracle import FIGURES

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["l1", "l2"]


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


def _engine(N, c, P=1, cap=None):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_REINFORCE, c["obs_dim"], c["n_act"], cap or max(c["Ts"]), n_learners=P, discrete=True, hidden=c["hidden"])


def _recs(call):
    T = len(call["rew"])
    return records([dict(obs=call["obs"], act=call["act"].astype(np.float32).reshape(T, 1), rew=call["rew"], done=call["done"],
                         next_obs=np.zeros_like(call["obs"]))])


def _state(e, p=0):
    return [e.get_params(0, k, p) for k in (0, 2, 3)] + [e.opt_step(0, p), e.cursor(p)]


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3:] == b[3:]


def _check_call(out, p, r, fig, ref_loss=None, label=""):
    """One learner's loss and normalised returns of one call against the oracle's (and the reference's loss)."""
    T = len(r["ghat"])
    loss, tol = float(out["loss"][p]), 4 * fig[0] * r["s"]
    print("%s loss %.9g oracle %.9g%s  |d|/s %.3g (bound %.3g)" % (label, loss, float(r["loss"]), "" if ref_loss is None else " reference %.9g" % ref_loss,
                                                                  abs(loss - float(r["loss"])) / max(r["s"], 1e-30), 4 * fig[0]))
    gd = np.abs(out["returns"][p, :T].astype(np.float64) - r["ghat"].astype(np.float64)).max()
    gmax = max(float(np.abs(r["ghat"]).max()), 1e-30)
    print("%s returns max |d| / max |g| %.3g (bound %.3g)" % (label, gd / gmax, 4 * fig[1]))
    assert abs(loss - float(r["loss"])) <= tol, "%s: loss %r vs oracle %r (s %.3g)" % (label, loss, float(r["loss"]), r["s"])
    if ref_loss is not None:
        assert abs(loss - float(ref_loss)) <= tol, "%s: loss %r vs reference %r (s %.3g)" % (label, loss, float(ref_loss), r["s"])
    assert gd <= 4 * fig[1] * gmax, "%s: normalised returns off by %.3g of max |g|" % (label, gd / gmax)
    assert np.isnan(out["returns"][p, T:]).all(), label + ": rows past the learner's length were written"


@pytest.mark.parametrize("name", list(ro.CASES))
def test_golden_and_oracle(N, name):
    """Every case, every call: loss against the reference and the oracle, normalised returns against the oracle, then the net and
    Adam's first moment element-wise against the oracle (test_gpu_sac_discrete.py's rules).  `flat`: nothing but the step count
    moves, bit for bit.  `clamp`: the clamped rows' log-probs are log(eps) / log(1 - eps) exactly."""
    fx = np.load(os.path.join(GOLDEN, "reinforce.npz"))
    c = ro.case(name)
    inp = ro.inputs(c)
    e = _engine(N, c)
    e.set_params(0, flat_params(inp["params"], NAMES))
    o = ro.Reinforce(inp["params"], c["lr"])
    for k, call in enumerate(inp["calls"]):
        T = len(call["rew"])
        if name == "clamp":       # select_action's log-prob of the forced action (Exp(1) draws that leave it no rival), before the update
            q = np.ones((T, c["n_act"]), np.float32)
            q[np.arange(T), call["act"]] = 1e-30
            a, lp = e.act(0, N.ACT_CAT_SAMPLE, call["obs"][None], eps=q[None], want_logp=True)
            np.testing.assert_array_equal(a[0, :, 0], call["act"])
            shut = call["obs"][:, -1] == 0
            lo, hi = np.log(np.float32(ro.EPS)), np.log(np.float32(1) - np.float32(ro.EPS))
            want = np.where(call["act"] == 0, hi, lo).astype(np.float32)
            np.testing.assert_array_equal(lp[0, shut, 0], want[shut], err_msg="clamped rows, call %d" % k)
            np.testing.assert_allclose(lp[0, :, 0], fx["clamp/logp"][sum(c["Ts"][:k]):sum(c["Ts"][:k]) + T], rtol=1e-5, atol=2e-5)
        before = _state(e)
        e.add_batch(_recs(call))
        assert e.cursor() == (T % e.capacity, T)
        out = e.reinforce_learn(gamma=c["gamma"], lr=c["lr"], n_steps=None if k % 2 else [T], want_loss=True, want_returns=True)
        r = o.learn_with(call["obs"], call["act"], call["rew"], call["done"], c["gamma"])
        _check_call(out, 0, r, FIGURES[name], fx[name + "/loss"][k], "%s call %d (T %d)" % (name, k, T))
        assert e.cursor() == (0, 0) and e.opt_step(0) == k + 1
        if name == "flat":
            after = _state(e)
            assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3])), "flat: the net, m or v moved in call %d" % k
            assert out["loss"][0] == 0 and not out["returns"][0, :T].any()
    _assert_net(e.get_params(0, 0), o.p, NAMES, 5e-4, 5e-6, c["lr"], c["n_learn"], name + " policy")
    _assert_m(e.get_params(0, 2), o.m, NAMES, name + " policy")
    assert e.opt_step(0) == int(fx[name + "/step"]) == c["n_learn"]
    assert e.pad_max(0) == 0 and e.pad_max(0, 2) == 0
    st = e.stats()
    assert st[0, 0, N.STAT_ACTOR_LOSS] == out["loss"][0] and np.isfinite(st[0, 0, N.STAT_ACTOR_GNORM])
    e.close()


def _learner(p, Ts):
    c = dict(ro.case("o4_a2"), seed=9900 + 37 * p, Ts=list(Ts))
    c["n_learn"] = len(Ts)
    return c, ro.inputs(c)


def _ragged(N, P, lens_by_call, watch, cap=96):
    """P learners with their own parameters and episodes; call k trains learner p on lens_by_call[k][p] steps (0: it sits out).
    Watched learners against oracles on exactly their inputs; every learner that sits a call out bit-equal to before."""
    c0 = ro.case("o4_a2")
    e = _engine(N, c0, P=P, cap=cap)
    data, orc = {}, {}
    for p in range(P):
        Ts = [ln[p] for ln in lens_by_call if ln[p] > 0]
        c, inp = _learner(p, Ts)
        e.set_params(0, flat_params(inp["params"], NAMES), learner=p)
        data[p] = iter(inp["calls"])
        if p in watch:
            orc[p] = ro.Reinforce(inp["params"], c0["lr"])
    steps = [0] * P
    for k, lens in enumerate(lens_by_call):
        calls = {p: next(data[p]) for p in range(P) if lens[p] > 0}
        who = sorted(calls)
        e.add_batch(np.concatenate([_recs(calls[p]) for p in who]), learners=np.repeat(np.array(who, np.int32), [lens[p] for p in who]))
        idle = {p: _state(e, p) for p in range(P) if lens[p] == 0 and (p in watch or p % 61 == 0)}
        # (NULL n_steps = the cursor sizes, which are the lengths here; the explicit form on the other calls)
        out = e.reinforce_learn(gamma=c0["gamma"], lr=c0["lr"], n_steps=lens if k % 2 == 0 else None, want_loss=True, want_returns=True)
        for p in range(P):
            steps[p] += lens[p] > 0
        for p, before in idle.items():
            assert _same_state(before, _state(e, p)), "learner %d sat call %d out and changed" % (p, k)
            assert np.isnan(out["loss"][p]) and np.isnan(out["returns"][p]).all()
        for p in watch:
            if lens[p] > 0:
                cl = calls[p]
                r = orc[p].learn_with(cl["obs"], cl["act"], cl["rew"], cl["done"], c0["gamma"])
                _check_call(out, p, r, FIGURES["o4_a2"], None, "P %d learner %d call %d (T %d)" % (P, p, k, lens[p]))
                assert e.cursor(p) == (0, 0)
            assert e.opt_step(0, p) == steps[p]
    for p in watch:
        if steps[p]:
            _assert_net(e.get_params(0, 0, p), orc[p].p, NAMES, 5e-4, 5e-6, c0["lr"], steps[p], "P %d learner %d" % (P, p))
            _assert_m(e.get_params(0, 2, p), orc[p].m, NAMES, "P %d learner %d" % (P, p))
    return e


@pytest.mark.parametrize("T", [32, 37])
def test_two_chunks_per_workgroup(N, T, monkeypatch):
    """FRL_RC=16, FRL_CPS=2, one learner, two episodes of T steps: a workgroup walks two row chunks and its second chunk ADDS to the
    slab its first one stored.  32 steps: one workgroup, two full chunks; 37: a second workgroup with the ragged 5-row chunk."""
    monkeypatch.setenv("FRL_RC", "16")
    monkeypatch.setenv("FRL_CPS", "2")
    e = _ragged(N, 1, [[T], [T]], watch=[0], cap=64)
    # rc from the engine; its cps (no getter in the C ABI) is pinned for exactly this engine by the plan on the CPU:
    # tests/test_engine_plan.py::test_rowchunk_addresses_stay_inside_the_plans_buffers ("rc 16 cps 2 S 2")
    assert e.lds_bytes()[1] == 16
    e.close()


def test_ragged_population_p5(N):
    """Lengths [33, 0, 2, capacity, 17] in one call (capacity 96: 32-row chunks, three of them for learner 3), then [0, 40, 0, 16, 0].
    Learner 1 holds its 40 steps through the first call untouched — parameters, m, v, step and cursor."""
    c0 = ro.case("o4_a2")
    lens1, lens2 = [33, 0, 2, 96, 17], [0, 40, 0, 16, 0]
    orc, inps = {}, {}
    e = _engine(N, c0, P=5, cap=96)
    assert e.lds_bytes()[1] == 32
    for p in range(5):
        Ts = [t for t in (lens1[p], lens2[p]) if t > 0]
        inps[p] = _learner(p, Ts)[1]
        e.set_params(0, flat_params(inps[p]["params"], NAMES), learner=p)
        orc[p] = ro.Reinforce(inps[p]["params"], c0["lr"])
    it = {p: iter(inps[p]["calls"]) for p in range(5)}
    first = {p: next(it[p]) for p in range(5)}                 # learner 1's 40 steps are stored before the first call
    e.add_batch(np.concatenate([_recs(first[p]) for p in range(5)]),
                learners=np.repeat(np.arange(5, dtype=np.int32), [len(first[p]["rew"]) for p in range(5)]))
    before = _state(e, 1)
    assert before[4] == (40, 40)
    out = e.reinforce_learn(gamma=c0["gamma"], lr=c0["lr"], n_steps=lens1, want_loss=True, want_returns=True)
    assert _same_state(before, _state(e, 1)), "learner 1 sat the call out and changed"
    assert np.isnan(out["loss"][1]) and np.isnan(out["returns"][1]).all()
    for p in (0, 2, 3, 4):
        cl = first[p]
        r = orc[p].learn_with(cl["obs"], cl["act"], cl["rew"], cl["done"], c0["gamma"])
        _check_call(out, p, r, FIGURES["o4_a2"], None, "learner %d call 0 (T %d)" % (p, lens1[p]))
        assert e.cursor(p) == (0, 0) and e.opt_step(0, p) == 1
    second = {1: first[1], 3: next(it[3])}
    e.add_batch(_recs(second[3]), learners=np.full(16, 3, np.int32))
    idle = {p: _state(e, p) for p in (0, 2, 4)}
    out = e.reinforce_learn(gamma=c0["gamma"], lr=c0["lr"], want_loss=True, want_returns=True)      # NULL n_steps: the cursor sizes
    for p in (0, 2, 4):
        assert _same_state(idle[p], _state(e, p)), "learner %d sat the second call out and changed" % p
    for p in (1, 3):
        cl = second[p]
        r = orc[p].learn_with(cl["obs"], cl["act"], cl["rew"], cl["done"], c0["gamma"])
        _check_call(out, p, r, FIGURES["o4_a2"], None, "learner %d call 1 (T %d)" % (p, lens2[p]))
        assert e.cursor(p) == (0, 0)
    assert [e.opt_step(0, p) for p in range(5)] == [1, 1, 1, 2, 1]
    for p in range(5):
        _assert_net(e.get_params(0, 0, p), orc[p].p, NAMES, 5e-4, 5e-6, c0["lr"], 2, "learner %d" % p)
        _assert_m(e.get_params(0, 2, p), orc[p].m, NAMES, "learner %d" % p)
    e.close()


def test_ragged_population_p512(N):
    """512 learners, lengths cycling through 0, 2, 16, 17, 33, 96 and shifted by three in the second call: 64-row chunks (the
    population fills the chip), two workgroups per learner, most of them with nothing or half a chunk to do."""
    cyc = [0, 2, 16, 17, 33, 96]
    lens = [[cyc[(p + s) % 6] for p in range(512)] for s in (0, 3)]
    e = _ragged(N, 512, lens, watch=(0, 1, 255, 256, 511))
    assert e.lds_bytes()[1] == 64
    e.close()


def test_determinism(N):
    """The same call twice from the same state: bit-identical parameters, moments and normalised returns."""
    got = []
    for _ in range(2):
        e = _ragged(N, 3, [[96, 33, 17], [50, 0, 64]], watch=())
        cl = _learner(7, [77])[1]["calls"][0]
        e.add_batch(_recs(cl), learners=np.full(77, 1, np.int32))
        out = e.reinforce_learn(gamma=0.99, lr=1e-3, want_loss=True, want_returns=True)
        got.append([e.get_params(0, k, p) for p in range(3) for k in (0, 2, 3)] + [out["returns"][1, :77], out["loss"][1:2]])
        e.close()
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)


LONG_WINDOW = (100, 1e-5, 1e-4)      # calls in the tight window, tolerance there, tolerance over the whole curve — both of s


def test_long_curve(N):
    """150 calls at O = 4, A = 2, T from 8..200 against the reference's curve, by the window / envelope rule of
    tests/test_gpu_longrun.py with the error stated against s: one net and no bootstrapped target, so — like DQN and PPO's critic
    there — the curve stays at rounding level: 1e-5 of s over the first 100 calls, 1e-4 of s over all 150.  Measured on an MI355X, max |d| / s
    over calls 0-49 / 50-99 / 100-149: 2.6e-7 / 1.6e-7 / 2.6e-7 (the float32 oracle against the same curve: 5.6e-7)."""
    g = np.load(os.path.join(GOLDEN, "long_reinforce.npz"))
    c = ro.case("long")
    inp = ro.inputs(c)
    e = _engine(N, c)
    e.set_params(0, flat_params(inp["params"], NAMES))
    o = ro.Reinforce(inp["params"], c["lr"])
    err = []
    for k, call in enumerate(inp["calls"]):
        e.add_batch(_recs(call))
        out = e.reinforce_learn(gamma=c["gamma"], lr=c["lr"], want_loss=True)
        r = o.learn_with(call["obs"], call["act"], call["rew"], call["done"], c["gamma"])
        err.append(abs(float(out["loss"][0]) - float(g["loss"][k])) / r["s"])
    err = np.array(err)
    n_tight, tol_tight, tol_all = LONG_WINDOW
    print("long curve: max |d| / s over calls 0-49 %.3g, 50-99 %.3g, 100-149 %.3g" % (err[:50].max(), err[50:100].max(), err[100:].max()))
    assert err[:n_tight].max() <= tol_tight and err.max() <= tol_all
    e.close()


def _code(N, fn):
    try:
        fn()
    except N.FrlError as ex:
        m = re.match(r"freerl_hip error (\d+): (.+)", str(ex))
        assert m and len(m.group(2)) > 10, str(ex)
        return int(m.group(1))
    return 0


def test_rejections_and_cursor(N):
    from freerl_amd.engine import Engine
    INVALID, STATE = 1, 4
    assert _code(N, lambda: Engine(N.ALGO_REINFORCE, 4, 65, 64, discrete=True)) == INVALID
    assert _code(N, lambda: Engine(N.ALGO_REINFORCE, 4, 2, 64, discrete=True, hidden=512)) == INVALID
    assert _code(N, lambda: Engine(N.ALGO_REINFORCE, [4, 4], [2, 2], 64, discrete=True)) == INVALID
    e = Engine(N.ALGO_REINFORCE, 4, 64, 64, n_learners=2, discrete=True)      # 64 actions: the most it takes
    assert e.lds_bytes()[0] <= 80 * 1024
    e.add_batch(np.zeros((40, e.width), np.float32), learners=np.zeros(40, np.int32))
    e.add_batch(np.zeros((1, e.width), np.float32), learners=np.ones(1, np.int32))
    before = [_state(e, p) for p in range(2)]
    L = N.lib()
    kw = dict(gamma=0.99, lr=1e-3)
    assert _code(N, lambda: e.reinforce_learn(n_steps=[40, 1], **kw)) == INVALID           # one stored step
    assert _code(N, lambda: e.reinforce_learn(**kw)) == INVALID                            # ... through the cursor sizes too
    assert _code(N, lambda: e.reinforce_learn(n_steps=[65, 0], **kw)) == INVALID           # more than capacity
    assert _code(N, lambda: e.reinforce_learn(n_steps=[-1, 0], **kw)) == INVALID
    assert _code(N, lambda: e.reinforce_learn(n_steps=[41, 0], **kw)) == STATE             # more than the ring holds
    e.set_cursor(0, 7, 40)
    assert _code(N, lambda: e.reinforce_learn(n_steps=[40, 0], **kw)) == STATE             # a ring that was not filled from empty
    e.set_cursor(0, 40, 40)
    assert _code(N, lambda: e.learn(8, gamma=0.99, tau=0.01)) == STATE
    assert L.frl_ppo_learn(e._h, C.byref(N.PpoArgs())) == STATE
    assert L.frl_rollout(e._h, None, None, None) == STATE
    assert _code(N, lambda: e.act_explore(N.ACT_ARGMAX, np.zeros((2, 1, 4), np.float32), kind=1)) == STATE
    assert [_same_state(b, _state(e, p)) for p, b in enumerate(before)] == [True, True], "a refused call changed the engine"
    # the three act modes it serves
    obs = np.zeros((2, 3, 4), np.float32)
    assert e.act(0, N.ACT_RAW, obs, out_dim=64).shape == (2, 3, 64)
    assert e.act(0, N.ACT_ARGMAX, obs).shape == (2, 3, 1)
    assert e.act(0, N.ACT_CAT_SAMPLE, obs, eps=np.ones((2, 3, 64), np.float32)).shape == (2, 3, 1)
    # after a learn the cursor of the learner that took part is 0, the other's stays
    e.reinforce_learn(n_steps=[40, 0], **kw)
    assert e.cursor(0) == (0, 0) and e.cursor(1) == (1, 1)
    assert e.opt_step(0, 0) == 1 and e.opt_step(0, 1) == 0
    e.close()
    d = Engine(N.ALGO_DQN, 4, 2, 64, discrete=True)
    d.add_batch(np.zeros((8, d.width), np.float32))
    assert _code(N, lambda: d.reinforce_learn(**kw)) == STATE
    d.close()


def test_class(N, tmp_path):
    """REINFORCE(dim_info, is_continue, lr, device): the reference's state_dict keys and shapes, select_action = torch's
    Categorical(probs).sample() under the same generator state, stage / commit / overwrite, all(), save / load, the four errors."""
    from freerl_amd.REINFORCE import REINFORCE
    O, A = 4, 2
    torch.manual_seed(3)
    pol = REINFORCE([O, A], False, 1e-3, torch.device("cpu"), max_steps=6)
    sd = pol.agent.policy_net.state_dict()
    assert list(sd.keys()) == ["l1.weight", "l1.bias", "l2.weight", "l2.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(128, O), (128,), (A, 128), (A,)]
    torch.manual_seed(3)                                   # torch's default nn.Linear init, l1 then l2
    l1, l2 = torch.nn.Linear(O, 128), torch.nn.Linear(128, A)
    assert torch.equal(sd["l1.weight"], l1.weight.detach()) and torch.equal(sd["l2.bias"], l2.bias.detach())
    rng = np.random.default_rng(5)
    for i in range(32):
        obs = rng.standard_normal(O).astype(np.float32)
        torch.manual_seed(100 + i)
        a = pol.select_action(obs)
        assert isinstance(a, np.int64)
        torch.manual_seed(100 + i)
        dist = torch.distributions.Categorical(pol.agent.policy_net(obs.reshape(1, -1)))
        want = dist.sample()
        assert int(want.item()) == int(a)
        assert abs(float(dist.log_prob(want).item()) - float(pol._staged[2][0])) < 1e-5
    # stage / commit / overwrite: nothing is stored until add(); a staged step that no add() follows is replaced
    assert pol.all() == ([], [], []) and pol._e.cursor() == (0, 0)
    o1, o2 = rng.standard_normal(O).astype(np.float32), rng.standard_normal(O).astype(np.float32)
    pol.select_action(o1)
    a2 = pol.evaluate_action(o2)
    lp2 = float(pol._staged[2][0])
    pol.add(1.5, False)
    rewards, dones, log_probs = pol.all()
    assert rewards == [1.5] and dones == [False] and len(log_probs) == 1 and float(log_probs[0].item()) == lp2
    row = pol._e.read_rows(0, 0, 1)[0]
    lay = pol._e.layout
    np.testing.assert_array_equal(row[lay.obs_off[0]:lay.obs_off[0] + O], o2)
    assert row[lay.act_off[0]] == a2 and row[lay.rew_off] == 1.5 and row[lay.done_off] == 0
    with pytest.raises(RuntimeError):
        pol.add(1.0, False)                                # nothing staged
    with pytest.raises(ValueError):
        pol.learn(0.99)                                    # one stored step: NaN in the reference
    for i in range(5):
        pol.select_action(rng.standard_normal(O))
        pol.add(1.0, i == 4)
    pol.select_action(o1)
    with pytest.raises(RuntimeError, match="max_steps"):
        pol.add(1.0, False)                                # a seventh step in a ring of six
    pol.track_loss = True
    before = pol.agent.policy_net.state_dict()
    pol.learn(0.99)
    assert np.isfinite(pol.last_loss) and pol.all() == ([], [], []) and pol._e.cursor() == (0, 0)
    assert not torch.equal(before["l2.bias"], pol.agent.policy_net.state_dict()["l2.bias"])
    assert pol.agent.policy_net_optimizer.state_dict()["step"] == 1
    with pytest.raises(ValueError):
        pol.learn(0.99)                                    # no stored step
    with pytest.raises(ValueError):
        REINFORCE([O, A], True, 1e-3, torch.device("cpu"))
    pol.save(str(tmp_path))
    assert os.listdir(str(tmp_path)) == ["REINFORCE.pt"]
    back = REINFORCE.load([O, A], False, str(tmp_path))
    for k, v in pol.agent.policy_net.state_dict().items():
        assert torch.equal(v, back.agent.policy_net.state_dict()[k])


def test_training_loop_follows_the_reference(N, tmp_path):
    """freerl_amd.train reinforce against REINFORCE.py's own `__main__` loop (tests/golden/loop_reinforce_cartpole.npz,
    make_reinforce_golden.py): same flags, in-repo CartPole, same seeds -> the actions identical step by step (Categorical
    draws, one learn() per episode), returns, the same result files, the checkpoint's digest."""
    from freerl_amd import envs as E
    from freerl_amd import train
    from tests.golden.make_loop_golden import Recorder
    fx = np.load(os.path.join(GOLDEN, "loop_reinforce_cartpole.npz"))
    argv = str(fx["flags"]).replace("--device cpu", "--device cuda").split() + ["--results_root", str(tmp_path / "results")]
    log = dict(actions=[], rewards=[])
    env = Recorder(E.make("CartPole-v1", prefer_gymnasium=False), log)
    out = train.run("reinforce", argv, env=env, log=lambda *a: None)
    acts, rews = np.stack(log["actions"]), np.stack(log["rewards"])
    assert acts.shape == fx["actions"].shape, (acts.shape, fx["actions"].shape)
    np.testing.assert_array_equal(acts, fx["actions"])
    np.testing.assert_allclose(rews, fx["rewards"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(out["returns"], fx["returns"], rtol=1e-3, atol=1e-3)
    assert len(out["returns"]) == 12
    files = sorted(os.listdir(out["model_dir"]))
    assert str(fx["npy_name"]) in files and str(fx["ckpt_name"]) in files, files
    assert os.path.basename(out["model_dir"]).startswith("REINFORCE_")
    sd = torch.load(os.path.join(out["model_dir"], str(fx["ckpt_name"])))
    synth.check_digest("ckpt", {k: v.numpy() for k, v in sd.items()}, fx, 5e-3, 5e-4, "loop_reinforce_cartpole")
