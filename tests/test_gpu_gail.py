"""GPU: GAIL's discriminator (GAIL_file/GAIL.py) on kernels_gail.hip, against the reference's outputs (tests/golden/gail.npz) and
the NumPy float64 restatement (tests/gail_oracle.py).

Tolerances are tests/test_gpu_envelope_ddpg.py's, unchanged: losses and the other returned means rtol 1e-4 / atol 1e-6; parameters
>= 99 % of a net's elements within (5e-4, 5e-6) and none further than 2 lr calls; Adam's first moment within 2e-3 of its largest on
99 % of a matrix, 5e-2 everywhere, 2e-2 for bias vectors; the gradient norm rtol 1e-3.  The 1 % allowance is for units within
rounding of the LeakyReLU kink, whose slope may differ between two fp32 implementations; tests/test_gail_oracle.py shows on the CPU
that float32 against float64 needs none of it on the golden inputs, second-order gradient included."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import gail_oracle as go
from tests.hip_helpers import flat_params, unflat_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = go.NAMES


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "gail.npz")))


def _engine(N, c, in_dim=None, P=1, batch_max=None, seed=0, cap=None):
    from freerl_amd.engine import Engine
    d = c["s_dim"] + c["a_dim"] if in_dim is None else in_dim
    act = N.ACT_LEAKY_RELU if c["activation"] == "LeakyReLU" else N.ACT_RELU
    return Engine(N.ALGO_GAIL, d - 1, 1, cap or c["n_table"], n_learners=P, hidden=c["hidden"], hidden_act=act,
                  batch_max=batch_max or max(c["n_expert"], c["n_policy"]), seed=seed)


def _records(e, expert):
    rec = np.zeros((len(expert), e.width), np.float32)
    assert e.layout.obs_off[0] == 0 and e.layout.act_off[0] == e.layout.obs_dim[0]
    rec[:, :expert.shape[1]] = expert
    return rec


def _learn(e, c, idx, rows, **kw):
    b = go.betas(c["gp_coef"])
    return e.gail_learn(rows, gp=c["gp_coef"] > 0, lr=c["d_lr"], beta1=b[0], beta2=b[1], idx=idx, **kw)["out"]


def _assert_net(got_flat, want, rtol, atol, lr, calls, label):
    got = unflat_params(got_flat, want, NAMES)
    for k in want:
        d = np.abs(got[k] - want[k])
        assert np.all(np.isfinite(got[k])), "%s/%s not finite" % (label, k)
        bad = d > atol + rtol * np.abs(want[k])
        assert bad.mean() <= 0.01, "%s/%s: %d of %d elements outside (max |diff| %.3g)" % (label, k, bad.sum(), bad.size, d.max())
        assert d.max() <= 2 * lr * calls, "%s/%s: max |diff| %.3g" % (label, k, d.max())


def _assert_m(got_flat, want, label):
    got = unflat_params(got_flat, want, NAMES)
    for k in want:
        scale = float(np.abs(want[k]).max())
        d = np.abs(got[k] - want[k]).reshape(-1)
        if d.size < 2048:
            assert d.max() <= 2e-2 * scale, "adam m %s/%s: %.3g of max |m| %.3g" % (label, k, d.max(), scale)
            continue
        assert np.quantile(d, 0.99) <= 2e-3 * scale, "adam m %s/%s: 99th percentile" % (label, k)
        assert d.max() <= 5e-2 * scale, "adam m %s/%s: max %.3g of %.3g" % (label, k, d.max(), scale)


def _check_state(e, o, c, calls, label, p=0):
    _assert_net(e.get_params(0, 0, p), o.p, 5e-4, 5e-6, c["d_lr"], calls, label)
    _assert_m(e.get_params(0, 2, p), o.opt.m, label)
    assert e.opt_step(0, learner=p) == calls == o.opt.t
    assert e.pad_max(0, 0, p) == 0.0 and e.pad_max(0, 2, p) == 0.0           # the padding slots never move


def _assert_out(got, want4, pen, norm, msg):
    np.testing.assert_allclose(got[:4], want4, rtol=1e-4, atol=1e-6, err_msg="returned 4-tuple, " + msg)
    np.testing.assert_allclose(got[4], pen, rtol=1e-4, atol=1e-6, err_msg="penalty mean, " + msg)
    np.testing.assert_allclose(got[5], norm, rtol=1e-3, err_msg="gradient norm, " + msg)


def _run_against_oracle(N, c, inp, calls, label, in_dim=None, batch_max=None):
    e = _engine(N, c, in_dim=in_dim, batch_max=batch_max)
    e.set_params(0, flat_params(inp["net"], NAMES))
    e.add_batch(_records(e, inp["expert"]))
    o = go.make(c, inp)
    outs = []
    for k in range(calls):
        got = _learn(e, c, inp["idx"][k][None], inp["policy"][k][None])[0]
        want = o.trian_D(inp["expert"][inp["idx"][k]], inp["policy"][k])
        print("%s call %d: got %s | oracle %s penalty %.8g norm %.8g" % (label, k, got, np.array(want), o.penalty, o.norm))
        _assert_out(got, want, o.penalty, o.norm, "%s call %d vs oracle" % (label, k))
        outs.append(got)
    _check_state(e, o, c, calls, label)
    return e, o, np.array(outs)


@pytest.mark.parametrize("name", list(go.CASES))
def test_golden_and_oracle(N, fx, name):
    """Both modes at O 3, A 1, H 32, E 37, N 29, three calls: every call's four returned values against the reference and the
    oracle, the penalty mean and the gradient norm against the oracle; at the end the net, Adam's m and the step count against the
    oracle and compute_reward on the probe batch against the reference."""
    c = go.case(name)
    inp = go.inputs(c)
    e, o, outs = _run_against_oracle(N, c, inp, c["n_learn"], name)
    np.testing.assert_allclose(outs[:, :4], fx[name + "/tuples"], rtol=1e-4, atol=1e-6, err_msg="vs reference")
    if name == "bce":
        assert np.all(outs[:, 3:5] == 0.0)
    assert e.opt_step(0) == int(fx[name + "/step"])
    r = e.gail_reward(inp["probe"][None], gp=c["gp_coef"] > 0)[0]
    assert r.dtype == np.float32 and r.shape == (c["n_probe"],)
    np.testing.assert_allclose(r, fx[name + "/reward"], rtol=1e-4, err_msg="compute_reward vs reference")
    logits = e.act(0, N.ACT_RAW, inp["probe"][None], out_dim=1)[0, :, 0]          # frl_act: the logits
    np.testing.assert_allclose(logits, o.forward(inp["probe"])[0], rtol=1e-4, atol=1e-6)
    e.close()


# (E, N, O + A, H): a single row of each kind; the kinds meet on a chunk boundary; a chunk holds both kinds and the last chunk is
# partial; the penalty on a sliver of one chunk; the reverse split; exactly one input column tile; two tiles (the unit backward's
# dX crosses a tile edge); hidden 64: the fused narrow-head path of device/net.hpp; the script's own shape
RAGGED_CASES = [(1, 1, 4, 32), (16, 16, 4, 32), (37, 29, 4, 32), (5, 300, 4, 32), (300, 5, 4, 32), (37, 29, 16, 32), (37, 29, 17, 32),
                (37, 29, 4, 64), (2048, 2048, 4, 128)]


@pytest.mark.parametrize("gp_coef", [0.0, 10.0])
@pytest.mark.parametrize("E,NP,IN,H", RAGGED_CASES)
def test_ragged_shapes(N, E, NP, IN, H, gp_coef):
    calls = 1 if E == 2048 else 3                   # the script's own shape, once
    c = dict(go.COMMON, gp_coef=gp_coef, seed=12000 + 7 * E + 3 * NP + IN + H, hidden=H, n_expert=E, n_policy=NP, n_table=max(60, E // 4))
    inp = go.inputs(c, n_learn=calls, in_dim=IN)
    e, _, _ = _run_against_oracle(N, c, inp, calls, "E%d N%d IN%d H%d gp%g" % (E, NP, IN, H, gp_coef), in_dim=IN)
    e.close()


@pytest.mark.parametrize("gp_coef", [0.0, 10.0])
@pytest.mark.parametrize("E,NP", [(16, 16), (20, 17)])
def test_two_chunks_per_workgroup(N, E, NP, gp_coef, monkeypatch):
    """FRL_RC=16, FRL_CPS=2, one learner: a workgroup walks two row chunks and its second chunk ADDS to the slab its first one stored
    (and, with the penalty, to what the chunk's own backward stored).  16 + 16 = 32 rows: one workgroup, two full chunks, one of each
    kind; 20 + 17 = 37 rows: the kinds meet inside the second chunk and a second workgroup takes the ragged 5-row chunk."""
    monkeypatch.setenv("FRL_RC", "16")
    monkeypatch.setenv("FRL_CPS", "2")
    c = dict(go.COMMON, gp_coef=gp_coef, seed=12500 + 7 * E + 3 * NP, hidden=32, n_expert=E, n_policy=NP, n_table=60)
    inp = go.inputs(c, n_learn=2, in_dim=4)
    e, _, _ = _run_against_oracle(N, c, inp, 2, "cps2 E%d N%d gp%g" % (E, NP, gp_coef), in_dim=4, batch_max=32)
    # rc from the engine; its cps (no getter in the C ABI) is pinned for exactly this engine by the plan on the CPU:
    # tests/test_engine_plan.py::test_rowchunk_addresses_stay_inside_the_plans_buffers ("rc 16 cps 2 S 2")
    assert e.lds_bytes()[1] == 16
    e.close()


@pytest.mark.parametrize("gp_coef", [0.0, 10.0])
def test_relu_hidden_activation(N, gp_coef):
    c = dict(go.COMMON, gp_coef=gp_coef, seed=12500, activation="ReLU")
    inp = go.inputs(c)
    e, o, _ = _run_against_oracle(N, c, inp, 3, "ReLU gp%g" % gp_coef)
    np.testing.assert_allclose(e.gail_reward(inp["probe"][None], gp=gp_coef > 0)[0], o.compute_reward(inp["probe"]), rtol=1e-4)
    e.close()


@pytest.mark.parametrize("bias", [20.0, -20.0, 90.0, -90.0])
def test_saturation_without_gp(N, bias):
    """The head bias puts every logit near +-20 / +-90, where fp32 sigmoid is exactly 1 (from 17) or p (1 - p) falls below 1e-12
    (and p is exactly 0 below -89): the loss is finite and equals the oracle's clamped value (the oracle's sigmoid rounded through
    float32, which is what decides where torch's clamps act); the parameters stay finite and match the oracle."""
    c = dict(go.COMMON, gp_coef=0.0, seed=12600, n_learn=2)
    inp = go.inputs(c)
    inp["net"][NAMES[2] + ".bias"][:] = bias
    e = _engine(N, c)
    e.set_params(0, flat_params(inp["net"], NAMES))
    e.add_batch(_records(e, inp["expert"]))
    o = go.make(c, inp, p32=True)
    for k in range(2):
        got = _learn(e, c, inp["idx"][k][None], inp["policy"][k][None])[0]
        want = o.trian_D(inp["expert"][inp["idx"][k]], inp["policy"][k])
        print("bias %g call %d: got %s | oracle %s norm %.6g" % (bias, k, got, np.array(want), o.norm))
        assert np.all(np.isfinite(got))
        np.testing.assert_allclose(got[:4], want, rtol=1e-4, atol=1e-6)
        if abs(bias) == 90.0:
            assert abs(got[0] - 100.0) < 1e-3           # one side's log is clamped at -100 on every row, the other side's loss is 0
    _check_state(e, o, c, 2, "bias %g" % bias)
    e.close()


POP = dict(hidden=32, n_expert=16, n_policy=16, n_table=40)


def pop_inputs(p, gp_coef):
    c = dict(go.COMMON, **POP, gp_coef=gp_coef, seed=13000 + 10 * p)
    return c, go.inputs(c, n_learn=2)


@pytest.mark.parametrize("P", [1, 40, 512])
def test_population(N, P):
    """Every learner has its own net, ring, rows and indices; learner 0, the two middle ones and the last are held to oracles of
    their own for two calls (the default mode, gp)."""
    c = pop_inputs(0, 10.0)[0]
    e = _engine(N, c, P=P)
    inps = [pop_inputs(p, 10.0)[1] for p in range(P)]
    for p in range(P):
        e.set_params(0, flat_params(inps[p]["net"], NAMES), learner=p)
    e.add_batch(np.concatenate([_records(e, i["expert"]) for i in inps]), learners=np.repeat(np.arange(P), c["n_table"]))
    check = sorted({0, max(P // 2 - 1, 0), P // 2, P - 1})
    orc = {p: go.make(c, inps[p]) for p in check}
    for k in range(2):
        got = _learn(e, c, np.stack([i["idx"][k] for i in inps]), np.stack([i["policy"][k] for i in inps]))
        assert got.shape == (P, 6) and np.all(np.isfinite(got))
        for p in check:
            want = orc[p].trian_D(inps[p]["expert"][inps[p]["idx"][k]], inps[p]["policy"][k])
            _assert_out(got[p], want, orc[p].penalty, orc[p].norm, "learner %d call %d" % (p, k))
    for p in check:
        _check_state(e, orc[p], c, 2, "P%d learner %d" % (P, p), p)
    e.close()


def test_device_draw(N):
    """idx = NULL: rows in range through idx_out, drawn with replacement (repeats appear and are allowed), different between
    learners and between calls; a replay with idx = idx_out on a fresh engine gives bit-identical outputs."""
    c = dict(go.COMMON, gp_coef=10.0, seed=13500, n_expert=64, n_policy=16, n_table=40, hidden=32)
    inp = go.inputs(c, n_learn=2)

    def fresh():
        e = _engine(N, c, P=2, seed=5)
        for p in range(2):
            e.set_params(0, flat_params(inp["net"], NAMES), learner=p)
        e.add_batch(np.concatenate([_records(e, inp["expert"])] * 2), learners=np.repeat(np.arange(2), c["n_table"]))
        return e
    b = go.betas(c["gp_coef"])
    kw = dict(gp=True, lr=c["d_lr"], beta1=b[0], beta2=b[1])
    rows = [np.stack([inp["policy"][k]] * 2) for k in range(2)]
    e = fresh()
    o1 = e.gail_learn(rows[0], n_expert=64, want_idx=True, **kw)
    o2 = e.gail_learn(rows[1], n_expert=64, want_idx=True, **kw)
    for o in (o1, o2):
        assert o["idx"].shape == (2, 64) and o["idx"].min() >= 0 and o["idx"].max() < c["n_table"] and np.all(np.isfinite(o["out"]))
        assert not np.array_equal(o["idx"][0], o["idx"][1])                 # learners draw their own
    assert not np.array_equal(o1["idx"], o2["idx"])                          # ... and so does every call
    assert any(len(set(r.tolist())) < 64 for o in (o1, o2) for r in o["idx"])      # 64 draws from 40 rows: repeats
    e.close()
    e2 = fresh()
    b1 = e2.gail_learn(rows[0], idx=o1["idx"], **kw)
    b2 = e2.gail_learn(rows[1], idx=o2["idx"], **kw)
    assert np.array_equal(b1["out"], o1["out"]) and np.array_equal(b2["out"], o2["out"])      # bit for bit
    e2.close()


def test_class(N, fx, tmp_path):
    """freerl_amd.GAIL.GAIL through the golden's class case: seeded init, load_expert, next_expert_indices + trian_D_indices, then
    trian_D with arrays; compute_reward; state_dict keys and shapes; a save / load round trip; the refusals."""
    from freerl_amd.GAIL import GAIL, ExpertDataset
    c = go.case("class")
    seed = c["seed"]
    inp = go.inputs(c)
    cfg = go.config(c)
    ds = ExpertDataset(go.raw_expert(c, seed))
    gail = GAIL(cfg, ppo="not called", max_rows=64)
    assert gail.ppo == "not called"
    assert gail.D_optimizer.defaults["betas"] == (0.5, 0.9) and gail.D_optimizer.param_groups[0]["lr"] == c["d_lr"]
    H, IN = c["hidden"], c["s_dim"] + c["a_dim"]
    sd = gail.D_model.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {"backbone.0.weight": (H, IN), "backbone.0.bias": (H,), "backbone.1.weight": (H, H),
                                                          "backbone.1.bias": (H,), "backbone.2.weight": (1, H), "backbone.2.bias": (1,)}
    for k, v in sd.items():                                                  # the reference's seeded default init
        np.testing.assert_array_equal(v.numpy(), fx["class/init/%s/full" % k].reshape(v.shape))
    gail.load_expert(ds)
    for k, v in gail.D_model.state_dict().items():                           # the net survives the ring's re-creation
        assert torch.equal(v, sd[k])
    torch.manual_seed(seed + 1)
    s_dim = c["s_dim"]
    for k in range(c["n_learn"]):
        idx = gail.next_expert_indices(c["n_expert"])
        np.testing.assert_array_equal(idx, fx["class/idx"][k])
        pol = inp["policy"][k]
        if k < c["n_learn"] - 1:
            got = gail.trian_D_indices(idx, pol[:, :s_dim], pol[:, s_dim:])
        else:                                                                # the array form: the expert rows are uploaded as given
            es, ea = ds.states[idx].astype(np.float32), ds.actions[idx].astype(np.float32)
            got = gail.trian_D(torch.as_tensor(es), torch.as_tensor(ea), torch.as_tensor(pol[:, :s_dim]), pol[:, s_dim:])
        assert len(got) == 4 and all(isinstance(v, float) for v in got)
        np.testing.assert_allclose(got, fx["class/tuples"][k], rtol=1e-4, atol=1e-6, err_msg="trian_D call %d" % k)
    assert gail.D_optimizer.state_dict()["step"] == c["n_learn"] == int(fx["class/step"])
    r = gail.compute_reward(inp["probe"][:, :s_dim], torch.as_tensor(inp["probe"][:, s_dim:]))
    assert isinstance(r, torch.Tensor) and r.dtype == torch.float32 and r.shape == (c["n_probe"],)
    np.testing.assert_allclose(r.numpy(), fx["class/reward"], rtol=1e-4)
    logits = gail.D_model(torch.as_tensor(inp["probe"]))
    assert logits.shape == (c["n_probe"], 1)                                 # gp: the model returns logits
    np.testing.assert_allclose(2 * -np.log(np.maximum(1 - 1 / (1 + np.exp(-logits.numpy()[:, 0].astype(np.float64))), 1e-4)), r.numpy(), rtol=1e-4)
    # checkpoint round trip
    path = os.path.join(str(tmp_path), "D.pt")
    want = gail.D_model.state_dict()
    torch.save(want, path)
    back = GAIL(cfg, max_rows=64)
    back.D_model.load_state_dict(torch.load(path))
    for k, v in back.D_model.state_dict().items():
        assert torch.equal(v, want[k]), k
    np.testing.assert_array_equal(back.compute_reward(inp["probe"][:, :s_dim], inp["probe"][:, s_dim:]).numpy(), r.numpy())
    # without gp the model returns probabilities, and the optimizer's betas follow
    plain = GAIL(dict(cfg, D=dict(cfg["D"], gp_coef=0.0)), max_rows=64)
    assert plain.D_optimizer.defaults["betas"] == (0.9, 0.999)
    pr = plain.D_model(torch.as_tensor(inp["probe"])).numpy()
    assert np.all((pr > 0) & (pr < 1))
    for bad in (dict(activation="Tanh"), dict(layernorm=True), dict(dropout=0.1)):
        with pytest.raises(ValueError):
            GAIL(dict(cfg, D=dict(cfg["D"], **bad)))
    with pytest.raises(NotImplementedError, match="PPO2"):
        gail.train(None, None, 1)


def test_rejections(N):
    from freerl_amd.engine import Engine
    with pytest.raises(N.FrlError, match="FRL_ACT_TANH"):
        Engine(N.ALGO_GAIL, 3, 1, 40, hidden=32, hidden_act=N.ACT_TANH, batch_max=32)
    with pytest.raises(N.FrlError, match="hidden"):
        Engine(N.ALGO_GAIL, 3, 1, 40, hidden=512, hidden_act=N.ACT_LEAKY_RELU, batch_max=32)
    with pytest.raises(N.FrlError, match="80 KB"):                      # 1000 input columns at hidden 256: no two workgroups per CU
        Engine(N.ALGO_GAIL, 1000, 1, 40, hidden=256, hidden_act=N.ACT_LEAKY_RELU, batch_max=32)
    with pytest.raises(N.FrlError, match="LEAKY"):                      # only the new engine kind takes the new activation
        Engine(N.ALGO_DDPG, 4, 3, 40, hidden_act=N.ACT_LEAKY_RELU, batch_max=32)
    big = Engine(N.ALGO_GAIL, 3, 1, 8, hidden=256, hidden_act=N.ACT_LEAKY_RELU, batch_max=32)      # hidden 256 fits two workgroups per CU
    assert big.lds_bytes()[0] <= 80 * 1024
    big.close()
    c = dict(go.COMMON, gp_coef=10.0, seed=13900, n_expert=8, n_policy=8, n_table=40)
    inp = go.inputs(c, n_learn=1)
    e = _engine(N, c, batch_max=16, cap=64)
    assert e.n_nets == 1
    e.set_params(0, flat_params(inp["net"], NAMES))
    rows, idx = inp["policy"][0][None], inp["idx"][0][None] % 20
    ok = dict(gp=1, lr=4e-4, beta1=0.5, beta2=0.9)
    with pytest.raises(N.FrlError, match="error 4.*empty"):             # FRL_ERR_STATE: nothing stored yet
        e.gail_learn(rows, idx=idx, **ok)
    e.add_batch(_records(e, inp["expert"])[:20])
    before = e.get_params(0)
    nan = float("nan")
    wide = np.zeros((1, 17, 4), np.float32)
    for kw, r, ix, msg in ((dict(n_expert=0), rows, None, "error 1.*n_expert"), (dict(n_expert=17), rows, None, "error 1.*n_expert"),
                           ({}, wide, idx, "error 1.*n_policy"), ({}, np.zeros((1, 0, 4), np.float32), idx, "error 1.*n_policy"),
                           (dict(lr=nan), rows, idx, "error 1.*NaN"), (dict(beta1=nan), rows, idx, "error 1.*NaN"),
                           (dict(beta2=nan), rows, idx, "error 1.*NaN"), (dict(gp_weight=nan), rows, idx, "error 1.*NaN"),
                           (dict(adam_eps=nan), rows, idx, "error 1.*NaN"), (dict(beta1=1.0), rows, idx, "error 1.*betas"),
                           (dict(beta2=-0.1), rows, idx, "error 1.*betas"), (dict(gp=2), rows, idx, "error 1.*gp"),
                           (dict(gp=-1), rows, idx, "error 1.*gp"), (dict(gp_weight=-1.0), rows, idx, "error 1.*gp_weight"),
                           ({}, rows, np.full((1, 8), 20), "error 4.*stored rows"), ({}, rows, np.full((1, 8), -1), "error 4.*stored rows")):
        with pytest.raises(N.FrlError, match=msg):
            e.gail_learn(r, idx=ix, **dict(ok, **kw))
    a = N.GailArgs()
    a.n_expert, a.n_policy, a.gp, a.gp_weight, a.lr, a.beta1, a.beta2, a.adam_eps = 8, 8, 1, 5.0, 4e-4, 0.5, 0.9, 1e-8
    assert e._L.frl_gail_learn(e._h, C.byref(a)) == 1 and b"policy_rows" in e._L.frl_last_error()      # FRL_ERR_INVALID: NULL rows
    with pytest.raises(N.FrlError, match="error 1"):
        e.gail_reward(np.zeros((1, 4, 4), np.float32), gp=2)
    # every other learn, rollout and explore entry point refuses the engine and names both ways in
    for call in (lambda: e.learn(8, gamma=0.99, tau=0.01, critic_lr=1e-3),
                 lambda: e.ppo_learn(8, 4, 1, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.0, actor_lr=1e-3, critic_lr=1e-3),
                 lambda: e.reinforce_learn(gamma=0.99, lr=1e-3),
                 lambda: e.envelope_learn(8, 1, gamma=0.99, tau=0.01, lr=1e-3, beta=0.5),
                 lambda: e.envelope_ddpg_learn(8, 1, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, beta=0.5),
                 lambda: e.act_explore(N.ACT_TANHHEAD, np.zeros((1, 1, 3), np.float32), kind=N.EXPLORE_GAUSS)):
        with pytest.raises(N.FrlError, match="error 4.*frl_gail_learn.*FRL_ACT_RAW"):
            call()
    ra, st = N.RolloutArgs(), N.RolloutStats()
    assert e._L.frl_rollout(e._h, None, C.byref(ra), C.byref(st)) == 4
    assert b"frl_gail_learn" in e._L.frl_last_error() and b"FRL_ACT_RAW" in e._L.frl_last_error()
    with pytest.raises(N.FrlError, match="FRL_ACT_RAW"):                # frl_act: the logits only
        e.act(0, N.ACT_TANHHEAD, np.zeros((1, 1, 4), np.float32), out_dim=1)
    assert np.array_equal(before, e.get_params(0)) and e.opt_step(0) == 0      # nothing was launched
    got = e.gail_learn(rows, idx=idx, **ok)["out"][0]
    assert np.all(np.isfinite(got)) and e.opt_step(0) == 1                      # ... and the engine still works
    e.close()
    d = Engine(N.ALGO_DDPG, 3, 1, 40, batch_max=32)
    with pytest.raises(N.FrlError, match="error 4.*frl_gail_learn"):
        d.gail_learn(rows, idx=idx, **ok)
    with pytest.raises(N.FrlError, match="error 4.*frl_gail_reward"):
        d.gail_reward(np.zeros((1, 4, 4), np.float32), gp=1)
    d.close()
