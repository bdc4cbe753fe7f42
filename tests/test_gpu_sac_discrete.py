"""GPU: discrete SAC (SAC_file/SAC_add_discrete.py) on kernels_sacd.hip, against the reference's outputs
(tests/golden/sac_discrete.npz, long_sac_discrete.npz) and the NumPy restatement (tests/sacd_oracle.py)."""
import os

import numpy as np
import pytest
import torch

from tests import sacd_oracle as so
from tests.golden import synth
from tests.hip_helpers import flat_params, records, unflat_params

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
A_NAMES, C_NAMES = ["l1", "l2", "l3"], ["l1", "l2", "l3", "l4", "l5", "l6"]


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


def _engine(N, c, P=1, cap=None, batch_max=None):
    from freerl_amd.engine import Engine
    e = Engine(N.ALGO_SAC_DISCRETE, c["obs_dim"], c["n_act"], cap or c["n_table"], n_learners=P, twin_critic=True,
               hidden=c["hidden"], batch_max=batch_max or c["batch"])
    if c["bn"]:
        e.obsnorm_enable(True)
    for p in range(P):
        e.set_alpha_state([np.log(c["alpha0"]), 0.0, 0.0, c["alpha0"]], 0, learner=p)
    return e


def _load(e, inp, p=0):
    for kind in (0, 1):
        e.set_params(0, flat_params(inp["actor"], A_NAMES), kind, learner=p)
        e.set_params(1, flat_params(inp["critic"], C_NAMES), kind, learner=p)


def _learn(N, e, c, idx, want=True):
    return e.learn(idx.shape[-1], gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"],
                   alpha_lr=c["alpha_lr"], target_entropy=float(np.float32(0.6) * -np.log(np.float32(1.0 / c["n_act"]), dtype=np.float32)),
                   idx=idx, want_stats=want)


# Parameter tolerances: the rules of test_gpu_wide_population.py (two fp32 implementations of one update differ by rounding in
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
    lr = max(c["actor_lr"], c["critic_lr"])
    _assert_net(e.get_params(0, 0, p), o.actor, A_NAMES, 5e-4, 5e-6, lr, calls, label + " actor")
    _assert_net(e.get_params(1, 0, p), o.critic, C_NAMES, 5e-4, 5e-6, lr, calls, label + " critic")
    _assert_net(e.get_params(0, 1, p), o.actor_t, A_NAMES, 5e-4, 5e-6, lr, calls, label + " actor_target")
    _assert_net(e.get_params(1, 1, p), o.critic_t, C_NAMES, 5e-4, 5e-6, lr, calls, label + " critic_target")
    _assert_m(e.get_params(0, 2, p), o.actor_opt.m, A_NAMES, label + " actor")
    _assert_m(e.get_params(1, 2, p), o.critic_opt.m, C_NAMES, label + " critic")


@pytest.mark.parametrize("name", list(so.CASES))
def test_golden_and_oracle(N, name):
    """Every case, every call: losses and alpha against the reference (1e-4) and the oracle; nets, targets, Adam m
    element-wise against the oracle."""
    fx = np.load(os.path.join(GOLDEN, "sac_discrete.npz"))
    c = so.case(name)
    inp = so.inputs(c)
    e = _engine(N, c)
    assert e.learn_path(c["batch"])[0] == 0, "discrete SAC runs the row-chunk chain"
    _load(e, inp)
    e.add_batch(records([inp["table"]]))
    o = so.make(c, inp)
    for k in range(c["n_learn"]):
        st = _learn(N, e, c, inp["idx"][k][None, None])
        cl, al, ll = o.learn_with(inp["idx"][k], c["gamma"], c["tau"])
        for key, stat, want in (("loss_critic", N.STAT_CRITIC_LOSS, cl), ("loss_actor", N.STAT_ACTOR_LOSS, al),
                                ("loss_alpha", N.STAT_ALPHA_LOSS, ll)):
            got = st[0, 0, stat]
            np.testing.assert_allclose(got, fx[name + "/" + key][k], rtol=1e-4, atol=1e-6, err_msg="%s call %d vs reference" % (key, k))
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg="%s call %d vs oracle" % (key, k))
        np.testing.assert_allclose(st[0, 0, N.STAT_ALPHA], fx[name + "/alpha"][k], rtol=1e-4, err_msg="alpha call %d" % k)
    _check_state(e, o, c, c["n_learn"], name)
    assert e.opt_step(0) == e.opt_step(1) == c["n_learn"]
    # select_action's forward: raw logits with the learner's Batch_ObsNorm statistics, and without them (the engine's actor
    # after 25 updates is the oracle's within the rounding tolerated above: logits to 1e-4; argmax where the top two differ)
    obs = inp["table"]["obs"][:40]
    xin = o.bn(obs.astype(np.float32), update=False) if c["bn"] else obs
    z_want, _ = o.pi.forward(o.actor, xin.astype(np.float32))
    np.testing.assert_allclose(e.act(0, N.ACT_RAW, obs[None], out_dim=c["n_act"])[0], z_want, rtol=1e-3, atol=1e-4)
    z_raw, _ = o.pi.forward(o.actor, obs.astype(np.float32))
    np.testing.assert_allclose(e.act(0, N.ACT_RAW, obs[None], out_dim=c["n_act"], normalize=False)[0], z_raw, rtol=1e-3, atol=1e-4)
    top2 = np.sort(z_want, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-3
    np.testing.assert_array_equal(e.act(0, N.ACT_ARGMAX, obs[None])[0, clear, 0], np.argmax(z_want, axis=1)[clear])
    # select_action (FRL_ACT_CAT_SAMPLE) with fixed Exp(1) draws q: argmax(softmax(z) / q) on the normalised obs, where the top two
    # ratios are apart by more than the logits' tolerance
    q = np.random.default_rng(11).exponential(size=(40, c["n_act"])).astype(np.float32)
    ratio = so.softmax(z_want) / q
    top2 = np.sort(ratio, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-3 * top2[:, 1]
    got = e.act(0, N.ACT_CAT_SAMPLE, obs[None], eps=q[None])[0, :, 0]
    assert clear.sum() >= 30
    np.testing.assert_array_equal(got[clear], np.argmax(ratio, axis=1)[clear])
    e.close()


@pytest.mark.parametrize("batch,n_act", [(1, 4), (37, 4), (1000, 4), (37, 64), (300, 64)])
def test_ragged_batches(N, batch, n_act):
    """Batches that leave a partial row chunk (1, 37) and many chunks per workgroup (1000 of batch_max 1024), Batch_ObsNorm on;
    64 actions = the most frl_create accepts (four head tiles, the softmax and per-row loops at their longest)."""
    c = dict(so.case("o8_a4_bn"), batch=batch, n_act=n_act, n_table=2048, n_learn=3, seed=7600 + batch + n_act)
    inp = so.inputs(c)
    e = _engine(N, c, batch_max=1024)
    _load(e, inp)
    e.add_batch(records([inp["table"]]))
    o = so.make(c, inp)
    for k in range(c["n_learn"]):
        st = _learn(N, e, c, inp["idx"][k][None, None])
        cl, al, ll = o.learn_with(inp["idx"][k], c["gamma"], c["tau"])
        np.testing.assert_allclose(st[0, 0, [N.STAT_CRITIC_LOSS, N.STAT_ACTOR_LOSS, N.STAT_ALPHA_LOSS]], [cl, al, ll],
                                   rtol=1e-4, atol=1e-6, err_msg="batch %d call %d" % (batch, k))
    _check_state(e, o, c, c["n_learn"], "batch %d" % batch)
    e.close()


@pytest.mark.parametrize("batch", [32, 37])
def test_two_chunks_per_workgroup(N, batch, monkeypatch):
    """FRL_RC=16, FRL_CPS=2, one learner: a workgroup walks two row chunks and its second chunk ADDS to the slab its first one stored,
    in both launches.  32 rows: one workgroup, two full chunks; 37 rows: a second workgroup with the ragged 5-row chunk."""
    monkeypatch.setenv("FRL_RC", "16")
    monkeypatch.setenv("FRL_CPS", "2")
    c = dict(so.case("o8_a4_bn"), batch=batch, n_table=256, n_learn=2, seed=7700 + batch)
    inp = so.inputs(c)
    e = _engine(N, c, batch_max=64)
    # rc from the engine; its cps (no getter in the C ABI) is pinned for exactly this engine by the plan on the CPU:
    # tests/test_engine_plan.py::test_rowchunk_addresses_stay_inside_the_plans_buffers ("rc 16 cps 2 S 2")
    assert e.lds_bytes()[1] == 16
    _load(e, inp)
    e.add_batch(records([inp["table"]]))
    o = so.make(c, inp)
    for k in range(c["n_learn"]):
        st = _learn(N, e, c, inp["idx"][k][None, None])
        cl, al, ll = o.learn_with(inp["idx"][k], c["gamma"], c["tau"])
        np.testing.assert_allclose(st[0, 0, [N.STAT_CRITIC_LOSS, N.STAT_ACTOR_LOSS, N.STAT_ALPHA_LOSS]], [cl, al, ll],
                                   rtol=1e-4, atol=1e-6, err_msg="cps2 batch %d call %d" % (batch, k))
    _check_state(e, o, c, c["n_learn"], "cps2 batch %d" % batch)
    e.close()


@pytest.mark.parametrize("P", [1, 40, 512])
def test_population(N, P):
    """P learners in one launch chain, each with its own parameters, table and rows; learners 0, the middle two and the last
    against oracles on exactly their inputs."""
    c = dict(so.case("o8_a4_bn"), batch=64, n_table=256, n_learn=2, bn=False)
    e = _engine(N, c, P=P)
    watch = sorted({0, P // 2 - 1 if P > 1 else 0, P // 2, P - 1})
    recs, idx, inps = [], np.zeros((P, 1, c["batch"]), np.int64), {}
    idxs = [[synth.indices(9000 + 31 * p + k, c["n_table"], c["batch"]) for p in range(P)] for k in range(c["n_learn"])]
    for p in range(P):
        cp = dict(c, seed=8000 + 10 * p)
        inp = dict(so.inputs(cp, n_learn=0), idx=[idxs[k][p] for k in range(c["n_learn"])])
        _load(e, inp, p)
        recs.append(records([inp["table"]]))
        if p in watch:
            inps[p] = (cp, inp)
    e.add_batch(np.concatenate(recs), learners=np.repeat(np.arange(P, dtype=np.int32), c["n_table"]))
    orcs = {p: so.make(cp, inp) for p, (cp, inp) in inps.items()}
    for k in range(c["n_learn"]):
        for p in range(P):
            idx[p, 0] = idxs[k][p]
        st = _learn(N, e, c, idx)
        for p, o in orcs.items():
            cl, al, ll = o.learn_with(idxs[k][p], c["gamma"], c["tau"])
            np.testing.assert_allclose(st[p, 0, [N.STAT_CRITIC_LOSS, N.STAT_ACTOR_LOSS, N.STAT_ALPHA_LOSS]], [cl, al, ll],
                                       rtol=1e-4, atol=1e-6, err_msg="learner %d call %d" % (p, k))
    for p, o in orcs.items():
        _check_state(e, o, c, c["n_learn"], "learner %d" % p, p=p)
    e.close()


def test_long_curve(N):
    """200 calls at O=8, A=4, B=256 against the reference's curve.  Measured, max relative difference per window of calls
    0-49 / 50-99 / 100-149 / 150-199:
        oracle vs reference   critic 2.2e-7 2.2e-7 2.2e-7 2.2e-7   actor 1.6e-7 2.4e-7 2.4e-7 2.4e-7
        engine vs reference   critic 2.3e-7 8.5e-7 1.4e-5 6.2e-5   actor 1.1e-6 4.4e-6 1.1e-4 4.3e-4   alpha <= 1e-6 throughout
    The engine's differences (MFMA summation order, and the ReLU flips of test_gpu_wide_population.py) grow by about 10x per 50
    calls past call 100.  So: both losses to 1e-4 over the first 100 calls (20x the measured 4.4e-6), a 2e-3 envelope over the
    last 100 (5x the measured 4.3e-4), alpha to 1e-5 and the alpha loss (which crosses zero) to 2e-3 of the curve's scale
    over all 200."""
    g = np.load(os.path.join(GOLDEN, "long_sac_discrete.npz"))
    c = so.case("long")
    inp = so.inputs(c)
    e = _engine(N, c)
    _load(e, inp)
    e.add_batch(records([inp["table"]]))
    got = np.array([_learn(N, e, c, inp["idx"][k][None, None])[0, 0] for k in range(c["n_learn"])])
    W = 100
    for stat, key in ((N.STAT_CRITIC_LOSS, "loss_critic"), (N.STAT_ACTOR_LOSS, "loss_actor")):
        np.testing.assert_allclose(got[:W, stat], g[key][:W], rtol=1e-4, err_msg=key + " calls 0-99")
        np.testing.assert_allclose(got[W:, stat], g[key][W:], rtol=2e-3, err_msg=key + " calls 100-199")
    np.testing.assert_allclose(got[:, N.STAT_ALPHA], g["alpha"], rtol=1e-5)
    np.testing.assert_allclose(got[:, N.STAT_ALPHA_LOSS], g["loss_alpha"], rtol=0, atol=2e-3 * np.abs(g["loss_alpha"]).max())
    e.close()


def test_device_draw(N):
    """Rows drawn on the device (no idx): 200 calls of finite, moving losses and alpha."""
    c = dict(so.case("o8_a4_bn"), n_table=1024)
    inp = so.inputs(c, n_learn=0)
    e = _engine(N, c)
    _load(e, inp)
    e.add_batch(records([inp["table"]]))
    kw = dict(gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], alpha_lr=c["alpha_lr"],
              target_entropy=0.6 * np.log(4.0), want_stats=True)
    st = np.array([e.learn(c["batch"], **kw)[0, 0] for _ in range(200)])
    assert np.all(np.isfinite(st))
    for k in (N.STAT_CRITIC_LOSS, N.STAT_ACTOR_LOSS, N.STAT_ALPHA):
        assert np.unique(st[:, k]).size > 150, k
    assert st[-1, N.STAT_ALPHA] != st[0, N.STAT_ALPHA]
    e.close()


def test_sac_class(N, tmp_path):
    """SAC(dim_info, is_continue=False, ...): the reference's state_dict keys and shapes, select_action = torch's
    Categorical(probs).sample() under the same generator state, evaluate_action = argmax, save / load, target_entropy."""
    from freerl_amd.SAC import SAC
    O, A = 4, 2
    pol = SAC([O, A], False, 1e-3, 3e-4, 1000, torch.device("cpu"), trick={"Batch_ObsNorm": False})
    H = 128
    want = {"actor": [("l1", H, O), ("l2", H, H), ("l3", A, H)],
            "critic": [("l1", H, O), ("l2", H, H), ("l3", A, H), ("l4", H, O), ("l5", H, H), ("l6", A, H)]}
    for net in ("actor", "critic", "actor_target", "critic_target"):
        sd = getattr(pol.agent, net).state_dict()
        layers = want[net.replace("_target", "")]
        assert list(sd.keys()) == [n + s for n, _, _ in layers for s in (".weight", ".bias")]
        for n, o, i in layers:
            assert tuple(sd[n + ".weight"].shape) == (o, i) and tuple(sd[n + ".bias"].shape) == (o,)
    te = 0.6 * (-torch.log(torch.tensor(1.0 / A)))            # SAC_add_discrete.py:218
    assert pol.alphas.target_entropy.dtype == torch.float32 and pol.alphas.target_entropy.item() == te.item()
    fx = np.load(os.path.join(GOLDEN, "sac_discrete.npz"))
    assert np.float32(pol.alphas.target_entropy.item()) == fx["o4_a2/target_entropy"]
    assert abs(pol.alphas.alpha.item() - 0.01) < 1e-9
    rng = np.random.default_rng(5)
    for i in range(64):
        obs = rng.standard_normal(O).astype(np.float32)
        torch.manual_seed(100 + i)
        a = pol.select_action(obs)
        assert isinstance(a, np.int64)
        torch.manual_seed(100 + i)
        probs = pol.agent.actor(obs.reshape(1, -1))
        assert int(torch.distributions.Categorical(probs=probs).sample().item()) == int(a)
        assert pol.evaluate_action(obs) == int(np.argmax(probs.numpy()[0]))
    # one learn() through the class (host draw), then the checkpoint round trip
    for i in range(300):
        pol.add(rng.standard_normal(O), int(rng.integers(A)), float(rng.standard_normal()), rng.standard_normal(O), False)
    pol.track_loss = True
    pol.learn(64, 0.99, 0.01)
    assert all(np.isfinite(pol.last_losses))
    pol.save(str(tmp_path))
    back = SAC.load([O, A], False, str(tmp_path), trick={"Batch_ObsNorm": False})
    for k, v in pol.agent.actor.state_dict().items():
        assert torch.equal(v, back.agent.actor.state_dict()[k])


def test_rejections(N):
    """What the discrete kernels do not take is refused at frl_create; fused collection is not offered."""
    from freerl_amd.engine import Engine
    for kw in (dict(act_dim=65), dict(hidden=512)):
        with pytest.raises(N.FrlError):
            Engine(N.ALGO_SAC_DISCRETE, 8, kw.get("act_dim", 4), 256, twin_critic=True, hidden=kw.get("hidden", 128))
    e = Engine(N.ALGO_SAC_DISCRETE, 8, 64, 256, twin_critic=True, batch_max=256)      # 64 actions: four head tiles
    e.add_batch(np.zeros((64, e.width), np.float32))
    with pytest.raises(N.FrlError):                                                    # the reference's loss is MSE only
        e.learn(8, gamma=0.99, tau=0.01, idx=np.arange(8)[None, None], huber_delta=1.0)
    L = N.lib()
    assert L.frl_rollout(e._h, None, None, None) == 4                                 # FRL_ERR_STATE
    obs = np.zeros((1, 1, 8), np.float32)
    with pytest.raises(N.FrlError):
        e.act_explore(N.ACT_ARGMAX, obs, kind=1)
    e.close()


def test_training_loop_follows_the_reference(N, tmp_path):
    """freerl_amd.train sac_discrete against SAC_add_discrete.py's own `__main__` loop (tests/golden/loop_sacd_cartpole.npz,
    make_sacd_golden.py): same flags, in-repo CartPole, same seeds -> the discrete actions identical step by step (64 action-space
    samples, then Categorical draws, 128 learn() calls with Batch_ObsNorm), returns to 1e-3, same result files."""
    from freerl_amd import envs as E
    from freerl_amd import train
    from tests.golden.make_loop_golden import Recorder
    fx = np.load(os.path.join(GOLDEN, "loop_sacd_cartpole.npz"))
    argv = str(fx["flags"]).replace("--device cpu", "--device cuda").split() + ["--results_root", str(tmp_path / "results")]
    log = dict(actions=[], rewards=[])
    env = Recorder(E.make("CartPole-v1", prefer_gymnasium=False), log)
    out = train.run("sac_discrete", argv, env=env, log=lambda *a: None)
    acts, rews = np.stack(log["actions"]), np.stack(log["rewards"])
    assert acts.shape == fx["actions"].shape, (acts.shape, fx["actions"].shape)
    np.testing.assert_array_equal(acts, fx["actions"])
    np.testing.assert_allclose(rews, fx["rewards"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(out["returns"], fx["returns"], rtol=1e-3, atol=1e-3)
    files = sorted(os.listdir(out["model_dir"]))
    assert str(fx["npy_name"]) in files and str(fx["ckpt_name"]) in files, files
    assert "SAC_add_discrete_running_mean_std_batch_size.npy" in files, files
    assert os.path.basename(out["model_dir"]).startswith("SAC_add_discrete_Batch_ObsNorm_")
    sd = torch.load(os.path.join(out["model_dir"], str(fx["ckpt_name"])))
    synth.check_digest("ckpt", {k: v.numpy() for k, v in sd.items()}, fx, 5e-3, 5e-4, "loop_sacd_cartpole")
