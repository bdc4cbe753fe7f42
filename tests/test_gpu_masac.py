"""GPU: MASAC (MAAC_file/MASAC.py) on kernels_masac.hip, against the reference's recorded outputs (tests/golden/masac.npz) and the NumPy
restatement (tests/masac_oracle.py) on exactly the reference's rows and draws.

Tolerances: tests/masac_oracle.py: tolerances() — the project's (losses rtol 1e-4 / atol 1e-6, norms rtol 1e-3, _assert_net's rule for
parameters, _assert_m's for Adam's first moment), unwidened in pair, hetero, spread3 and seq.  In `clamp` the LOSS tolerance is 4 x the
float32-float64 gap measured on the CPU (the number format's, whatever the engine is compared with); norms, parameters, Adam's m and
alpha's exp_avg keep the project's tolerances against the oracle and are 4 x the RECORDING's gap against the recording only (torch's
autograd noise at std = 2e-9, which the closed form of oracle and kernel does not have): tests/masac_oracle.py says which and why."""
import os

import numpy as np
import pytest

from tests import masac_oracle as mo
from tests.hip_helpers import flat_params, records
from tests.test_gpu_envelope_ddpg import _assert_m, _assert_net

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ST_CRITIC_LOSS, ST_ACTOR_LOSS, ST_ALPHA, ST_CRITIC_GNORM, ST_ACTOR_GNORM = 0, 1, 3, 4, 5          # enum frl_stat


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "masac.npz")))


def _engine(N, c, P=1, batch_max=None, seed=0):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_MASAC, [o for o, _ in c["dims"]], [a for _, a in c["dims"]], c["n_table"], n_learners=P, hidden=c["hidden"],
                  batch_max=batch_max or c["batch"], seed=seed, twin_critic=True)


def _load(e, c, inp, p=0):
    a0 = c["alpha0"] or [0.01] * len(c["dims"])
    for j in range(len(inp["actor"])):
        for kind in (0, 1):
            e.set_params(2 * j, flat_params(inp["actor"][j], mo.ACTOR_NAMES), kind, learner=p)
            e.set_params(2 * j + 1, flat_params(inp["critic"][j], mo.CRITIC_NAMES), kind, learner=p)
        la = np.float32(np.log(a0[j]))
        e.set_alpha_state_agent(j, [la, 0.0, 0.0, np.exp(la)], 0, learner=p)


def _learn(e, c, idx, eps, **kw):
    """idx [P, n, B], eps [P, n, 2 n + 1, B, act_max] -> stats [P, n, 8]"""
    return e.learn(np.asarray(idx).shape[-1], gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], alpha_lr=mo.ALPHA_LR,
                   idx=idx, noise=eps, want_stats=True, **kw)


def _eps(c, eps_call, B=None):
    n = len(c["dims"])
    return mo.pad_eps(eps_call, n, B or c["batch"], max(a for _, a in c["dims"]))


def _check_state(e, o, c, calls, label, tol, p=0):
    for j in range(len(c["dims"])):
        for net, online, target, opt, lr, names in ((2 * j, o.actor[j], o.actor_t[j], o.aopt[j], c["actor_lr"], mo.ACTOR_NAMES),
                                                    (2 * j + 1, o.critic[j], o.critic_t[j], o.copt[j], c["critic_lr"], mo.CRITIC_NAMES)):
            tag = "%s agent %d %s" % (label, j, "actor" if net % 2 == 0 else "critic")
            _assert_net(e.get_params(net, 0, p), online, names, tol["param"][0], tol["param"][1], lr, calls, tag)
            _assert_net(e.get_params(net, 1, p), target, names, tol["param"][0], tol["param"][1], lr, calls, tag + " target")
            _assert_m(e.get_params(net, 2, p), opt.m, names, tag)
            assert e.opt_step(net, learner=p) == calls == opt.t, tag
        v, step = e.alpha_state_agent(j, learner=p)
        np.testing.assert_allclose(v[0], float(o.log_alpha[j]["log_alpha"]), rtol=1e-5, err_msg=label + " log_alpha")
        np.testing.assert_allclose(v[3], float(o.alpha(j)), rtol=tol["alpha"], err_msg=label + " alpha")
        np.testing.assert_allclose(v[1], float(o.alopt[j].m["log_alpha"]), rtol=tol["alpha_m"], atol=1e-9, err_msg=label + " alpha exp_avg")
        assert step == calls


def _assert_call(st, want, tol, label):
    np.testing.assert_allclose(st[:, ST_CRITIC_LOSS], want["critic_loss"], rtol=tol["loss"][0], atol=tol["loss"][1], err_msg="critic loss, " + label)
    np.testing.assert_allclose(st[:, ST_ACTOR_LOSS], want["actor_loss"], rtol=tol["loss"][0], atol=tol["loss"][1], err_msg="actor loss, " + label)
    np.testing.assert_allclose(st[:, ST_CRITIC_GNORM], want["critic_norm"], rtol=tol["norm"], err_msg="critic norm, " + label)
    np.testing.assert_allclose(st[:, ST_ACTOR_GNORM], want["actor_norm"], rtol=tol["norm"], err_msg="actor norm, " + label)
    np.testing.assert_allclose(st[:, ST_ALPHA], np.array(want["alpha"], np.float64), rtol=tol["alpha"], err_msg="alpha, " + label)


def _check_digests(e, fx, pre, c, tol):
    """the engine's nets, targets and Adam m against the REFERENCE's recorded digests"""
    for j in range(len(c["dims"])):
        for net, key, names in ((2 * j, "actor", mo.ACTOR_NAMES), (2 * j + 1, "critic", mo.CRITIC_NAMES)):
            tmpl = {k2: np.zeros(s) for (k2, s) in _shapes(c, j, key)}
            for kind, suffix in ((0, ""), (1, "_target")):
                from tests.hip_helpers import unflat_params
                got = unflat_params(e.get_params(net, kind), tmpl, names)
                p = "%s/%d/%s%s" % (pre, j, key, suffix)
                mo.check_digest(got, names, fx[p + "/stats"], fx[p + "/sample"], tol["param"][0], tol["param"][1], p)
            got = unflat_params(e.get_params(net, 2), tmpl, names)
            p = "%s/%d/%s_m" % (pre, j, key)
            scale = float(np.abs(fx[p + "/sample"]).max())
            mo.check_digest(got, names, fx[p + "/stats"], fx[p + "/sample"], tol["m"], tol["m"] * scale, p)


def _shapes(c, j, key):
    layers = mo.actor_layers(c, j) if key == "actor" else mo.critic_layers(c)
    return [(n + suf, (o, i) if suf == ".weight" else (o,)) for n, o, i in layers for suf in (".weight", ".bias")]


@pytest.mark.parametrize("name", list(mo.CASES))
def test_golden_and_oracle(N, fx, name):
    """Every case, after 1 and 3 calls, on the rows and draws the reference took: losses, pre-clip norms and alpha per agent against the
    reference and the oracle; every net, target, Adam m and alpha with its Adam state against both; no padding slot written."""
    c = mo.case(name)
    inp = mo.inputs(c)
    tol, tol_ref = mo.tolerances(name, "oracle"), mo.tolerances(name, "reference")
    n = len(c["dims"])
    e = _engine(N, c)
    assert e.n_nets == 2 * n and e.learn_path(c["batch"])[0] is False
    _load(e, c, inp)
    e.add_batch(records(inp["table"]))
    o = mo.make(c, inp)
    for k in range(c["n_learn"]):
        idx, eps = fx[name + "/idx"][k], fx[name + "/eps"][k]
        st = _learn(e, c, idx[None], eps[None])[0]
        want = o.learn_with(idx, inp["eps"][k], c["gamma"], c["tau"])
        print("%s call %d: critic loss %s reference %s | actor loss %s reference %s | norms %s %s reference %s %s | alpha %s reference %s" %
              (name, k, st[:, 0], fx[name + "/critic_loss"][k], st[:, 1], fx[name + "/actor_loss"][k], st[:, 4], st[:, 5],
               fx[name + "/critic_norm"][k], fx[name + "/actor_norm"][k], st[:, 3], fx[name + "/alpha"][k]))
        ref = {key: fx["%s/%s" % (name, key)][k] for key in ("critic_loss", "actor_loss", "critic_norm", "actor_norm", "alpha")}
        _assert_call(st, ref, tol_ref, "call %d vs reference" % k)
        _assert_call(st, want, tol, "call %d vs oracle" % k)
        if k + 1 in mo.RECORD_AFTER:
            _check_state(e, o, c, k + 1, name + " after %d" % (k + 1), tol)
            _check_digests(e, fx, "%s/after%d" % (name, k + 1), c, tol_ref)
    for net in range(2 * n):
        assert e.pad_max(net) == 0.0 and e.pad_max(net, 1) == 0.0 and e.pad_max(net, 2) == 0.0
    e.close()


def _against_oracle(N, c, inp, e, calls, label, B=None):
    """`calls` learn() calls on the oracle's rows and draws: losses, norms, alpha per call, then every net, target, Adam m and alpha"""
    tol = mo.tolerances("-")
    _load(e, c, inp)
    e.add_batch(records(inp["table"]))
    o = mo.make(c, inp)
    for k in range(calls):
        st = _learn(e, c, inp["idx"][k][None], _eps(c, inp["eps"][k], B)[None])[0]
        _assert_call(st, o.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"]), tol, "%s call %d" % (label, k))
    _check_state(e, o, c, calls, label, tol)
    assert all(e.pad_max(net, kind) == 0.0 for net in range(e.n_nets) for kind in (0, 1, 2))


@pytest.mark.parametrize("B", [100, 128])
def test_two_chunks_per_workgroup(N, B, monkeypatch):
    """FRL_CPS=2 (the create-time knob the other row-chunk tests use): a workgroup walks two row chunks and its second chunk ADDS to
    the slab its first one stored, in the critic and in every per-agent actor launch; 100 rows leave the last chunk ragged"""
    monkeypatch.setenv("FRL_CPS", "2")
    c = mo.case("hetero")
    inp = mo.inputs(c, n_learn=2, batch=B, seed=8700)
    e = _engine(N, c, batch_max=128)
    rc = e.lds_bytes()[1]
    assert rc < B and (128 // rc) % 2 == 0, rc
    _against_oracle(N, c, inp, e, 2, "cps2 B%d" % B, B)
    e.close()


def test_single_agent(N):
    """n_agents = 1: one actor, one twin critic, 3 draw sets; frl_alpha_get / _set serve the one agent"""
    c = dict(mo.COMMON, dims=[(11, 3)], hidden=64, batch=40, seed=8600, rew_scale=[1.0])
    inp = mo.inputs(c, n_learn=2)
    e = _engine(N, c)
    assert e.n_nets == 2 and e.noise_sets == 3
    _against_oracle(N, c, inp, e, 2, "single")
    v, t = e.alpha_state()
    va, ta = e.alpha_state_agent(0)
    assert v.tolist() == va.tolist() and t == ta == 2
    e.set_alpha_state([-1.0, 0.5, 0.25, 0.125], 9)
    v, t = e.alpha_state_agent(0)
    assert v.tolist() == [-1.0, 0.5, 0.25, 0.125] and t == 9
    e.close()


def test_two_learners_are_two_engines(N):
    """P = 2 learners with different data and parameters give the bits of two P = 1 engines"""
    c = mo.case("hetero")
    inps = [mo.inputs(c, seed=9100 + 100 * p) for p in range(2)]
    n = len(c["dims"])
    e2 = _engine(N, c, P=2)
    for p in range(2):
        _load(e2, c, inps[p], p)
        e2.add_batch(records(inps[p]["table"]), learners=np.full(c["n_table"], p))
    solo = []
    for p in range(2):
        e = _engine(N, c)
        _load(e, c, inps[p])
        e.add_batch(records(inps[p]["table"]))
        solo.append(e)
    for k in range(2):
        idx = np.stack([inps[p]["idx"][k] for p in range(2)])
        eps = np.stack([_eps(c, inps[p]["eps"][k]) for p in range(2)])
        st2 = _learn(e2, c, idx, eps)
        for p in range(2):
            st = _learn(solo[p], c, idx[p][None], eps[p][None])
            np.testing.assert_array_equal(st2[p], st[0])
    for p in range(2):
        for net in range(2 * n):
            for kind in (0, 1, 2, 3):
                np.testing.assert_array_equal(e2.get_params(net, kind, p), solo[p].get_params(net, kind))
        for j in range(n):
            a, b = e2.alpha_state_agent(j, learner=p), solo[p].alpha_state_agent(j)
            np.testing.assert_array_equal(a[0], b[0])
            assert a[1] == b[1] == 2
        solo[p].close()
    e2.close()


def test_device_draws(N):
    """noise = NULL, idx = NULL: finite results, rows within range and distinct, the same seed twice gives the same bits"""
    c = mo.case("spread3")
    inp = mo.inputs(c, n_learn=1)
    outs = []
    for _ in range(2):
        e = _engine(N, c, seed=1234)
        _load(e, c, inp)
        e.add_batch(records(inp["table"]))
        sts = [e.learn(c["batch"], gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], want_stats=True) for _ in range(3)]
        rows = e.last_indices(c["batch"])
        assert rows.min() >= 0 and rows.max() < c["n_table"]
        assert all(len(set(rows[0, j].tolist())) == c["batch"] for j in range(len(c["dims"])))
        assert all(np.isfinite(s).all() for s in sts)
        params = [e.get_params(net, kind) for net in range(e.n_nets) for kind in (0, 1)]
        assert all(np.isfinite(p).all() for p in params)
        assert all(e.pad_max(net, kind) == 0.0 for net in range(e.n_nets) for kind in (0, 1, 2, 3))
        outs.append((sts, params, rows))
        e.close()
    for a, b in zip(outs[0][0], outs[1][0]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(outs[0][1], outs[1][1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


def test_act(N):
    """frl_act: Q of both heads, online and target, on rows [all obs | all actions]; FRL_ACT_SAC_SAMPLE, FRL_ACT_TANHHEAD and FRL_ACT_RAW
    on the stacked [mean | log_std] head — against the oracle's forward, after one call (online and target differ)"""
    c = mo.case("hetero")
    inp = mo.inputs(c)
    n = len(c["dims"])
    e = _engine(N, c, batch_max=64)
    _load(e, c, inp)
    e.add_batch(records(inp["table"]))
    o = mo.make(c, inp)
    _learn(e, c, inp["idx"][0][None], _eps(c, inp["eps"][0])[None])
    o.learn_with(inp["idx"][0], inp["eps"][0], c["gamma"], c["tau"])
    rows = np.arange(37)
    t = inp["table"]
    obs, act = [x["obs"][rows] for x in t], [x["act"][rows] for x in t]
    x = np.concatenate(obs + act, axis=1)
    for j in range(n):
        for tgt, p in ((False, o.critic[j]), (True, o.critic_t[j])):
            q1, q2, _, _ = o.q(p, obs, act)
            for h, want in ((0, q1), (1, q2)):
                got = e.act(2 * j + 1, N.ACT_RAW, x[None], out_dim=1, head=h, use_target=tgt)[0]
                np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg="Q%d agent %d target %s" % (h + 1, j, tgt))
        A = c["dims"][j][1]
        eps = np.random.default_rng(j).standard_normal((37, A)).astype(np.float32)
        for tgt, p in ((False, o.actor[j]), (True, o.actor_t[j])):
            a, _, k = mo.actor_forward(p, obs[j], eps)
            np.testing.assert_allclose(e.act(2 * j, N.ACT_SAC_SAMPLE, obs[j][None], eps=eps[None], out_dim=A, use_target=tgt)[0], a, rtol=1e-4, atol=1e-6)
            np.testing.assert_allclose(e.act(2 * j, N.ACT_TANHHEAD, obs[j][None], out_dim=A, use_target=tgt)[0], np.tanh(k["mean"]), rtol=1e-4, atol=1e-6)
            np.testing.assert_allclose(e.act(2 * j, N.ACT_RAW, obs[j][None], out_dim=2 * A, use_target=tgt)[0], np.concatenate([k["mean"], k["raw"]], axis=1),
                                       rtol=1e-4, atol=1e-6)
    e.close()


def test_alpha_accessors_and_refusals(N):
    c = mo.case("pair")
    inp = mo.inputs(c)
    e = _engine(N, c)
    _load(e, c, inp)
    e.add_batch(records(inp["table"]))
    e.set_alpha_state_agent(1, [-1.5, 0.25, 0.125, 0.5], 7)
    v, t = e.alpha_state_agent(1)
    assert v.tolist() == [-1.5, 0.25, 0.125, 0.5] and t == 7
    v0, t0 = e.alpha_state_agent(0)
    np.testing.assert_allclose(v0, [np.log(0.01), 0, 0, 0.01], rtol=1e-6)
    assert t0 == 0
    L = N.lib()

    def refused(call, *words):
        with pytest.raises(N.FrlError) as ei:
            call()
        msg = str(ei.value)
        assert all(w in msg for w in words), msg
        return msg
    refused(lambda: e.alpha_state(), "frl_alpha_get_agent")
    refused(lambda: e.set_alpha_state([0, 0, 0, 1.0]), "frl_alpha_set_agent")
    refused(lambda: e.obsnorm_enable(True), "Batch_ObsNorm")
    idx, eps = inp["idx"][0][None], _eps(c, inp["eps"][0])[None]
    refused(lambda: _learn(e, c, idx, eps, use_policy_noise=True), "use_policy_noise")
    refused(lambda: e.act_explore(N.ACT_SAC_SAMPLE, np.zeros((1, 1, c["dims"][0][0]), np.float32), kind=0, out_dim=4), "frl_act_explore", "MASAC")
    import ctypes as C
    assert L.frl_rollout(e._h, None, None, None) == 4      # FRL_ERR_STATE, said before the arguments are looked at
    assert b"frl_rollout" in L.frl_last_error()
    e.close()


def test_existing_engines_keep_their_bits(N):
    """a TD3, a SAC and a MATD3 engine at one small shape give the same bits before and after a MASAC engine is created and trained in
    the same process"""
    from freerl_amd.engine import Engine
    from tests.golden import synth

    def run(algo, dims, twin, noise_sets):
        e = Engine(algo, [o for o, _ in dims], [a for _, a in dims], 128, hidden=64, batch_max=32, seed=5, twin_critic=twin)
        e.fill_synthetic(128, seed=3)
        n = len(dims)
        for net in range(e.n_nets):
            flat = synth.normal(100 + net, (e.num_params(net),)) * np.float32(0.1)
            e.set_params(net, flat, 0)
            e.set_params(net, flat, 1)
        if algo == N.ALGO_SAC:
            e.set_alpha_state([np.log(0.2), 0, 0, 0.2], 0)
        idx = np.stack([synth.indices(50 + j, 128, 32) for j in range(n)])[None]
        noise = synth.normal(60, (1, n, noise_sets, 32, max(a for _, a in dims)))
        st = e.learn(32, gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3, idx=idx, noise=noise, want_stats=True,
                     use_policy_noise=algo != N.ALGO_SAC, policy_noise=0.2, noise_clip=0.5, target_entropy=-2.0)
        out = [st] + [e.get_params(net, kind) for net in range(e.n_nets) for kind in (0, 1, 2, 3)]
        e.close()
        return out
    shapes = [(N.ALGO_TD3, [(5, 2)], True, 2), (N.ALGO_SAC, [(5, 2)], True, 2), (N.ALGO_MADDPG, [(5, 2), (4, 1)], True, 2)]
    before = [run(*s) for s in shapes]
    c = mo.case("pair")
    inp = mo.inputs(c)
    m = _engine(N, c)
    _load(m, c, inp)
    m.add_batch(records(inp["table"]))
    _learn(m, c, inp["idx"][0][None], _eps(c, inp["eps"][0])[None])
    after = [run(*s) for s in shapes]
    m.close()
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


DIM_INFO = {"agent_0": [6, 2], "agent_1": [5, 3], "agent_2": [6, 2]}


def _drive(pol, steps=40, seed=0):
    g = np.random.default_rng(seed)
    for _ in range(steps):
        obs = {a: g.standard_normal(d[0]).astype(np.float32) for a, d in DIM_INFO.items()}
        act = pol.select_action(obs)
        pol.add(obs, act, {a: float(g.standard_normal()) for a in DIM_INFO}, {a: g.standard_normal(d[0]).astype(np.float32) for a, d in DIM_INFO.items()},
                {a: bool(g.random() < 0.1) for a in DIM_INFO})
    return obs


def test_class(N, tmp_path):
    """two MASAC instances in one process; learn in host-RNG mode is reproducible under the same seeds; save / load round trip;
    update_target; the reference's state_dict keys"""
    import torch
    from freerl_amd.MASAC import MASAC
    pols = []
    for _ in range(2):
        torch.manual_seed(11)
        np.random.seed(11)
        pol = MASAC(DIM_INFO, True, 1e-3, 1e-3, 64, "cpu", rng="host", batch_max=16)
        obs = _drive(pol)
        for _ in range(3):
            pol.learn(8, 0.95, 0.01)
        pols.append(pol)
    a, b = pols
    for aid in DIM_INFO:
        sa, sb = a.agents[aid].actor.state_dict(), b.agents[aid].actor.state_dict()
        assert list(sa) == ["l1.weight", "l1.bias", "l2.weight", "l2.bias", "mean_layer.weight", "mean_layer.bias", "log_std_layer.weight", "log_std_layer.bias"]
        assert list(a.agents[aid].critic_target.state_dict()) == [n + s for n in mo.CRITIC_NAMES for s in (".weight", ".bias")]
        for k in sa:
            assert torch.equal(sa[k], sb[k]) and torch.isfinite(sa[k]).all()
        assert float(a.alphas[aid].alpha) == float(b.alphas[aid].alpha) != 0.01
        assert a.alphas[aid].target_entropy == -DIM_INFO[aid][1]
        np.testing.assert_allclose(float(a.alphas[aid].log_alpha.exp()), float(a.alphas[aid].alpha), rtol=1e-6)
    ev = a.evaluate_action(obs)
    assert all(ev[aid].shape == (DIM_INFO[aid][1],) and np.abs(ev[aid]).max() <= 1 for aid in DIM_INFO)
    q1, q2 = a.agents["agent_1"].critic([torch.zeros(4, d[0]) for d in DIM_INFO.values()], [torch.zeros(4, d[1]) for d in DIM_INFO.values()])
    assert q1.shape == q2.shape == (4, 1)
    act, lp = a.agents["agent_1"].actor(torch.zeros(4, 5))
    assert act.shape == (4, 3) and lp.shape == (4, 1)
    # update_target
    before = a.agents["agent_0"].critic_target.state_dict()
    online = a.agents["agent_0"].critic.state_dict()
    a.update_target(0.5)
    after = a.agents["agent_0"].critic_target.state_dict()
    for k in before:
        np.testing.assert_allclose(after[k].numpy(), 0.5 * before[k].numpy() + 0.5 * online[k].numpy(), rtol=1e-6, atol=1e-7)
    # save / load
    a.save(str(tmp_path))
    assert os.path.exists(os.path.join(str(tmp_path), "MASAC.pth"))
    c = MASAC.load(DIM_INFO, True, str(tmp_path))
    for aid in DIM_INFO:
        sa, sc = a.agents[aid].actor.state_dict(), c.agents[aid].actor.state_dict()
        assert all(torch.equal(sa[k], sc[k]) for k in sa)
    evc = c.evaluate_action(obs)
    assert all(np.array_equal(ev[aid], evc[aid]) for aid in DIM_INFO)
