"""GPU: action-masked MAPPO (MAPPO_file/MAPPO_for_mask_action.py) on kernels_mappo_mask.hip, against the reference's recorded outputs
(tests/golden/mappo_mask.npz, loop_mappo_mask.npz) and the NumPy restatement (tests/mappo_mask_oracle.py), at the smallest shapes at
which each part can go wrong: three agents of unequal dims (5, 4), (4, 3), (5, 6), hidden 32, horizon 40 in ONE minibatch (several
row chunks with a short last one), K 2.

Tolerances are tests/test_gpu_mappo.py's: advantages and value targets rtol 1e-5 / atol 2e-6, losses rtol 1e-4 / atol 1e-6, parameters
and Adam's first moment by tests/mappo_oracle.py's assert_net / assert_m."""
import os

import numpy as np
import pytest

from tests import mappo_mask_oracle as mm
from tests import mappo_oracle as mo
from tests.hip_helpers import records

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "mappo_mask.npz")))


@pytest.fixture(scope="module")
def loop_fx():
    return dict(np.load(os.path.join(HERE, "golden", "loop_mappo_mask.npz")))


@pytest.fixture(scope="module")
def runs():
    """the oracle's run of a case, computed once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mm.run(mm.case(name))
        return cache[name]
    return get


def _extra_cols(c, masked=True):
    n, acts = len(c["dims"]), sum(a for _, a in c["dims"])
    if c["cont"]:
        return acts + n
    return 2 * n + (acts if masked else 0)


def _engine(N, c, P=1, masked=True, algo=None, **kw):
    from freerl_amd.engine import Engine
    args = dict(n_learners=P, discrete=not c["cont"], hidden=c["hidden"], batch_max=c["horizon"], extra_cols=_extra_cols(c, masked))
    args.update(kw)
    e = Engine(N.ALGO_MAPPO if algo is None else algo, [o for o, _ in c["dims"]], [a for _, a in c["dims"]], c["horizon"], **args)
    e.net_norm_set(c["trick"]["feature_norm"], c["trick"]["LayerNorm"])
    if masked and not c["cont"]:
        e.action_mask_set(True)
    return e


def _records(c, rows, masked=True):
    """[log-prob blocks | one adv_done column per agent | one mask block per agent]"""
    cols = [r["logp"] for r in rows] + [r["adv_done"] for r in rows]
    if masked and not c["cont"]:
        cols += [r["mask"].astype(F32) for r in rows]
    return records(rows, np.concatenate(cols, axis=1))


def _load(e, c, inp, p=0):
    for i in range(len(c["dims"])):
        e.set_params(2 * i, mo.flat(c, "actor", inp["actors"][i]), learner=p)
        e.set_params(2 * i + 1, mo.flat(c, "critic", inp["critics"][i]), learner=p)


def _hyper(c):
    """what freerl_amd.MAPPO_for_mask_action passes: two Adams per agent, eps 1e-5 with trick['adam_eps'], clipped at 0.5"""
    t = c["trick"]
    return dict(gamma=c["gamma"], lmbda=c["lmbda"], clip=c["clip"], ent_coef=c["ent_coef"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"],
                adv_norm=t["adv_norm"], value_clip=t["ValueClip"], huber_delta=c["huber_delta"] if t["huber_loss"] else None,
                adam_eps=1e-5 if t["adam_eps"] else 1e-8, clip_norm=0.5)


def _learn(e, c, perms):
    return e.mappo_learn(c["horizon"], c["horizon"], c["k_epochs"], perms=perms, want_trace=True, want_adv=True, **_hyper(c))


def _run(N, c, inps, perms, masked=True):
    """the case's learn() calls on one engine for len(inps) learners: rows 0 .. fill-1 added, learn, [the second rows, learn].
    perms [P][calls][n][K][T] -> (engine, the last call's adv / v_target, the calls' traces side by side)"""
    P = len(inps)
    e = _engine(N, c, P=P, masked=masked)
    fill = c["horizon"] if c["fill"] is None else c["fill"]
    for p, inp in enumerate(inps):
        _load(e, c, inp, p)
    e.add_batch(np.concatenate([_records(c, inp["rows"], masked)[:fill] for inp in inps]), learners=np.repeat(np.arange(P), fill).astype(np.int32))
    assert e.cursor(0) == (fill % c["horizon"], fill)
    out = _learn(e, c, perms[:, 0])
    traces = [out["trace"]]
    assert e.cursor(0) == (0, 0)                    # Buffer_for_PPO_mask.clear: counters only
    if c["second"]:
        k = c["second"]
        e.add_batch(np.concatenate([_records(c, mm.second_rows(c), masked)[:k] for _ in inps]), learners=np.repeat(np.arange(P), k).astype(np.int32))
        out = _learn(e, c, perms[:, 1])
        traces.append(out["trace"])
    out["trace"] = np.concatenate(traces, axis=2)
    return e, out


def _check_against(e, c, o, fx, name, out, p=0):
    n, steps = len(c["dims"]), c["k_epochs"] * mm.calls(c)
    print("%s: first losses kernel %s reference %s oracle %s" % (name, out["trace"][p, 0, 0], fx[name + "/trace"][0, 0], o.trace[0, 0]))
    for want, who in ((fx[name + "/adv"], "reference"), (o.adv_raw, "oracle")):
        np.testing.assert_allclose(out["adv"][p], want, rtol=1e-5, atol=2e-6, err_msg="adv vs " + who)
    for want, who in ((fx[name + "/v_target"], "reference"), (o.v_target, "oracle")):
        np.testing.assert_allclose(out["v_target"][p], want, rtol=1e-5, atol=2e-6, err_msg="v_target vs " + who)
    for want, who in ((fx[name + "/trace"], "reference"), (o.trace, "oracle")):
        np.testing.assert_allclose(out["trace"][p], want, rtol=1e-4, atol=1e-6, err_msg="loss trace vs " + who)
    for i in range(n):
        for net, tag, want, opt, lr in ((2 * i, "actor", o.actors[i], o.aopt[i], c["actor_lr"]), (2 * i + 1, "critic", o.critics[i], o.copt[i], c["critic_lr"])):
            key = "%s/%d/%s" % (name, i, tag)
            got = e.get_params(net, 0, p)
            if key + "/p" in fx:
                mo.assert_net(got, fx[key + "/p"], lr, steps, key + " vs reference")
            mo.assert_net(got, mo.flat(c, tag, want), lr, steps, key + " vs oracle")
            mo.assert_m(e.get_params(net, 2, p), mo.flat(c, tag, opt.m), key)
            assert e.opt_step(net, learner=p) == steps == int(fx[key + "/step"])
            assert e.pad_max(net, 0, p) == 0.0


@pytest.mark.parametrize("name", list(mm.CASES))
def test_golden_and_oracle(N, fx, runs, name):
    """plain / tricks / partial (13 all-closed zero rows: the normalisation order) / stale (a second learn over 18 new and 22 old rows) /
    edges (one open action, all open) / wide (3 x (18, 11), hidden 128) / cont (masks stored, never read)"""
    c = mm.case(name)
    e, out = _run(N, c, [mm.inputs(c)], fx[name + "/perms"][None])
    if name == "partial":      # the loss the other normalisation order would give is further than 1e-3 away (recorded by the maker)
        other = fx["partial/first_actor_loss_other_order"]
        assert (np.abs(out["trace"][0, :, 0, 0] - other) > 1e-3 * np.abs(other)).all()
    _check_against(e, c, runs(name), fx, name, out)


def test_act_masked_with_injected_draws(N, loop_fx):
    """the reference class's first episode (its parameters not yet updated): its actions exactly, its log-probs at atol 1e-6; then 70
    rows (two row chunks) per agent against the oracle's masked sample"""
    c, env = mm.LOOP, mm.ToyEnv()
    inp = mm.inputs(c)
    e = _engine(N, c)
    _load(e, c, inp)
    T = mm.LOOP_EPISODES[0]
    rng = np.random.Generator(np.random.PCG64(9))
    for i, (O, A) in enumerate(c["dims"]):
        got, lp = e.act_masked(2 * i, env.obs[i][:T], env.mask[i][:T], eps=loop_fx["q/%d" % i][:T], want_logp=True)
        print("agent %d: max |logp - reference| %.3g" % (i, np.abs(lp[0] - loop_fx["logp"][:T, i]).max()))
        assert np.array_equal(got[0], loop_fx["actions"][:T, i])
        np.testing.assert_allclose(lp[0], loop_fx["logp"][:T, i], rtol=0, atol=1e-6)
        rows = 70
        obs = rng.normal(0, 1, (rows, O)).astype(F32)
        mask = rng.random((rows, A)) < 0.5
        mask[np.arange(rows), rng.integers(0, A, rows)] = True
        mask[:3] = False                                      # all closed: p = 1 / A, log-prob exactly 0
        q = rng.exponential(1.0, (rows, A)).astype(F32)
        want, wlp, margin = mm.sample(mo.forward(inp["actors"][i], mo.ACTOR_D, obs, c["trick"])[0], mask, q)
        got, lp = e.act_masked(2 * i, obs, mask, eps=q, want_logp=True)
        sure = margin > 1e-3
        assert sure.mean() > 0.9 and np.array_equal(got[0][sure], want[sure])
        np.testing.assert_allclose(lp[0][sure], wlp[sure], rtol=2e-5, atol=2e-5)
        assert np.all(lp[0][:3] == 0)
        open_rows = mask.any(axis=1)
        assert mask[np.arange(rows), got[0].astype(int)][open_rows].all()


def test_device_draws_respect_the_mask(N):
    """4096 device-drawn rows with random masks: a closed action is never drawn; then 8 (observation, mask) pairs x 512 rows: every
    action's frequency within 5 standard errors of the oracle's masked probability (0 for a closed one)"""
    c = mm.case("plain")
    inp = mm.inputs(c)
    e = _engine(N, c)
    _load(e, c, inp)
    rng = np.random.Generator(np.random.PCG64(10))
    i, (O, A) = 2, c["dims"][2]
    rows = 4096
    obs = rng.normal(0, 1, (rows, O)).astype(F32)
    mask = rng.random((rows, A)) < 0.5
    mask[np.arange(rows), rng.integers(0, A, rows)] = True
    got = e.act_masked(2 * i, obs, mask)[0].astype(int)
    assert got.min() >= 0 and got.max() < A and mask[np.arange(rows), got].all()
    again = e.act_masked(2 * i, obs, mask)[0].astype(int)
    assert not np.array_equal(got, again)                      # a new Philox counter per call
    groups, per = 8, 512
    obs = np.repeat(obs[:groups], per, axis=0)
    mask = np.repeat(mask[:groups], per, axis=0)
    got = e.act_masked(2 * i, obs, mask)[0].astype(int).reshape(groups, per)
    _, p, _ = mm.masked_dist(mo.forward(inp["actors"][i], mo.ACTOR_D, obs[::per], c["trick"])[0], mask[::per])
    for g in range(groups):
        freq = np.bincount(got[g], minlength=A) / per
        se = np.sqrt(p[g] * (1 - p[g]) / per)
        assert (np.abs(freq - p[g]) <= 5 * se).all(), (g, freq, p[g])
        assert np.all(freq[~mask[g * per]] == 0)


def _digest_close(got_flat, want, label, rtol=5e-3, atol=5e-4):
    d = mo.digest(got_flat)
    np.testing.assert_allclose(d[2:], want[2:], rtol=rtol, atol=atol, err_msg=label + " sample")
    tol = rtol * want[1] + atol * np.asarray(got_flat).size
    assert abs(d[0] - want[0]) <= tol and abs(d[1] - want[1]) <= tol, "%s sums %r vs %r" % (label, d[:2], want[:2])


def _policy(c, inp, actor_lr=None, critic_lr=None, trick=None, cont=False):
    from freerl_amd.MAPPO_for_mask_action import MAPPO
    dim_info = {"agent_%d" % i: list(d) for i, d in enumerate(c["dims"])}
    algo = MAPPO(dim_info, cont, c["actor_lr"] if actor_lr is None else actor_lr, c["critic_lr"] if critic_lr is None else critic_lr,
                 c["horizon"], "cuda", trick=dict(c["trick"], **(trick or {})), hidden=c["hidden"])
    if inp is not None:
        _load(algo._e, c, inp)
    return algo


def test_episode_run_follows_the_reference_class(loop_fx):
    """freerl_amd.MAPPO_for_mask_action.MAPPO with rng="host" on the toy environment: four episodes of 13, 9, 16 and 5 steps at horizon 16
    with a learn() after each (a partly filled ring, a stale tail, an exactly full ring, a short episode).  In the reference's run every
    draw's winner leads by >= 1e-3 relative, so the actions are equal; log-probs rtol 1e-4 / atol 1e-6; the final nets' digests at
    tests/test_gpu_mappo_loop.py's 5e-3 / 5e-4"""
    import torch
    c = mm.LOOP
    algo = _policy(c, mm.inputs(c))
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"] + 1000)
    acts, lps = mm.run_loop(algo, mm.ToyEnv(c))
    first_diff = np.argwhere(acts != loop_fx["actions"])
    assert first_diff.size == 0, "first differing (step, agent): %s" % first_diff[:1]
    print("max |logp - reference| %.3g" % np.abs(lps - loop_fx["logp"]).max())
    np.testing.assert_allclose(lps, loop_fx["logp"], rtol=1e-4, atol=1e-6)
    for i in range(len(c["dims"])):
        _digest_close(algo._e.get_params(2 * i), loop_fx["%d/actor/digest" % i], "actor %d" % i)
        _digest_close(algo._e.get_params(2 * i + 1), loop_fx["%d/critic/digest" % i], "critic %d" % i)
        assert algo._e.opt_step(2 * i) == algo._e.opt_step(2 * i + 1) == len(mm.LOOP_EPISODES) * mm.LOOP_HYPER["k_epochs"]


def test_population(N, fx):
    """two learners with different parameters, rows and masks: each equals its single-learner run bit for bit"""
    c = mm.case("tricks")
    inps = [mm.inputs(c), mm.inputs(c, seed=c["seed"] + 500)]
    assert not np.array_equal(inps[0]["rows"][0]["mask"], inps[1]["rows"][0]["mask"])
    perms = np.stack([fx["tricks/perms"], mm.perms(dict(c, seed=c["seed"] + 500))])
    e2, out2 = _run(N, c, inps, perms)
    for p in range(2):
        e1, out1 = _run(N, c, [inps[p]], perms[p][None])
        for k in ("adv", "v_target", "trace"):
            assert np.array_equal(out2[k][p], out1[k][0]), k
        for net in range(e2.n_nets):
            for kind in (0, 2, 3):
                assert np.array_equal(e2.get_params(net, kind, p), e1.get_params(net, kind, 0))
            assert e2.opt_step(net, learner=p) == e1.opt_step(net) == c["k_epochs"]


def test_all_open_agrees_with_the_unmasked_engine(N, fx):
    """every mask open: the masked update against an unmasked FRL_ALGO_MAPPO engine given the same clip_norm, lrs and eps (two kernels,
    two forms of the logarithm: the project's tolerances, not bits)"""
    c = mm.case("plain")
    inp = mm.inputs(c)
    for r in inp["rows"]:
        r["mask"] = np.ones_like(r["mask"])
    perms = fx["plain/perms"][None]
    em, om = _run(N, c, [inp], perms)
    eu, ou = _run(N, c, [inp], perms, masked=False)
    np.testing.assert_allclose(om["adv"], ou["adv"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(om["v_target"], ou["v_target"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(om["trace"], ou["trace"], rtol=1e-4, atol=1e-6)
    for net in range(em.n_nets):
        lr = c["actor_lr"] if net % 2 == 0 else c["critic_lr"]
        mo.assert_net(em.get_params(net), eu.get_params(net), lr, c["k_epochs"], "net %d vs the unmasked engine" % net)
        mo.assert_m(em.get_params(net, 2), eu.get_params(net, 2), "net %d vs the unmasked engine" % net)
    # ... and a closed action makes a difference
    inp["rows"][0]["mask"][:, 1] = inp["rows"][0]["act"][:, 0] == 1
    ec, oc = _run(N, c, [inp], perms)
    assert not np.array_equal(oc["trace"][0, 0], om["trace"][0, 0]) and np.array_equal(oc["trace"][0, 1:, 0, 1], om["trace"][0, 1:, 0, 1])


def _state(e):
    return [e.get_params(net, kind) for net in range(e.n_nets) for kind in (0, 2, 3)] + [e.opt_step(net) for net in range(e.n_nets)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refusals_change_nothing(N, fx):
    c = mm.case("plain")
    inp = mm.inputs(c)
    A0, O0 = c["dims"][0][1], c["dims"][0][0]
    obs, mask = np.zeros((1, 1, O0), F32), np.ones((1, 1, A0), F32)
    for algo, who in ((N.ALGO_IPPO, "IPPO"), (N.ALGO_HAPPO, "HAPPO")):
        e = _engine(N, c, masked=False, algo=algo)
        before = _state(e)
        with pytest.raises(N.FrlError, match="frl_action_mask_set does not serve %s engines" % who):
            e.action_mask_set(True)
        with pytest.raises(N.FrlError, match="frl_act_masked does not serve %s engines" % who):
            e.act_masked(0, obs, mask)
        assert _same(before, _state(e))
        with pytest.raises(N.FrlError, match="extra_cols"):      # the mask blocks belong to FRL_ALGO_MAPPO engines
            _engine(N, c, masked=False, algo=algo, extra_cols=_extra_cols(c, True))
    cont = mm.case("cont")
    e = _engine(N, cont)
    with pytest.raises(N.FrlError, match="continuous"):
        e.action_mask_set(True)
    narrow = _engine(N, c, masked=False)
    _load(narrow, c, inp)
    before = _state(narrow)
    with pytest.raises(N.FrlError, match="mask columns"):
        narrow.action_mask_set(True)
    with pytest.raises(N.FrlError, match="masking is off"):
        narrow.act_masked(0, obs, mask)
    assert _same(before, _state(narrow))
    # a refused switch leaves the engine unmasked: it still takes the unmasked step
    narrow.add_batch(_records(c, inp["rows"], masked=False))
    ref = _engine(N, c, masked=False)
    _load(ref, c, inp)
    ref.add_batch(_records(c, inp["rows"], masked=False))
    assert np.array_equal(_learn(narrow, c, fx["plain/perms"])["trace"], _learn(ref, c, fx["plain/perms"])["trace"])
    wide = _engine(N, c)
    wide.action_mask_set(False)
    with pytest.raises(N.FrlError, match="masking is off"):
        wide.act_masked(0, obs, mask)
    wide.action_mask_set(True)
    with pytest.raises(N.FrlError, match="not an actor"):
        wide.act_masked(1, np.zeros((1, 1, sum(o for o, _ in c["dims"])), F32), np.ones((1, 1, c["dims"][0][1]), F32))
    with pytest.raises(N.FrlError, match="in_dim"):
        wide.act_masked(0, np.zeros((1, 1, O0 + 1), F32), mask)


def _fill(algo, c, inp, count):
    agents = algo.agent_ids
    rows = inp["rows"]
    for t in range(count):
        col = lambda key, sq=False: {a: (rows[i][key][t][0] if sq else rows[i][key][t]) for i, a in enumerate(agents)}
        algo.add(col("obs"), col("act"), col("rew", True), col("next_obs"), col("done", True), col("logp"), col("adv_done", True), col("mask"))


def test_lr_decay_reaches_both_optimisers_and_the_next_learn():
    """lr_decay(1, 2) halves both lrs (MAPPO_for_mask_action.py:389-396); the next learn() is then, to the bit, the learn() of a policy
    built with the halved lrs, and not the undecayed one's"""
    c = mm.LOOP
    inp = mm.inputs(c)

    def after(actor_lr, critic_lr, decay):
        algo = _policy(c, inp, actor_lr, critic_lr, trick=dict(lr_decay=True))
        if decay:
            algo.lr_decay(1, 2)
        a0 = algo.agents["agent_0"]
        lrs = (a0.actor_optimizer.lr, a0.critic_optimizer.lr, algo.agents["agent_2"].critic_optimizer.lr)
        _fill(algo, c, inp, 11)
        np.random.seed(5)
        algo.learn(4, 0.99, 0.95, 0.2, 2, 0.01, 10.0)
        assert algo.buffers["agent_0"]._size == 0
        return lrs, [algo._e.get_params(net) for net in range(algo._e.n_nets)]
    lrs, decayed = after(1e-3, 2e-3, True)
    assert lrs == (5e-4, 1e-3, 1e-3)
    _, direct = after(5e-4, 1e-3, False)
    _, undecayed = after(1e-3, 2e-3, False)
    assert all(np.array_equal(a, b) for a, b in zip(decayed, direct))
    assert all(not np.array_equal(a, b) for a, b in zip(decayed, undecayed))


def test_continuous_policy_stores_masks_and_ignores_them():
    """is_continue=True (MAPPO_for_mask_action.py:250-254, 343-347): Normal(mean, std) as in MAPPO.py; the masks are kept and never read"""
    import torch
    c = mm.case("cont")
    inp = mm.inputs(c)
    outs = []
    for flip in (False, True):
        algo = _policy(dict(c, horizon=16), inp, cont=True)
        torch.manual_seed(3)
        obs = {a: inp["rows"][i]["obs"][0] for i, a in enumerate(algo.agent_ids)}
        avail = {a: inp["rows"][i]["mask"][0] ^ flip for i, a in enumerate(algo.agent_ids)}
        action, logp = algo.select_action(obs, avail)
        assert all(action[a].shape == (c["dims"][i][1],) and logp[a].shape == (c["dims"][i][1],) for i, a in enumerate(algo.agent_ids))
        rows = [dict(r, mask=r["mask"] ^ flip) for r in inp["rows"]]
        _fill(algo, c, dict(inp, rows=rows), 9)
        assert np.array_equal(algo._avail["agent_1"][:9], rows[1]["mask"][:9]) and not algo._avail["agent_1"][9:].any()
        np.random.seed(5)
        algo.learn(4, 0.99, 0.95, 0.2, 2, 0.01, 10.0)
        outs.append([action[a] for a in algo.agent_ids] + [algo._e.get_params(net) for net in range(algo._e.n_nets)])
        assert all(np.isfinite(x).all() for x in outs[-1])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
