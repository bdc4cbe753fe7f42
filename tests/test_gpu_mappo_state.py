"""GPU: MAPPO with a global-state critic (MAPPO_file/MAPPO_for_mask_action_state.py) on kernels_mappo_state.hip, against the
reference's recorded outputs (tests/golden/mappo_state.npz, loop_mappo_state.npz) and the NumPy restatement
(tests/mappo_state_oracle.py), at the smallest shapes at which each part can go wrong: three agents of unequal dims (5, 4), (4, 3),
(5, 6) = 14 observation columns, state widths 1, 2 (a first layer of exactly 16 columns), 3 (17), 7 and 23, hidden 32, horizon 40 in
ONE minibatch (or minibatches of 16 under the SAMPLE pairing: a short last minibatch), K 2; `wide` is 99 columns at hidden 128.

Tolerances are tests/test_gpu_mappo.py's: advantages and value targets rtol 1e-5 / atol 2e-6, losses rtol 1e-4 / atol 1e-6, parameters
and Adam's first moment by tests/mappo_oracle.py's assert_net / assert_m."""
import os

import numpy as np
import pytest

from tests import mappo_oracle as mo
from tests import mappo_state_oracle as ms
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
    return dict(np.load(os.path.join(HERE, "golden", "mappo_state.npz")))


@pytest.fixture(scope="module")
def loop_fx():
    return dict(np.load(os.path.join(HERE, "golden", "loop_mappo_state.npz")))


@pytest.fixture(scope="module")
def runs():
    """the oracle's run of a case (and pairing), computed once and left unchanged"""
    cache = {}

    def get(name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = ms.run(ms.case(name, **kw))
        return cache[key]
    return get


def _base_cols(c, masked=True):
    n, acts = len(c["dims"]), sum(a for _, a in c["dims"])
    if c["cont"]:
        return acts + n
    return 2 * n + (acts if masked else 0)


def _engine(N, c, P=1, masked=True, state=True, algo=None, **kw):
    from freerl_amd.engine import Engine
    sd = c["state_dim"] if state else 0
    args = dict(n_learners=P, discrete=not c["cont"], hidden=c["hidden"], batch_max=c["horizon"], extra_cols=_base_cols(c, masked) + sd, state_dim=sd,
                state_rows=N.STATE_ROWS_SAMPLE if state and c["state_rows"] == "sample" else N.STATE_ROWS_POSITION)
    args.update(kw)
    e = Engine(N.ALGO_MAPPO if algo is None else algo, [o for o, _ in c["dims"]], [a for _, a in c["dims"]], c["horizon"], **args)
    e.net_norm_set(c["trick"]["feature_norm"], c["trick"]["LayerNorm"])
    if masked and not c["cont"]:
        e.action_mask_set(True)
    return e


def _records(c, rows, state=None, masked=True):
    """[log-prob blocks | one adv_done column per agent | one mask block per agent | the state block]"""
    cols = [r["logp"] for r in rows] + [r["adv_done"] for r in rows]
    if masked and not c["cont"]:
        cols += [r["mask"].astype(F32) for r in rows]
    if state is not None:
        cols.append(state[:len(rows[0]["rew"])])
    return records(rows, np.concatenate(cols, axis=1))


def _load(e, c, inp, p=0):
    for i in range(len(c["dims"])):
        e.set_params(2 * i, mo.flat(c, "actor", inp["actors"][i]), learner=p)
        e.set_params(2 * i + 1, mo.flat(c, "critic", inp["critics"][i]), learner=p)


def _hyper(c):
    """what the class passes: two Adams per agent, eps 1e-5 with trick['adam_eps'], clipped at 0.5"""
    t = c["trick"]
    return dict(gamma=c["gamma"], lmbda=c["lmbda"], clip=c["clip"], ent_coef=c["ent_coef"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"],
                adv_norm=t["adv_norm"], value_clip=t["ValueClip"], huber_delta=c["huber_delta"] if t["huber_loss"] else None,
                adam_eps=1e-5 if t["adam_eps"] else 1e-8, clip_norm=0.5)


def _learn(e, c, perms):
    return e.mappo_learn(c["horizon"], c["minibatch"], c["k_epochs"], perms=perms, want_trace=True, want_adv=True, **_hyper(c))


def _add(e, c, sets, count):
    """sets: per learner (rows, state)"""
    P = len(sets)
    e.add_batch(np.concatenate([_records(c, rows, st)[:count] for rows, st in sets]), learners=np.repeat(np.arange(P), count).astype(np.int32))


def _run(N, c, inps, perms, state=True, **kw):
    """the case's learn() calls on one engine for len(inps) learners: rows 0 .. fill-1 added, learn, [the second rows, learn].
    perms [P][calls][n][K][T] -> (engine, the last call's adv / v_target, the calls' traces side by side)"""
    e = _engine(N, c, P=len(inps), state=state, **kw)
    fill = c["horizon"] if c["fill"] is None else c["fill"]
    for p, inp in enumerate(inps):
        _load(e, c, inp, p)
    _add(e, c, [(inp["rows"], inp["state"] if state else None) for inp in inps], fill)
    assert e.cursor(0) == (fill % c["horizon"], fill)
    out = _learn(e, c, perms[:, 0])
    traces = [out["trace"]]
    assert e.cursor(0) == (0, 0)                    # Buffer_for_PPO_state_mask.clear: counters only
    if c["second"]:
        _add(e, c, [ms.second_rows(c) if state else (ms.second_rows(c)[0], None) for _ in inps], c["second"])
        out = _learn(e, c, perms[:, 1])
        traces.append(out["trace"])
    out["trace"] = np.concatenate(traces, axis=2)
    return e, out


def _check_against(e, c, o, out, fx=None, name=None, p=0):
    n = len(c["dims"])
    steps = o.aopt[0].t
    print("%s: first critic losses kernel %s oracle %s" % (name, out["trace"][p, :, 0, 1], o.trace[:, 0, 1]))
    wants = dict(adv=[(o.adv_raw, "oracle")], v_target=[(o.v_target, "oracle")], trace=[(o.trace, "oracle")])
    if fx is not None:
        for k in wants:
            wants[k].insert(0, (fx["%s/%s" % (name, k)], "reference"))
    for want, who in wants["adv"]:
        np.testing.assert_allclose(out["adv"][p], want, rtol=1e-5, atol=2e-6, err_msg="adv vs " + who)
    for want, who in wants["v_target"]:
        np.testing.assert_allclose(out["v_target"][p], want, rtol=1e-5, atol=2e-6, err_msg="v_target vs " + who)
    for want, who in wants["trace"]:
        np.testing.assert_allclose(out["trace"][p], want, rtol=1e-4, atol=1e-6, err_msg="loss trace vs " + who)
    for i in range(n):
        for net, tag, want, opt, lr in ((2 * i, "actor", o.actors[i], o.aopt[i], c["actor_lr"]), (2 * i + 1, "critic", o.critics[i], o.copt[i], c["critic_lr"])):
            key = "%s/%d/%s" % (name, i, tag)
            got = e.get_params(net, 0, p)
            if fx is not None and key + "/p" in fx:
                mo.assert_net(got, fx[key + "/p"], lr, steps, key + " vs reference")
            if fx is not None:
                assert steps == int(fx[key + "/step"])
            mo.assert_net(got, mo.flat(c, tag, want), lr, steps, key + " vs oracle")
            mo.assert_m(e.get_params(net, 2, p), mo.flat(c, tag, opt.m), key)
            assert e.opt_step(net, learner=p) == steps
            assert e.pad_max(net, 0, p) == 0.0


@pytest.mark.parametrize("name", list(ms.CASES))
def test_golden_and_oracle(N, fx, runs, name):
    """plain / tricks (the input LayerNorm over both segments) / partial (13 rows never written: zero state) / stale (a second learn over 18
    new and 22 old rows and states) / cont / wide (99 columns, hidden 128) / state widths 1, 2, 3 and 23 on 14 observation columns"""
    c = ms.case(name)
    e, out = _run(N, c, [ms.inputs(c)], fx[name + "/perms"][None])
    assert e.state_info() == (c["state_dim"], e.layout.extra_off + e.layout.extra - c["state_dim"])
    assert e.num_params(1) == c["hidden"] * (ms.critic_width(c) + 1) + c["hidden"] * (c["hidden"] + 1) + c["hidden"] + 1
    # neither the other pairing's first critic loss nor the one without the state block (recorded by the maker: > 1e-3 away)
    for other in (fx[name + "/first_critic_loss_sample"], fx[name + "/first_critic_loss_zero_state"]):
        assert (np.abs(out["trace"][0, :, 0, 1] - other) > 5e-4 * np.abs(other)).all()
    _check_against(e, c, runs(name), out, fx, name)


@pytest.mark.parametrize("name,minibatch", [("plain", 40), ("tricks", 16), ("stale", 16), ("cont", 16), ("sd3", 16), ("sd23", 40)])
def test_sample_pairing_against_the_oracle(N, fx, runs, name, minibatch):
    """FRL_STATE_ROWS_SAMPLE: [obs[perm[r]] | state[perm[r]]]; minibatches of 16 on a horizon of 40 are a short last minibatch (8 rows) and
    a short last row chunk"""
    c = ms.case(name, state_rows="sample", minibatch=minibatch)
    e, out = _run(N, c, [ms.inputs(c)], fx[name + "/perms"][None])
    n_mb = -(-c["horizon"] // minibatch)
    assert out["trace"].shape == (1, 3, c["k_epochs"] * n_mb * ms.calls(c), 2)
    _check_against(e, c, runs(name, state_rows="sample", minibatch=minibatch), out, name=name)
    if minibatch == c["horizon"]:      # the reference's pairing is another computation
        assert (np.abs(out["trace"][0, :, 0, 1] - fx[name + "/trace"][:, 0, 1]) > 5e-4 * np.abs(fx[name + "/trace"][:, 0, 1])).all()


def _state(e, p=0):
    return [e.get_params(net, kind, p) for net in range(e.n_nets) for kind in (0, 2, 3)] + [e.opt_step(net, learner=p) for net in range(e.n_nets)]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["tricks", "sd3"])
def test_pairings_give_identical_bits_where_they_must(N, fx, name):
    """injected identity permutations: row r is ring row r under both pairings; random permutations with ONE state vector in every row:
    the state read is the same whichever row it comes from.  And with the case's own rows and permutations they differ.  `sd3` puts the
    straight copy and the gather side by side at the tile edge (17 columns)."""
    c = ms.case(name)
    inp = ms.inputs(c)
    perms = fx[name + "/perms"][None]
    ident = np.broadcast_to(np.arange(c["horizon"]), perms.shape).copy()
    same_state = dict(inp, state=np.tile(inp["state"][:1], (c["horizon"], 1)))
    for inp_k, perm_k in ((inp, ident), (same_state, perms)):
        got = []
        for rows in ("position", "sample"):
            e, out = _run(N, dict(c, state_rows=rows), [inp_k], perm_k)
            got.append(_state(e) + [out["adv"], out["v_target"], out["trace"]])
        assert _same(got[0], got[1])
    ep, op = _run(N, c, [inp], perms)
    es, os_ = _run(N, dict(c, state_rows="sample"), [inp], perms)
    assert np.array_equal(op["v_target"], os_["v_target"]) and not np.array_equal(op["trace"][..., 1], os_["trace"][..., 1])
    assert np.array_equal(op["trace"][0, :, 0, 0], os_["trace"][0, :, 0, 0])      # the actors' first step does not see the state


@pytest.mark.parametrize("name", ["plain", "sd2", "sd3"])
def test_zero_state_columns_reproduce_the_masked_engine(N, fx, name):
    """feature_norm off and the state columns of every critic's first layer zero: the state engine on the same rows is the masked engine
    without a state whose critics are the observation columns of the same layers (a wrong column offset would not be).  One epoch, so one
    step per net: the first step moves the state columns off zero, and the engines part from the second step on"""
    c = ms.case(name, k_epochs=1)
    c["trick"] = dict(c["trick"], feature_norm=False)      # (the input LayerNorm would see the state through the row's mean and variance)
    inp = ms.inputs(c)
    ot = sum(o for o, _ in c["dims"])
    for p in inp["critics"]:
        p["l1.weight"][:, ot:] = 0
    narrow = dict(inp, critics=[dict(p, **{"l1.weight": p["l1.weight"][:, :ot].copy()}) for p in inp["critics"]])
    perms = fx[name + "/perms"][None, :, :, :1]
    es, outs = _run(N, c, [inp], perms)
    em, outm = _run(N, c, [narrow], perms, state=False)
    assert em.state_info() == (0, 0) and es.num_params(1) > em.num_params(1)
    np.testing.assert_allclose(outs["adv"], outm["adv"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(outs["v_target"], outm["v_target"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(outs["trace"], outm["trace"], rtol=1e-4, atol=1e-6)
    H, steps = c["hidden"], c["k_epochs"]
    for i in range(len(c["dims"])):
        mo.assert_net(es.get_params(2 * i), em.get_params(2 * i), c["actor_lr"], steps, "actor %d vs the masked engine" % i)
        w = ms.critic_width(c)
        gs, gm = es.get_params(2 * i + 1), em.get_params(2 * i + 1)
        l1s, l1m = gs[:H * w].reshape(H, w), gm[:H * ot].reshape(H, ot)
        mo.assert_net(np.concatenate([l1s[:, :ot].reshape(-1), gs[H * w:]]), np.concatenate([l1m.reshape(-1), gm[H * ot:]]), c["critic_lr"], steps,
                      "critic %d vs the masked engine" % i)
        assert np.abs(l1s[:, ot:]).max() > 0      # the state columns take gradient all the same


def test_act_raw_on_a_state_critic_takes_both_segments(N):
    """frl_act with FRL_ACT_RAW on nets 2i+1 of a state engine: rows [obs_0 .. obs_{n-1} | state] through the update's normalised forward;
    a row of the observations' width alone is refused"""
    for name in ("tricks", "sd3", "sd2"):
        c = ms.case(name)
        inp = ms.inputs(c)
        e = _engine(N, c)
        _load(e, c, inp)
        rows = np.concatenate([r["obs"] for r in inp["rows"]] + [inp["state"]], axis=1)
        assert rows.shape[1] == ms.critic_width(c)
        for i in range(len(c["dims"])):
            got = e.act(2 * i + 1, N.ACT_RAW, rows, out_dim=1)[0, :, 0]
            np.testing.assert_allclose(got, mo.value(inp["critics"][i], rows, c["trick"])[:, 0], rtol=2e-5, atol=2e-6)      # tests/test_gpu_mappo.py's
        with pytest.raises(N.FrlError, match="in_dim"):
            e.act(1, N.ACT_RAW, rows[:, :14], out_dim=1)


def test_population(N, fx):
    """three learners with different parameters, rows and states: each equals its single-learner run bit for bit"""
    c = ms.case("tricks")
    seeds = [c["seed"], c["seed"] + 500, c["seed"] + 700]
    inps = [ms.inputs(c, seed=s) for s in seeds]
    assert not np.array_equal(inps[0]["state"], inps[1]["state"]) and not np.array_equal(inps[1]["state"], inps[2]["state"])
    perms = np.stack([fx["tricks/perms"]] + [ms.perms(dict(c, seed=s)) for s in seeds[1:]])
    e3, out3 = _run(N, c, inps, perms)
    for p in range(3):
        e1, out1 = _run(N, c, [inps[p]], perms[p][None])
        for k in ("adv", "v_target", "trace"):
            assert np.array_equal(out3[k][p], out1[k][0]), k
        assert _same(_state(e3, p), _state(e1))
        assert e3.opt_step(1, learner=p) == c["k_epochs"]


def test_refusals_change_nothing(N, fx):
    from freerl_amd.engine import Engine
    c = ms.case("plain")
    inp = ms.inputs(c)
    sd = c["state_dim"]
    obs, acts = [o for o, _ in c["dims"]], [a for _, a in c["dims"]]
    # a state on anything but FRL_ALGO_MAPPO
    for algo in (N.ALGO_IPPO, N.ALGO_HAPPO):
        with pytest.raises(N.FrlError, match="FRL_ALGO_MAPPO"):
            _engine(N, c, masked=False, algo=algo)
    with pytest.raises(N.FrlError, match="FRL_ALGO_MAPPO"):
        Engine(N.ALGO_TD3, 5, 3, 64, twin_critic=True, state_dim=sd)
    # extra_cols that cannot hold the block; a bad state_rows; a bad size
    with pytest.raises(N.FrlError, match="state columns"):
        _engine(N, c, extra_cols=_base_cols(c) + sd - 1)
    with pytest.raises(N.FrlError, match="state columns"):
        _engine(N, c, masked=False, extra_cols=_base_cols(c, False))
    with pytest.raises(N.FrlError, match="state_rows 2"):
        _engine(N, c, state_rows=2)
    with pytest.raises(N.FrlError, match="state_dim -1"):
        _engine(N, c, state_dim=-1)
    with pytest.raises(ValueError, match="without a state_dim"):      # (the binding's own: the library would ignore the pairing)
        _engine(N, c, state=False, state_rows=N.STATE_ROWS_SAMPLE)
    import ctypes as C
    cfg = _engine(N, c).cfg
    h = C.c_void_p()
    assert N.lib().frl_create_ex(C.byref(cfg), C.byref(N.ConfigExt(16, sd, 0)), C.byref(h)) == 1 and not h.value
    assert b"frl_config_ext.size 16" in N.lib().frl_last_error()
    # a state width that trips the LDS limit is named
    with pytest.raises(N.FrlError, match=r"160 KB \(a first layer of \d+ input columns, 4000 of them the state's"):
        _engine(N, c, state_dim=4000, extra_cols=_base_cols(c) + 4000)
    # ext == NULL and state_dim == 0 build the engine without a state
    e0 = _engine(N, c, state=False)
    assert e0.state_info() == (0, 0) and e0.num_params(1) == c["hidden"] * (14 + 1) + c["hidden"] * (c["hidden"] + 1) + c["hidden"] + 1
    assert N.lib().frl_create_ex(C.byref(e0.cfg), C.byref(N.ConfigExt(12, 0, 1)), C.byref(h)) == 0
    sdim, scol = C.c_int(-1), C.c_int(-1)
    assert N.lib().frl_state_info(h, C.byref(sdim), C.byref(scol)) == 0 and (sdim.value, scol.value) == (0, 0)
    N.lib().frl_destroy(h)
    # frl_action_mask_set without room for the mask blocks in front of the state block
    tight = _engine(N, c, masked=False)
    _load(tight, c, inp)
    before = _state(tight)
    with pytest.raises(N.FrlError, match="mask columns"):
        tight.action_mask_set(True)
    roomy = _engine(N, c, masked=False, state_dim=sum(acts), extra_cols=_base_cols(c, False) + sum(acts))      # room for the mask blocks, all of it state
    with pytest.raises(N.FrlError, match=r"\+ 13 state columns"):
        roomy.action_mask_set(True)
    assert _same(before, _state(tight))
    # minibatch != horizon under POSITION; any minibatch under SAMPLE
    e = _engine(N, c)
    _load(e, c, inp)
    _add(e, c, [(inp["rows"], inp["state"])], c["horizon"])
    before = _state(e)
    with pytest.raises(N.FrlError, match="FRL_STATE_ROWS_POSITION"):
        _learn(e, dict(c, minibatch=16), fx["plain/perms"])
    assert _same(before, _state(e)) and e.cursor(0) == (0, c["horizon"])
    # ... and the refused engine still takes the case's step
    ref, out_ref = _run(N, c, [inp], fx["plain/perms"][None])
    assert np.array_equal(_learn(e, c, fx["plain/perms"])["trace"], out_ref["trace"]) and _same(_state(e), _state(ref))
    assert len(obs) == 3


# ------------------------------------------------------------------------------------------------ the class
def _policy(c, inp, state_dim="case", cont=False, trick=None, actor_lr=None, critic_lr=None, **kw):
    from freerl_amd.MAPPO_for_mask_action_state import MAPPO
    dim_info = {"agent_%d" % i: list(d) for i, d in enumerate(c["dims"])}
    algo = MAPPO(dim_info, cont, c["actor_lr"] if actor_lr is None else actor_lr, c["critic_lr"] if critic_lr is None else critic_lr, c["horizon"], "cuda",
                 dict(c["trick"], **(trick or {})), c["state_dim"] if state_dim == "case" else state_dim, hidden=c["hidden"], **kw)
    if inp is not None:
        _load(algo._e, c, inp)
    return algo


def _fill(algo, rows, state, count, with_state=True):
    agents = algo.agent_ids
    for t in range(count):
        col = lambda key, sq=False: {a: (rows[i][key][t][0] if sq else rows[i][key][t]) for i, a in enumerate(agents)}
        args = (col("obs"), col("act"), col("rew", True), col("next_obs"), col("done", True), col("logp"), col("adv_done", True), col("mask"))
        algo.add(*(args + ((state[t],) if with_state else ())))


def test_class_follows_the_engine_and_keeps_stale_states(N, fx, runs):
    """the class on the `stale` case: add / learn / add 18 rows / learn is the engine's run bit for bit, so rows 18 .. 39 kept their old
    states; with state_rows="sample" it is the other pairing's"""
    c = ms.case("stale")
    inp = ms.inputs(c)
    second, second_state = ms.second_rows(c)
    for rows in ("position", "sample"):
        ck = dict(c, state_rows=rows)
        algo = _policy(ck, inp, state_rows=rows)
        assert algo.state_dim == c["state_dim"] and algo._e.state_info()[0] == c["state_dim"]
        algo.track_loss = True
        np.random.seed(c["seed"] + 1000)
        _fill(algo, inp["rows"], inp["state"], c["horizon"])
        algo.learn(7, c["gamma"], c["lmbda"], c["clip"], c["k_epochs"], c["ent_coef"], c["huber_delta"])
        _fill(algo, second, second_state, c["second"])
        algo._e.flush()
        ring = algo._e.read_rows(0, 0, c["horizon"])
        col = algo._e.state_info()[1]
        assert np.array_equal(ring[:18, col:col + 7], second_state) and np.array_equal(ring[18:, col:col + 7], inp["state"][18:])
        algo.learn(7, c["gamma"], c["lmbda"], c["clip"], c["k_epochs"], c["ent_coef"], c["huber_delta"])
        e, out = _run(N, ck, [inp], fx["stale/perms"][None])
        assert _same(_state(algo._e), _state(e))
        assert np.array_equal(algo.last_trace, out["trace"][:, :, c["k_epochs"]:])
    _check_against(e, ck, runs("stale", state_rows="sample"), out, name="stale")


def test_class_edges():
    """state_dim=None: built and filled like the masked class, learn() raises ValueError (the reference's 9-way unpack); a state_dim with
    state=None or a state of another length: ValueError, nothing added"""
    c = ms.case("plain")
    inp = ms.inputs(c)
    narrow = dict(inp, critics=[dict(p, **{"l1.weight": p["l1.weight"][:, :14].copy()}) for p in inp["critics"]])
    algo = _policy(c, narrow, state_dim=None)
    assert algo.state_dim is None and algo._e.state_info() == (0, 0)
    _fill(algo, inp["rows"], inp["state"], 5)
    _fill(algo, inp["rows"], inp["state"], 2, with_state=False)
    assert algo.buffers["agent_0"]._size == 7
    before = _state(algo._e)
    with pytest.raises(ValueError, match="expected 9, got 8"):
        algo.learn(7, 0.99, 0.95, 0.2, 2, 0.01, 10.0)
    assert _same(before, _state(algo._e)) and algo.buffers["agent_0"]._size == 7
    algo = _policy(c, inp)
    with pytest.raises(ValueError, match="state of no values"):
        _fill(algo, inp["rows"], inp["state"], 1, with_state=False)
    with pytest.raises(ValueError, match="state of 6 values"):
        _fill(algo, inp["rows"], inp["state"][:, :6], 1)
    assert algo.buffers["agent_0"]._size == 0
    with pytest.raises(ValueError, match="state_rows"):
        _policy(c, None, state_rows="row")


def test_continuous_policy_ignores_masks_and_uses_the_state():
    import torch
    c = ms.case("cont")
    inp = ms.inputs(c)
    outs = []
    for flip, scale in ((False, 1.0), (True, 1.0), (False, 0.5)):
        algo = _policy(dict(c, horizon=16), inp, cont=True)
        torch.manual_seed(3)
        rows = [dict(r, mask=r["mask"] ^ flip) for r in inp["rows"]]
        _fill(algo, rows, inp["state"] * F32(scale), 9)
        assert np.array_equal(algo._avail["agent_1"][:9], rows[1]["mask"][:9])
        np.random.seed(5)
        algo.learn(4, 0.99, 0.95, 0.2, 2, 0.01, 10.0)
        outs.append([algo._e.get_params(net) for net in range(algo._e.n_nets)])
        assert all(np.isfinite(x).all() for x in outs[-1])
    assert _same(outs[0], outs[1])                                       # the masks are never read
    assert not np.array_equal(outs[0][1], outs[2][1])                    # the state is


def test_lr_decay_reaches_the_next_learn():
    c = ms.LOOP
    inp = ms.inputs(c)

    def after(actor_lr, critic_lr, decay):
        algo = _policy(c, inp, actor_lr=actor_lr, critic_lr=critic_lr, trick=dict(lr_decay=True))
        if decay:
            algo.lr_decay(1, 2)
        _fill(algo, inp["rows"], inp["state"], 11)
        np.random.seed(5)
        algo.learn(4, 0.99, 0.95, 0.2, 2, 0.01, 10.0)
        return [algo._e.get_params(net) for net in range(algo._e.n_nets)]
    decayed, direct, undecayed = after(1e-3, 2e-3, True), after(5e-4, 1e-3, False), after(1e-3, 2e-3, False)
    assert _same(decayed, direct) and all(not np.array_equal(a, b) for a, b in zip(decayed, undecayed))


def _digest_close(got_flat, want, label, rtol=5e-3, atol=5e-4):
    d = mo.digest(got_flat)
    np.testing.assert_allclose(d[2:], want[2:], rtol=rtol, atol=atol, err_msg=label + " sample")
    tol = rtol * want[1] + atol * np.asarray(got_flat).size
    assert abs(d[0] - want[0]) <= tol and abs(d[1] - want[1]) <= tol, "%s sums %r vs %r" % (label, d[:2], want[:2])


def test_episode_run_follows_the_reference_class(loop_fx):
    """the class with rng="host" on the toy environment with a get_state(): four episodes of 13, 9, 16 and 5 steps at horizon 16 with a
    learn() after each, by tests/test_gpu_mappo_mask.py's rules: in the reference's run every draw's winner leads by >= 1e-3 relative,
    so the actions are equal; log-probs rtol 1e-4 / atol 1e-6; the final nets' digests at 5e-3 / 5e-4"""
    import torch
    c = ms.LOOP
    algo = _policy(c, ms.inputs(c))
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"] + 1000)
    acts, lps = ms.run_loop(algo, ms.ToyEnv(c))
    first_diff = np.argwhere(acts != loop_fx["actions"])
    assert first_diff.size == 0, "first differing (step, agent): %s" % first_diff[:1]
    print("max |logp - reference| %.3g" % np.abs(lps - loop_fx["logp"]).max())
    np.testing.assert_allclose(lps, loop_fx["logp"], rtol=1e-4, atol=1e-6)
    for i in range(len(c["dims"])):
        _digest_close(algo._e.get_params(2 * i), loop_fx["%d/actor/digest" % i], "actor %d" % i)
        _digest_close(algo._e.get_params(2 * i + 1), loop_fx["%d/critic/digest" % i], "critic %d" % i)
        assert algo._e.opt_step(2 * i) == algo._e.opt_step(2 * i + 1) == len(ms.LOOP_EPISODES) * ms.LOOP_HYPER["k_epochs"]
