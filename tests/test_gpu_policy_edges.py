"""SAC's and TD3's policy arithmetic (device/policy.hpp) at its clamp and clip edges, on every kernel family that runs it, against the
float64 reference of tests/policy_edge_cases.py on the same seeded inputs: log_std columns exactly on and past the clamp's bounds (the
gate closed: bit-unchanged, Adam moments exactly 0; the gate open on the closed bound: moved, and equal to the reference), across the
head tile's seam, a target actor whose log_std differs from the online one, alpha 0.2 so that the log-prob carries weight, means that
saturate tanh and take softplus's threshold branch, TD3's smoothing with two fifths of the noise and a fifth of the target actions
clipped, done rows in every batch; a population of three learners with a layout each.

Families (asserted with learn_path before the first call): row-chunk (kernels_critic / _actor), narrow chained (kernels_critic2 /
_actor2), K-sliced (kernels_criticw / _actorw), hidden-256 x-stationary (kernels_criticx / _actorx), kernels_solo, kernels_solow.

Tolerances are tests/test_gpu_parity.py's, unchanged: losses rtol 1e-4 (actor: atol 2e-6 too), alpha rtol 1e-5, every parameter of actor,
critic and both targets rtol 5e-4 / atol 5e-6 on all elements, Adam step counts equal; select_action rtol 5e-4 / atol 5e-5, tanh heads
rtol 1e-5 / atol 1e-6.  Every test asserts the conditions on its inputs (policy_edge_cases.assert_conditions: the float32 oracle within
a quarter of each tolerance of float64, hidden units off ReLU's kink, the clip populations, the bound columns' first step) before it
creates an engine.  Each (case, family) pair runs once, on one engine with 3 (SAC) or 4 (TD3) learn calls; the tests share that run.

Measured on an MI355X, as the part of each tolerance used against float64, worst case per family (losses / alpha / parameters / forward
checks): row-chunk 0.004 / 0.010 / 0.42 / 0.22, narrow chained 0.014 / 0.008 / 0.14 / 0.30, kernels_solo 0.014 / 0.008 / 0.15 / 0.30,
K-sliced 0.003 / 0.010 / 0.02 / 0.22, kernels_solow 0.003 / 0.010 / 0.03 / 0.22, x-stationary 0.002 / 0.008 / 0.58 / 0.13 (the
parameters' 0.42 and 0.58 are td3-h256-b17, where the float32 oracle is at 0.15; the next largest is 0.17).  The padding assertion
found kernels_solow.hip summing slab slots that no pass had written; everything else passed as the kernels stood."""
import numpy as np
import pytest

from tests import policy_edge_cases as pc
from tests.hip_helpers import flat_params, records, unflat_params

pytestmark = pytest.mark.gpu

F32 = np.float32
KNOBS = ("FRL_CRITIC_V2", "FRL_SOLO", "FRL_SOLOW", "FRL_SOLOW_NARROW", "FRL_SOLOW_FUSE", "FRL_SOLO_PREDRAW", "FRL_SOLO_MAXP", "FRL_SOLOW_HELPERS")
NETS = ("actor", "critic", "actor_t", "critic_t")


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


# ------------------------------------------------------------------------------------------------ engine side
def actor_flat(c, p):
    return flat_params(p, pc.ACTOR_NAMES[c["algo"]], "log_std" if c["algo"] == "sac" else None)


def actor_unflat(c, flat, like):
    return unflat_params(flat, like, pc.ACTOR_NAMES[c["algo"]], "log_std" if c["algo"] == "sac" else None)


def make_engine(N, c, v2, monkeypatch, n_learners=1):
    from freerl_amd.engine import Engine
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if v2 is not None:
        monkeypatch.setenv("FRL_CRITIC_V2", v2)
    return Engine(N.ALGO_SAC if c["algo"] == "sac" else N.ALGO_TD3, c["O"], c["A"], pc.N_TABLE, n_learners=n_learners, twin_critic=True,
                  batch_max=pc.BATCH_MAX, hidden=c["H"])


def load(N, e, c, learner=0):
    sp = pc.spec(c["name"])
    for kind, a, q in ((N.PARAM_ONLINE, "actor", "critic"), (N.PARAM_TARGET, "actor_t", "critic_t")):
        e.set_params(0, actor_flat(c, sp[a]), kind, learner=learner)
        e.set_params(1, flat_params(sp[q], pc.CRITIC_NAMES), kind, learner=learner)
    if c["algo"] == "sac":
        e.set_alpha_state([np.log(pc.ALPHA0), 0, 0, pc.ALPHA0], 0, learner)
    recs = records([sp["table"]])
    e.add_batch(recs, learners=np.full(len(recs), learner, np.int32))


def learn_call(N, e, cs, k):
    """Call k of every learner's case (same algorithm, shape and batch): [P, 1, FRL_STAT_COUNT] stats."""
    c, B, A = cs[0], cs[0]["batch"], cs[0]["A"]
    sps = [pc.spec(x["name"]) for x in cs]
    idx = np.stack([sp["idx"][k] for sp in sps])
    nz = np.zeros((len(cs), 1, 2, B, A), F32)
    for p, sp in enumerate(sps):
        for j, n in enumerate(sp["noise"][k]):
            nz[p, 0, j] = n
    h = sps[0]["hyper"]
    kw = dict(gamma=h["gamma"], tau=h["tau"], actor_lr=h["actor_lr"], critic_lr=h["critic_lr"])
    if c["algo"] == "sac":
        kw.update(alpha_lr=h["alpha_lr"], target_entropy=h["target_entropy"])
    else:
        kw.update(do_actor=(k + 1) % h["policy_freq"] == 0, use_policy_noise=True, policy_noise=h["policy_noise"], noise_clip=h["noise_clip"],
                  max_action=h["max_action"], policy_noise_scale=h["policy_noise_scale"])
    return e.learn(B, idx=idx, noise=nz, want_stats=True, **kw)


def snapshot(N, e, c, learner=0):
    """The online actor's log_std and its Adam moments (SAC) after a call."""
    if c["algo"] != "sac":
        return {}
    A = c["A"]
    return {name: e.get_params(0, kind, learner=learner)[-A:].copy() for name, kind in
            (("log_std", N.PARAM_ONLINE), ("m", N.PARAM_ADAM_M), ("v", N.PARAM_ADAM_V))}


def final_state(N, e, c, learner=0):
    like = pc.reference_run(c["name"])["calls"][-1]
    out = dict(actor=actor_unflat(c, e.get_params(0, N.PARAM_ONLINE, learner=learner), like["actor"]),
               actor_t=actor_unflat(c, e.get_params(0, N.PARAM_TARGET, learner=learner), like["actor_t"]),
               critic=unflat_params(e.get_params(1, N.PARAM_ONLINE, learner=learner), like["critic"], pc.CRITIC_NAMES),
               critic_t=unflat_params(e.get_params(1, N.PARAM_TARGET, learner=learner), like["critic_t"], pc.CRITIC_NAMES))
    out["steps"] = (e.opt_step(0, learner), e.opt_step(1, learner))
    out["pads"] = {"%s/net%d" % (nm, net): e.pad_max(net, kind, learner=learner) for net in (0, 1) for kind, nm in
                   ((N.PARAM_ONLINE, "theta"), (N.PARAM_TARGET, "target"), (N.PARAM_ADAM_M, "m"), (N.PARAM_ADAM_V, "v"))}
    if c["algo"] == "sac":
        out["alpha_state"] = e.alpha_state(learner)
    return out


def stats_of(N, c, per_call, learner=0):
    st = np.stack(per_call)[:, learner, 0]
    h = pc.spec(c["name"])["hyper"]
    out = dict(critic_loss=st[:, N.STAT_CRITIC_LOSS].astype(np.float64))
    if c["algo"] == "sac":
        out.update(actor_loss=st[:, N.STAT_ACTOR_LOSS].astype(np.float64), alpha_loss=st[:, N.STAT_ALPHA_LOSS].astype(np.float64),
                   alpha=st[:, N.STAT_ALPHA].astype(np.float64))
    else:
        out["actor_loss"] = st[h["policy_freq"] - 1::h["policy_freq"], N.STAT_ACTOR_LOSS].astype(np.float64)
    return out


_RUNS = {}
_STOP = []          # the first error that was no assertion (a HIP error, say): nothing more of this module is started on the device after it


def engine_run(N, c, family, monkeypatch):
    """The case on a fresh engine of the family: the forward checks on the parameters as set, then the learn calls.  Kept for the tests
    that share it; a run that raised is not started again."""
    key = (c["name"], family)
    if key not in _RUNS and _STOP:
        raise RuntimeError("not started: an earlier run of this module ended with %r" % (_STOP[0],))
    if key not in _RUNS:
        _RUNS[key] = RuntimeError("%s on %s did not finish" % key)
        try:
            pc.assert_conditions(c)
            e = make_engine(N, c, pc.SHAPES[c["shape"]]["families"][family], monkeypatch)
            try:
                path = e.learn_path(c["batch"])
                assert pc.path_is(family, path, c["batch"]), "%s: frl_learn_path %r is not the %s family" % (c["name"], path, family)
                load(N, e, c)
                obs = pc.act_inputs(c["name"])[0]
                acts = {}
                for label, eps, target, _ in pc.act_checks(c):
                    acts[label] = e.act(0, N.ACT_SAC_SAMPLE if eps is not None else N.ACT_TANHHEAD, obs, eps=eps, use_target=target, out_dim=c["A"])[0].copy()
                per_call, snaps = [], []
                for k in range(c["n_calls"]):
                    per_call.append(learn_call(N, e, [c], k).copy())
                    snaps.append(snapshot(N, e, c))
                out = dict(final_state(N, e, c), path=path, acts=acts, snaps=snaps, **stats_of(N, c, per_call))
            finally:
                e.close()
            _RUNS[key] = out
        except BaseException as ex:
            _RUNS[key] = ex
            if not isinstance(ex, AssertionError):
                _STOP.append(ex)
            raise
    if isinstance(_RUNS[key], BaseException):
        raise _RUNS[key]
    return _RUNS[key]


# ------------------------------------------------------------------------------------------------ assertions
def assert_learner(c, got, label):
    """Losses, alpha, every parameter of the four sets, step counts and padding of one learner against its float64 reference."""
    ref = pc.reference_run(c["name"])
    np.testing.assert_allclose(got["critic_loss"], ref["critic_loss"], rtol=pc.LOSS_RTOL, err_msg=label + " critic loss")
    np.testing.assert_allclose(got["actor_loss"], ref["actor_loss"], rtol=pc.LOSS_RTOL, atol=pc.ACTOR_LOSS_ATOL, err_msg=label + " actor loss")
    if c["algo"] == "sac":
        np.testing.assert_allclose(got["alpha_loss"], ref["alpha_loss"], rtol=pc.LOSS_RTOL, err_msg=label + " alpha loss")
        np.testing.assert_allclose(got["alpha"], ref["alpha"], rtol=pc.ALPHA_RTOL, err_msg=label + " alpha")
        vals, t = got["alpha_state"]
        np.testing.assert_allclose(vals[3], ref["alpha"][-1], rtol=pc.ALPHA_RTOL, err_msg=label + " alpha state")
        assert t == c["n_calls"], label
    last = ref["calls"][-1]
    for net in NETS:
        for k, want in last[net].items():
            np.testing.assert_allclose(got[net][k], want, rtol=pc.P_RTOL, atol=pc.P_ATOL, err_msg="%s %s %s" % (label, net, k))
    assert got["steps"] == ref["steps"], (label, got["steps"], ref["steps"])
    bad = {k: v for k, v in got["pads"].items() if v != 0.0}
    assert not bad, "%s: padding slots moved away from zero: %r" % (label, bad)


def assert_gate(c, snaps, label):
    """The clamp's gradient gate of one SAC learner, after every call."""
    name = c["name"]
    ref, raw = pc.reference_run(name), pc.spec(name)["actor"]["log_std"].reshape(-1)
    closed, on_bound = pc.gate_columns(name)
    for k, s in enumerate(snaps):
        where = "%s call %d" % (label, k)
        # closed: nothing of it may ever change — compared as bits
        np.testing.assert_array_equal(s["log_std"][closed].view(np.uint32), raw[closed].view(np.uint32), err_msg=where + ": a gated log_std column moved")
        assert not s["m"][closed].any() and not s["v"][closed].any(), (where, "Adam moments of a gated column", s["m"][closed], s["v"][closed])
        # open on the closed bound: it moves, by Adam's first step of lr (1 - eps / |g|) in the first call, and follows the reference
        assert (s["log_std"][on_bound] != raw[on_bound]).all(), (where, "a column exactly on the bound did not move", s["log_std"][on_bound])
        assert s["m"][on_bound].all() and s["v"][on_bound].all(), (where, "Adam moments of a column on the bound", s["m"][on_bound])
        want = ref["calls"][k]["actor"]["log_std"].reshape(-1)
        np.testing.assert_allclose(s["log_std"], want, rtol=pc.P_RTOL, atol=pc.P_ATOL, err_msg=where + " log_std")
        np.testing.assert_array_equal(np.sign(s["m"][on_bound]), np.sign(ref["calls"][k]["actor_m"]["log_std"].reshape(-1)[on_bound]), err_msg=where + " sign of Adam's m")
    step = (snaps[0]["log_std"].astype(np.float64) - raw)[on_bound]
    want = (ref["calls"][0]["actor"]["log_std"].reshape(-1) - raw)[on_bound]
    assert ((np.abs(step) >= 0.5 * pc.LR) & (np.abs(step) <= 1.5 * pc.LR) & (np.sign(step) == np.sign(want))).all(), (label, "first step of the bound columns", step, want)


pair_id = lambda p: "%s-%s" % (p[0]["name"], p[1])


@pytest.mark.parametrize("pair", pc.PAIRS, ids=pair_id)
def test_family_against_the_float64_reference(N, pair, monkeypatch):
    c, family = pair
    got = engine_run(N, c, family, monkeypatch)
    assert pc.path_is(family, got["path"], c["batch"]), (got["path"], family)
    assert_learner(c, got, pair_id(pair))


@pytest.mark.parametrize("pair", pc.SAC_PAIRS, ids=pair_id)
def test_log_std_gate_closed_past_the_bounds_open_on_them(N, pair, monkeypatch):
    c, family = pair
    got = engine_run(N, c, family, monkeypatch)
    assert_gate(c, got["snaps"], pair_id(pair))
    # the target copy follows the soft update of the reference, clamped columns included (tdiff: its own layout)
    want = pc.reference_run(c["name"])["calls"][-1]["actor_t"]["log_std"]
    np.testing.assert_allclose(got["actor_t"]["log_std"], want, rtol=pc.P_RTOL, atol=pc.P_ATOL)
    assert (got["actor_t"]["log_std"] != pc.spec(c["name"])["actor_t"]["log_std"]).any()


@pytest.mark.parametrize("pair", pc.PAIRS, ids=pair_id)
def test_act_on_clamped_log_std_and_saturated_heads(N, pair, monkeypatch):
    """select_action's sample tanh(mean + exp(clamp(log_std)) eps) and the tanh heads (SAC's evaluate_action, TD3's online and
    gain-saturated target actor) on the parameters as set, before the first update."""
    c, family = pair
    got = engine_run(N, c, family, monkeypatch)
    obs = pc.act_inputs(c["name"])[0]
    for label, eps, target, tol in pc.act_checks(c):
        np.testing.assert_allclose(got["acts"][label], pc.act_reference(c["name"], obs, eps, target), err_msg="%s %s" % (pair_id(pair), label), **tol)


@pytest.mark.parametrize("family", pc.POPULATION_FAMILIES)
def test_population_of_three_layouts_each_against_its_own_reference(N, family, monkeypatch):
    """Three learners of one engine at the narrow shape with the upper, the lower and an interior layout: a gate (or a clamp) indexed
    by anything but the learner's own log_std gives at least one of them another learner's columns."""
    cs = pc.POPULATION
    assert not _STOP, "not started: an earlier run of this module ended with %r" % (_STOP[0],)
    for c in cs:
        pc.assert_conditions(c)
    B = cs[0]["batch"]
    e = make_engine(N, cs[0], pc.SHAPES["narrow"]["families"][family], monkeypatch, n_learners=len(cs))
    try:
        path = e.learn_path(B)
        assert pc.path_is(family, path, B), (path, family)
        for p, c in enumerate(cs):
            load(N, e, c, learner=p)
        per_call, snaps = [], [[] for _ in cs]
        for k in range(cs[0]["n_calls"]):
            per_call.append(learn_call(N, e, cs, k).copy())
            for p, c in enumerate(cs):
                snaps[p].append(snapshot(N, e, c, learner=p))
        for p, c in enumerate(cs):
            got = dict(final_state(N, e, c, learner=p), **stats_of(N, c, per_call, learner=p))
            assert_learner(c, got, "learner %d (%s) on %s" % (p, c["layout"], family))
            assert_gate(c, snaps[p], "learner %d (%s) on %s" % (p, c["layout"], family))
    finally:
        e.close()
