"""The register-chained kernels (kernels_critic2 / _actor2) leave the PADDING of their 16-wide tiles out of the clip + Adam + soft
update stream: the lanes whose 16-byte slot of a first-layer tile holds only input columns past the real ones, or of a head tile an
output past the real ones, neither load nor store theta / m / v / target (device/chain_net.hpp: unit_voff, adam_head).  The padded
slots hold exact zeros and nothing writes them.

Shapes (O, A), chosen so that every padding boundary occurs (a lane group q holds input columns 4q .. 4q + 3):

    (8, 2)   critic first layer 10 columns: q = 2 partly real, q = 3 padding;   actor 8 columns: q >= 2 padding
    (7, 3)   critic 10 columns;                                                 actor 7 columns: q = 1 partly real
    (3, 1)   critic 4 columns: q >= 1 padding;                                  actor 3 columns: q = 0 partly real
    (12, 4)  critic 16 columns: no padding;                                     actor 12 columns: q = 3 padding, four head outputs

Batches: 100 (ragged: the last 16-row tile partly filled, one 128-row chunk partly empty) and 256.  Every case runs the chained family
(FRL_CRITIC_V2=1) on P = 3 learners, each with its own parameters and table, and asserts learn_path(B)[0].

  1. oracle parity after 4 learn() calls (the delayed policy step on calls 1 and 3: m, v and the targets are written at least twice),
     with the helpers and tolerances of tests/test_gpu_narrow_population.py, plus Adam's second moment element-wise;
  2. two engines with the same inputs end with the same bits in every array, and the padded slots are still exact zeros
     (a dropped lane that read something other than zero would show here);
  3. set_params of all four kinds, get_params bit-equal, and one more learn() that matches an oracle restarted from those vectors.

Tests 2 and 3 run at batch 100 only: the update phase they aim at does not depend on the batch, and 100 is the ragged one.

Inputs are given (idx=, noise=), and they are chosen so that the comparison is well posed (_pick): a draw is passed over when the ORACLE,
on its own, has a hidden pre-activation closer to zero than fp32 can resolve, because then whether that ReLU unit is open for that row is
not defined by the reference, two correct fp32 implementations take different branches, and everything downstream of the unit's gradient
differs by a whole row's term instead of by rounding.  (The first version of this file drew without that rule; DDPG (3, 1) at batch 100 had
a critic layer-2 pre-activation of 1.5e-8 in its third call, and the actor loss of that call — the mean of Q through the critic just
updated — was 3.8e-4 off the oracle for rtol 1e-4, with this library and with the one from before the padding was skipped alike.)"""
import contextlib
import copy

import numpy as np
import pytest

from tests.golden import cases, synth
from tests.hip_helpers import flat_params, records, unflat_params
from tests.test_gpu_wide_population import AC, SAC_A, TWIN, _assert_adam_m, _assert_net, _fill

pytestmark = pytest.mark.gpu
P, N_TAB, CAP, CALLS = 3, 400, 512, 4
SINGLE = ["l1", "l2", "l3"]
KW = dict(gamma=0.99, tau=0.005, actor_lr=1e-3, critic_lr=1e-3)
# (algorithm, O, A, FRL_CHAIN_WAVES)
CONFIGS = [("TD3", 8, 2, None), ("TD3", 7, 3, None), ("TD3", 3, 1, None), ("TD3", 12, 4, None), ("TD3", 8, 2, "4"),
           ("DDPG", 3, 1, None), ("SAC", 7, 3, None)]
IDS = ["%s-%d-%d%s" % (a, o, n, "-w4" if w else "") for a, o, n, w in CONFIGS]


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


def _names(algo):
    """(actor layer names, its extra parameter, critic layer names)"""
    return (SAC_A, "log_std", TWIN) if algo == "SAC" else (AC, None, TWIN if algo == "TD3" else SINGLE)


def _make_engine(N, monkeypatch, algo, O, A, B, waves):
    from freerl_amd.engine import Engine
    monkeypatch.setenv("FRL_CRITIC_V2", "1")
    monkeypatch.delenv("FRL_SOLO", raising=False)
    if waves:
        monkeypatch.setenv("FRL_CHAIN_WAVES", waves)
    else:
        monkeypatch.delenv("FRL_CHAIN_WAVES", raising=False)
    e = Engine(getattr(N, "ALGO_" + algo), O, A, CAP, n_learners=P, twin_critic=(algo != "DDPG"), batch_max=B)
    assert e.learn_path(B)[0], "%s (%d, %d) batch %d did not take the register-chained kernels: %r" % (algo, O, A, B, e.learn_path(B))
    return e


def _initial(algo, O, A, p):
    an, extra, cn = _names(algo)
    if algo == "SAC":
        a = synth.mlp_params(41000 + p, cases.actor_layers(O, A, head="mean_layer"))
        actor = dict([("log_std", np.random.default_rng(42000 + p).uniform(-0.5, 0.2, (1, A)).astype(np.float32))] + list(a.items()))
    else:
        actor = synth.mlp_params(41000 + p, cases.actor_layers(O, A))
    critic = synth.mlp_params(43000 + p, cases.critic_layers(O + A, twin=(algo != "DDPG")))
    return actor, critic


def _oracle(algo, actor, critic, O, A):
    from oracle import algos
    if algo == "SAC":
        return algos.SAC(actor, critic, O, A, 1e-3, 1e-3, CAP)
    if algo == "DDPG":
        return algos.DDPG(actor, critic, O, A, 1e-3, 1e-3, CAP)
    return algos.TD3(actor, critic, O, A, 1e-3, 1e-3, CAP)


def _load(N, e, algo, ref):
    """Every learner's own initial parameters (online = target) and table into the engine"""
    an, extra, cn = _names(algo)
    tabs = ref["tabs"]
    for p in range(P):
        actor, critic = ref["actors"][p], ref["critics"][p]
        for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
            e.set_params(0, flat_params(actor, an, extra), kind, learner=p)
            e.set_params(1, flat_params(critic, cn), kind, learner=p)
        if algo == "SAC":
            e.set_alpha_state([np.log(0.01), 0, 0, 0.01], 0, learner=p)
        recs = records([tabs[p]])
        e.add_batch(recs, learners=np.full(len(recs), p, np.int32))


@contextlib.contextmanager
def _relu_ties():
    """Watches every hidden layer the oracle evaluates (oracle.nn.linear with cases.H outputs: a ReLU follows) and reports whether any
    pre-activation z = sum_k x_k w_k + b lies inside the rounding of that sum in fp32.  Bound: sqrt(n) u (sum_k |x_k w_k| + |b|) with u = 2^-24,
    the probabilistic error bound of an n-term fp32 sum in ANY order (Higham & Mary 2019; the worst case n u ... is never seen and would
    reject every draw).  It is ~1e-6 at the 128-term layer, about five times the random-walk estimate u sqrt(n) |partial sums| ~ 2e-7:
    that factor is the room for the rounding x inherits from the layer before and the parameters from the Adam steps before."""
    from oracle import nn
    orig, tie = nn.linear, [False]

    def watched(x, p, name):
        z = orig(x, p, name)
        w = p[name + ".weight"]
        if w.shape[0] == cases.H:
            mag = np.abs(x) @ np.abs(w).T + np.abs(p[name + ".bias"])
            tie[0] = tie[0] or bool((np.abs(z) < np.sqrt(w.shape[1]) * 2.0 ** -24 * mag).any())
        return z
    nn.linear = watched
    try:
        yield tie
    finally:
        nn.linear = orig


def _oracle_learn(orc, algo, idx_p, nz_p):
    """one oracle update on learner p's inputs -> (critic loss, actor loss or None, alpha loss or None)"""
    if algo == "SAC":
        return orc.learn_with(idx_p, nz_p[0], nz_p[1], 0.99, 0.005)
    if algo == "DDPG":
        return orc.learn_with(idx_p, None, 0.99, 0.005) + (None,)
    return orc.learn_with(idx_p, nz_p[0], 0.99, 0.005, 0.2, 0.5, 1.0, 2, 1.0) + (None,)


def _pick(orc, algo, k, p, B, A):
    """idx [B] and noise [2, B, A] of learner p's call k: the first draw of a fixed seed sequence on which the oracle's update has no ReLU tie
    (_relu_ties) -> (idx, noise, the oracle after that update, its losses).  Decided by the oracle alone, before any kernel runs."""
    for s in range(200):
        idx_p = synth.indices(44000 + 100 * k + p + 1000 * s, N_TAB, B)
        nz_p = np.random.default_rng(45000 + 100 * k + p + 1000 * s).standard_normal((2, B, A)).astype(np.float32)
        trial = copy.deepcopy(orc)
        with _relu_ties() as tie:
            losses = _oracle_learn(trial, algo, idx_p, nz_p)
        if not tie[0]:
            return idx_p, nz_p, trial, losses
    raise AssertionError("no well-posed draw in 200 for learner %d call %d" % (p, k))


_REF = {}


def _reference(algo, O, A, B):
    """Computed once per (algorithm, shape, batch) and shared, never changed: every learner's table and initial parameters, the inputs of
    the CALLS calls, the oracle's losses per call and the oracles after the last call."""
    key = (algo, O, A, B)
    if key not in _REF:
        tabs, actors, critics, orcs = [], [], [], []
        for p in range(P):
            tabs.append(synth.transitions(40000 + p, N_TAB, O, A))
            actor, critic = _initial(algo, O, A, p)
            actors.append(actor); critics.append(critic)
            orcs.append(_oracle(algo, actor, critic, O, A))
            _fill(orcs[p], tabs[p])
        inputs, losses = [], []
        for k in range(CALLS):
            picked = [_pick(orcs[p], algo, k, p, B, A) for p in range(P)]
            orcs = [x[2] for x in picked]
            inputs.append((np.stack([x[0] for x in picked])[:, None], np.stack([x[1] for x in picked])[:, None]))
            losses.append([x[3] for x in picked])
        _REF[key] = dict(tabs=tabs, actors=actors, critics=critics, inputs=inputs, losses=losses, orcs=orcs)
    return _REF[key]


def _learn(N, e, algo, B, A, k, idx, nz, do_actor):
    if algo == "SAC":
        return e.learn(B, alpha_lr=1e-4, target_entropy=-float(A), idx=idx, noise=nz, want_stats=True, **KW)
    if algo == "DDPG":
        return e.learn(B, do_actor=do_actor, idx=idx, noise=nz, want_stats=True, **KW)
    return e.learn(B, do_actor=do_actor, use_policy_noise=True, policy_noise=0.2, noise_clip=0.5, max_action=1.0, idx=idx, noise=nz,
                   want_stats=True, **KW)


def _check_losses(N, st, p, want, lab):
    cl, al, ll = want
    np.testing.assert_allclose(st[p, 0, N.STAT_CRITIC_LOSS], cl, rtol=1e-4, err_msg="critic loss, " + lab)
    if al is not None:
        # (atol as in tests/test_gpu_narrow_population.py: 1e-5 for SAC — the one with an alpha loss —, 1e-6 for TD3 / DDPG)
        np.testing.assert_allclose(st[p, 0, N.STAT_ACTOR_LOSS], al, rtol=1e-4, atol=1e-6 if ll is None else 1e-5, err_msg="actor loss, " + lab)
    if ll is not None:
        np.testing.assert_allclose(st[p, 0, N.STAT_ALPHA_LOSS], ll, rtol=1e-4, err_msg="alpha loss, " + lab)


def _assert_adam_v(got_flat, opt_v, names, extra, label):
    """Adam's second moment against the oracle's.  tests/test_gpu_wide_population.py bounds the FIRST moment — an average of the clipped
    gradient g — by eps of the array's largest element: eps = 2e-3 on 99 % of a matrix, 5e-2 on all of it, 2e-2 on a bias vector, where
    eps covers rounding in every gradient element and single ReLU units that are open in one implementation and shut in the other.
    v is the same average of g * g.  If two implementations' gradients differ by |dg| <= eps max|g|, their squares differ by
    |2 g dg + dg^2| <= (2 eps + eps^2) max|g|^2, so the same rule holds for v with eps replaced by 2 eps + eps^2, relative to max|v|."""
    sq = lambda eps: 2 * eps + eps * eps
    got = unflat_params(got_flat, opt_v, names, extra)
    for k in opt_v:
        scale = float(np.abs(opt_v[k]).max())
        d = np.abs(got[k] - opt_v[k]).reshape(-1)
        rel = d.max() / max(scale, 1e-30)
        print("adam v %s/%s: max |diff| %.3g = %.2e of max |v| %.3g" % (label, k, d.max(), rel, scale))
        if d.size < 2048:
            assert d.max() <= sq(2e-2) * scale, "adam v %s/%s: max |diff| %.3g = %.2e of max |v| %.3g" % (label, k, d.max(), rel, scale)
            continue
        q99 = float(np.quantile(d, 0.99))
        assert q99 <= sq(2e-3) * scale, "adam v %s/%s: 99th percentile of |diff| %.3g = %.2e of max |v| %.3g" % (label, k, q99, q99 / max(scale, 1e-30), scale)
        assert d.max() <= sq(5e-2) * scale, "adam v %s/%s: max |diff| %.3g = %.2e of max |v| %.3g" % (label, k, d.max(), rel, scale)


def _check_state(N, e, orc, algo, p, lab):
    an, extra, cn = _names(algo)
    _assert_net(e.get_params(1, N.PARAM_ONLINE, learner=p), orc.critic, cn, None, 5e-4, 5e-6, lab + " critic")
    _assert_net(e.get_params(1, N.PARAM_TARGET, learner=p), orc.critic_t, cn, None, 5e-4, 5e-6, lab + " critic_target")
    _assert_net(e.get_params(0, N.PARAM_ONLINE, learner=p), orc.actor, an, extra, 5e-4, 5e-6, lab + " actor")
    _assert_net(e.get_params(0, N.PARAM_TARGET, learner=p), orc.actor_t, an, extra, 5e-4, 5e-6, lab + " actor_target")
    _assert_adam_m(e.get_params(1, N.PARAM_ADAM_M, learner=p), orc.critic_opt.m, cn, None, lab + " critic")
    _assert_adam_m(e.get_params(0, N.PARAM_ADAM_M, learner=p), orc.actor_opt.m, an, extra, lab + " actor")
    _assert_adam_v(e.get_params(1, N.PARAM_ADAM_V, learner=p), orc.critic_opt.v, cn, None, lab + " critic")
    _assert_adam_v(e.get_params(0, N.PARAM_ADAM_V, learner=p), orc.actor_opt.v, an, extra, lab + " actor")


def _four_calls(N, e, algo, B, A, ref, check=False):
    """CALLS learn() calls on the reference's inputs, the delayed policy step on the odd ones; check: the losses against the oracle's per call"""
    for k in range(CALLS):
        idx, nz = ref["inputs"][k]
        st = _learn(N, e, algo, B, A, k, idx, nz, do_actor=(k % 2 == 1))
        assert np.all(np.isfinite(st))
        for p in range(P if check else 0):
            _check_losses(N, st, p, ref["losses"][k][p], "learner %d call %d" % (p, k))
    return st


@pytest.mark.parametrize("B", [100, 256])
@pytest.mark.parametrize("algo,O,A,waves", CONFIGS, ids=IDS)
def test_chained_update_matches_oracle(N, monkeypatch, algo, O, A, waves, B):
    ref = _reference(algo, O, A, B)
    e = _make_engine(N, monkeypatch, algo, O, A, B, waves)
    _load(N, e, algo, ref)
    _four_calls(N, e, algo, B, A, ref, check=True)
    for p in range(P):
        _check_state(N, e, ref["orcs"][p], algo, p, "%s (%d, %d) B=%d learner %d" % (algo, O, A, B, p))
    e.close()


def _all_arrays(N, e):
    return [e.get_params(net, kind, learner=p) for net in range(2) for kind in (N.PARAM_ONLINE, N.PARAM_TARGET, N.PARAM_ADAM_M, N.PARAM_ADAM_V)
            for p in range(P)]


@pytest.mark.parametrize("algo,O,A,waves", CONFIGS, ids=IDS)
def test_same_inputs_same_bits(N, monkeypatch, algo, O, A, waves):
    B = 100
    ref = _reference(algo, O, A, B)
    out = []
    for _ in range(2):
        e = _make_engine(N, monkeypatch, algo, O, A, B, waves)
        _load(N, e, algo, ref)
        st = _four_calls(N, e, algo, B, A, ref)
        out.append((_all_arrays(N, e), st))
        for net in range(2):
            for kind in (N.PARAM_ONLINE, N.PARAM_TARGET, N.PARAM_ADAM_M, N.PARAM_ADAM_V):
                for p in range(P):
                    assert e.pad_max(net, kind, learner=p) == 0.0, "net %d kind %d learner %d: a padded slot is no longer zero" % (net, kind, p)
        e.close()
    for x, y in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("algo,O,A,waves", CONFIGS, ids=IDS)
def test_layout_stays_invisible(N, monkeypatch, algo, O, A, waves):
    B = 100
    an, extra, cn = _names(algo)
    ref = _reference(algo, O, A, B)
    tabs, actors, critics = ref["tabs"], ref["actors"], ref["critics"]
    e = _make_engine(N, monkeypatch, algo, O, A, B, waves)
    _load(N, e, algo, ref)
    _four_calls(N, e, algo, B, A, ref)
    g = np.random.default_rng(46000)
    # fresh vectors of all four kinds (weights 0.1, first moment 0.01, second moment non-negative: 1e-4 |x|): bit-equal on the way back
    scale = {N.PARAM_ONLINE: 0.1, N.PARAM_TARGET: 0.1, N.PARAM_ADAM_M: 0.01, N.PARAM_ADAM_V: 1e-4}
    vec = {}
    for net in range(2):
        for kind in scale:
            for p in range(P):
                flat = (g.standard_normal(e.num_params(net)) * scale[kind]).astype(np.float32)
                if kind == N.PARAM_ADAM_V:
                    flat = np.abs(flat)
                e.set_params(net, flat, kind, learner=p)
                vec[net, kind, p] = flat
    for (net, kind, p), flat in vec.items():
        np.testing.assert_array_equal(e.get_params(net, kind, learner=p), flat)
    # one more learn(), with the policy step, against the oracle restarted from those vectors and the engine's step counts
    orcs = []
    for p in range(P):
        un = lambda net, kind: unflat_params(vec[net, kind, p], actors[p] if net == 0 else critics[p], an if net == 0 else cn, extra if net == 0 else None)
        orc = _oracle(algo, un(0, N.PARAM_ONLINE), un(1, N.PARAM_ONLINE), O, A)
        orc.actor_t, orc.critic_t = un(0, N.PARAM_TARGET), un(1, N.PARAM_TARGET)
        orc.actor_opt.m, orc.actor_opt.v, orc.actor_opt.t = un(0, N.PARAM_ADAM_M), un(0, N.PARAM_ADAM_V), e.opt_step(0, learner=p)
        orc.critic_opt.m, orc.critic_opt.v, orc.critic_opt.t = un(1, N.PARAM_ADAM_M), un(1, N.PARAM_ADAM_V), e.opt_step(1, learner=p)
        assert orc.critic_opt.t == CALLS and orc.actor_opt.t == (CALLS // 2 if algo == "TD3" else CALLS)
        if algo == "SAC":
            (la, am, av, al), at = e.alpha_state(learner=p)
            orc.alpha_p["log_alpha"] = np.array(la, dtype=np.float32)
            orc.alpha_opt.m["log_alpha"], orc.alpha_opt.v["log_alpha"] = np.array(am, dtype=np.float32), np.array(av, dtype=np.float32)
            orc.alpha_opt.t, orc.alpha = at, np.float32(al)
        if algo == "TD3":
            orc.total_it = 1                 # the next call is a policy step (policy_freq 2)
        _fill(orc, tabs[p])
        orcs.append(orc)
    picked = [_pick(orcs[p], algo, CALLS, p, B, A) for p in range(P)]
    idx, nz = np.stack([x[0] for x in picked])[:, None], np.stack([x[1] for x in picked])[:, None]
    st = _learn(N, e, algo, B, A, CALLS, idx, nz, do_actor=True)
    for p in range(P):
        lab = "%s (%d, %d) restarted, learner %d" % (algo, O, A, p)
        _check_losses(N, st, p, picked[p][3], lab)
        _check_state(N, e, picked[p][2], algo, p, lab)
    e.close()
