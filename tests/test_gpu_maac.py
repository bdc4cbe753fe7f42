"""GPU: MAAC (MAAC_file/MAAC_discrete.py) on kernels_maac.hip against the float64 NumPy oracle (tests/maac_oracle.py) on its rows and
Exp(1) draws, and against the recording of the reference class (tests/golden/maac.npz).  Tolerances: maac_oracle.TOL, unwidened.
A draw is argmax_k probs[k] / eps[k]: a near tie could flip between the GPU's summation order and NumPy's.  SEEDS holds, per case, a seed
at which the smallest relative gap between winner and runner-up over all draws of the three calls (float64 oracle) is >= 1e-4 and the
float32 oracle picks the same indices; None is the case's own seed, another one (mo.inputs(c, seed=...)) skips the golden comparison."""
import os

import numpy as np
import pytest

from tests import maac_oracle as mo
from tests.hip_helpers import flat_params, records, unflat_params
from tests.test_maac_golden import ACTOR_KEYS, _m_check

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maac.npz")
RECORDED = ("pair", "hetero", "spread3", "spread5")
# measured on the CPU (smallest gap / float32 picks the same): pair 1.2e-3, hetero 4.7e-4 (seeds + 1, + 2 of the population case: 8.8e-4,
# 3.3e-4), spread3 5.2e-4, eight 3.1e-4, wide17 1.3e-3, b1 3.0e-3, b15 1.1e-4, b33 1.1e-3; spread5's own seed 3.7e-5 (short), 9401: 2.2e-4
SEEDS = dict({name: None for name in mo.CASES}, spread5=9401)
ST_CRITIC_LOSS, ST_ACTOR_LOSS, ST_CRITIC_GNORM, ST_ACTOR_GNORM = 0, 1, 4, 5          # enum frl_stat


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


def _engine(N, c, P=1, batch_max=None):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_MAAC, [o for o, _ in c["dims"]], [a for _, a in c["dims"]], c["n_table"], n_learners=P, hidden=c["hidden"],
                  batch_max=batch_max or c["batch"], discrete=True, hidden_act=N.ACT_LEAKY_RELU)


def _load(e, c, inp, p=0):
    n = len(c["dims"])
    for j in range(n):
        for kind in (0, 1):
            e.set_params(2 * j, flat_params(inp["actor"][j], mo.ACTOR_NAMES), kind, learner=p)
            e.set_params(2 * j + 1, flat_params(inp["own"][j], mo.OWN_LAYERS), kind, learner=p)
            e.set_params(2 * n + j, np.concatenate([inp["att"][k].reshape(-1) for k in mo.ATT_KEYS]), kind, learner=p)
        e.set_alpha_state_agent(j, [np.log(c["alpha"]), 0.0, 0.0, c["alpha"]], 0, learner=p)
    e.add_batch(records(inp["table"]), learners=np.full(c["n_table"], p, np.int32))


def _critic(e, c, j, kind, p=0):
    """agent j's critic as its 20 state_dict tensors: the attention block (net 2 n + j) and its own layers (net 2 j + 1)"""
    n = len(c["dims"])
    flat = np.concatenate([e.get_params(2 * n + j, kind, p), e.get_params(2 * j + 1, kind, p)])
    return mo.unflat_critic(flat, c, j)


def _close(got, want, lr, calls, label):
    """tests/test_gpu_envelope_ddpg.py's _assert_net rule on dicts: >= 99 % of a tensor within TOL['param'], none further than 2 lr calls"""
    rtol, atol = mo.TOL["param"]
    for k in want:
        d = np.abs(got[k] - want[k])
        assert (d > atol + rtol * np.abs(want[k])).mean() <= 0.01, "%s/%s: max |diff| %.3g" % (label, k, d.max())
        assert d.max() <= 2 * lr * calls, "%s/%s: max |diff| %.3g" % (label, k, d.max())


def _close_m(got, want, label):
    for k in want:
        scale = float(np.abs(want[k]).max())
        if scale == 0.0:          # (one other agent: the key's and the query's gradients are exactly zero)
            assert not got[k].any(), label + " " + k
            continue
        assert np.quantile(np.abs(got[k] - want[k]), 0.99) <= mo.TOL["m"] * scale, "adam m %s/%s" % (label, k)


def _check_state(e, o, c, inp, calls, label, p=0, rec=None):
    n = len(c["dims"])
    for j in range(n):
        tag = "%s agent %d" % (label, j)
        actor = {kind: unflat_params(e.get_params(2 * j, kind, p), inp["actor"][j], mo.ACTOR_NAMES) for kind in (0, 1, 2)}
        critic = {kind: _critic(e, c, j, kind, p) for kind in (0, 1, 2)}
        _close(actor[0], o.actor[j], c["actor_lr"], calls, tag + " actor")
        _close(actor[1], o.actor_t[j], c["actor_lr"], calls, tag + " actor target")
        _close(critic[0], o.critic(j), c["critic_lr"], calls, tag + " critic")
        _close(critic[1], o.critic(j, True), c["critic_lr"], calls, tag + " critic target")
        _close_m(actor[2], o.aopt[j].m, tag + " actor")
        _close_m(critic[2], o.copt[j].m, tag + " critic")
        assert not any(critic[2][k].any() for k in mo.FROZEN_KEYS), tag + ": a frozen tensor has Adam state"
        assert e.opt_step(2 * j, learner=p) == e.opt_step(2 * j + 1, learner=p) == e.opt_step(2 * n + j, learner=p) == calls
        for k in mo.FROZEN_KEYS:
            assert np.array_equal(critic[0][k], inp["own"][j][k]), tag + ": frozen " + k
        if rec is not None:
            pre, (pr, pa) = "%s/%d/" % (rec[1], j), mo.TOL["param"]
            for key, got, keys in (("actor", actor[0], ACTOR_KEYS), ("actor_target", actor[1], ACTOR_KEYS), ("critic", critic[0], mo.CRITIC_KEYS),
                                   ("critic_target", critic[1], mo.CRITIC_KEYS)):
                mo.check_keys(got, keys, rec[0][pre + key + "/stats"], rec[0][pre + key + "/sample"], pr, pa, tag + " recorded " + key)
            _m_check(actor[2], ACTOR_KEYS, rec[0][pre + "actor_m/stats"], rec[0][pre + "actor_m/sample"], tag + " recorded actor m")
            _m_check(critic[2], mo.TRAINED_KEYS, rec[0][pre + "critic_m/stats"], rec[0][pre + "critic_m/sample"], tag + " recorded critic m")


def _run(e, c, inps, label, rec=None):
    """the case's calls on learner p's own inputs inps[p], each learner against its own float64 oracle after calls 1 and 3"""
    n, B, am = len(c["dims"]), c["batch"], max(a for _, a in c["dims"])
    oracles = [mo.make(c, inp, np.float64) for inp in inps]
    for p, inp in enumerate(inps):
        _load(e, c, inp, p)
    (lr, la), nr = mo.TOL["loss"], mo.TOL["norm"]
    for k in range(c["n_learn"]):
        st = e.learn(B, gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], idx=np.stack([inp["idx"][k] for inp in inps]),
                     noise=np.stack([mo.pad_eps(inp["eps"][k], n, B, am) for inp in inps]), want_stats=True)
        for p, (inp, o) in enumerate(zip(inps, oracles)):
            want = o.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"])
            if k + 1 not in mo.RECORD_AFTER:
                continue
            tag = "%s learner %d call %d" % (label, p, k + 1)
            np.testing.assert_allclose(st[p][:, ST_CRITIC_LOSS], want["critic_loss"], rtol=lr, atol=la, err_msg=tag + " critic loss")
            np.testing.assert_allclose(st[p][:, ST_ACTOR_LOSS], want["actor_loss"], rtol=lr, atol=la, err_msg=tag + " actor loss")
            np.testing.assert_allclose(st[p][:, ST_CRITIC_GNORM], want["critic_norm"], rtol=nr, err_msg=tag + " critic norm")
            np.testing.assert_allclose(st[p][:, ST_ACTOR_GNORM], want["actor_norm"], rtol=nr, err_msg=tag + " actor norm")
            _check_state(e, o, c, inp, k + 1, tag, p, None if rec is None else (rec, "%s/after%d" % (label, k + 1)))


@pytest.mark.parametrize("name", list(mo.CASES))
def test_cases_against_oracle_and_recording(N, name):
    c = mo.case(name)
    rec = None
    if name in RECORDED and SEEDS[name] is None:
        with np.load(GOLDEN) as z:
            rec = {k: z[k] for k in z.files if k.startswith(name + "/")}
    e = _engine(N, c)
    _run(e, c, [mo.inputs(c, seed=SEEDS[name])], name, rec)
    e.close()


def test_population_of_three(N):
    """three learners of hetero with seeds seed, seed + 1, seed + 2 in one engine, each against its own oracle"""
    c = mo.case("hetero")
    e = _engine(N, c, P=3)
    _run(e, c, [mo.inputs(c, seed=c["seed"] + k) for k in range(3)], "hetero x 3")
    e.close()


@pytest.mark.parametrize("name,P,batch_max", [("b33", 48, 64), ("spread3", 24, 64)])
def test_several_chunks_per_workgroup(N, name, P, batch_max):
    """a population for which the plan gives a gradient workgroup two 16-row chunks (b33: its second workgroup one ragged chunk)"""
    c = mo.case(name)
    e = _engine(N, c, P=P, batch_max=batch_max)
    rows = e.learn_path(c["batch"])[2]
    assert rows > e.lds_bytes()[1] == 16, "the plan gave every workgroup one chunk: %d rows" % rows
    _run(e, c, [mo.inputs(c, seed=SEEDS[name])] * P, name + " x %d" % P)
    e.close()


def test_device_drawn_call(N):
    """no idx, no noise: rows from draw_kernel, Exp(1) draws from maac_noise_kernel; two calls step every optimiser twice, give finite
    losses, leave the frozen tensors as loaded, and the same seed gives the same bits"""
    c = mo.case("hetero")
    inp = mo.inputs(c)
    runs = []
    for _ in range(2):
        e = _engine(N, c)
        _load(e, c, inp)
        for _ in range(2):
            st = e.learn(c["batch"], gamma=c["gamma"], tau=c["tau"], actor_lr=c["actor_lr"], critic_lr=c["critic_lr"], want_stats=True)
        assert np.isfinite(st).all() and (st[0][:, ST_CRITIC_GNORM] > 0).all() and (st[0][:, ST_ACTOR_GNORM] > 0).all()
        assert all(e.opt_step(net) == 2 for net in range(3 * len(c["dims"])))
        critics = [_critic(e, c, j, 0) for j in range(len(c["dims"]))]
        assert all(np.array_equal(critics[j][k], inp["own"][j][k]) for j in range(len(c["dims"])) for k in mo.FROZEN_KEYS)
        assert any(not np.array_equal(critics[0][k], inp["att"][k]) for k in mo.ATT_KEYS)
        runs.append(np.concatenate([mo.flat_critic(cr) for cr in critics]))
        e.close()
    assert np.array_equal(runs[0], runs[1])


def test_select_action(N):
    """frl_act with FRL_ACT_CAT_SAMPLE and injected draws = actor_forward's index on every row; the critic's all_q through FRL_ACT_RAW"""
    c = mo.case("hetero")
    inp = mo.inputs(c)
    e = _engine(N, c)
    _load(e, c, inp)
    tab, rows = inp["table"], 37
    for j, (O, A) in enumerate(c["dims"]):
        obs, eps = tab[j]["obs"][:rows], np.random.default_rng(j).standard_exponential((rows, A)).astype(np.float32)
        want = mo.actor_forward({k: v.astype(np.float64) for k, v in inp["actor"][j].items()}, obs.astype(np.float64), eps)[0]
        got = e.act(2 * j, N.ACT_CAT_SAMPLE, obs, eps=eps)[0, :, 0]
        assert np.array_equal(got.astype(np.int64), want), "agent %d" % j
    o = mo.make(c, inp, np.float64)
    joint = np.concatenate([t["obs"][:rows] for t in tab] + [t["act"][:rows] for t in tab], axis=1)
    for j, (O, A) in enumerate(c["dims"]):
        want = o.all_q(j, [t["obs"][:rows].astype(np.float64) for t in tab], [t["act"][:rows].astype(np.float64) for t in tab])[0]
        np.testing.assert_allclose(e.act(2 * j + 1, N.ACT_RAW, joint, out_dim=A)[0], want, rtol=1e-4, atol=1e-5, err_msg="all_q of agent %d" % j)
    e.close()
