"""The Categorical DQN update (kernels_c51.hip) at its support and shape edges, at Engine level: losses after every call and
every online and target parameter after three calls against the oracle (oracle/algos.py: C51DQN.learn_with) on the same
seeded inputs.  Tolerances are those of the other Engine-vs-oracle tests (test_tiny_batches): losses rtol 1e-4 / atol 1e-7,
parameters rtol 1e-3 / atol 1e-5.

The tables are tests/c51_cases.py's: every batch holds rows whose target lands exactly on an atom (bottom, top, middle),
half way between two, clamped with all its atoms at either end, and `done = 0` rows whose top atoms clamp to v_max — the
common case, and on the OVERSHOOT supports the one where the float32 bin position used to be atoms - 1 plus one ulp and the
kernel stored at m[atoms], one slot past the row.  That store carried b - floor(b), one ulp of the source's
mass, so these tests pass against the unclamped kernel as well (run once on an MI355X): they pin the arithmetic around the
clamp, they cannot see the stray store.  The case they did fail on is 7 actions on 3 atoms, where the rows' q values
shared LDS slots.

Two steps of the update are discontinuous: the argmax over the next state's actions (the kernel takes it from hardware
exp) and the 1e-5 < p < 1 - 1e-5 gate of the loss.  No row is left out of any comparison; the seeds are chosen so that, in
the oracle alone, every sampled row of every call keeps its two best next-state action values more than 1e-3 of the support
width apart and every probability of its taken action outside [0.5e-5, 2e-5] and [1 - 2e-5, 1 - 0.5e-5].  Each test asserts
that on the oracle's numbers before it creates an engine."""
import functools

import numpy as np
import pytest

from tests import c51_cases
from tests.golden import cases as gcases
from tests.golden import synth

pytestmark = pytest.mark.gpu

F32 = np.float32
O, H, N_TAB, CAP, B_MAX, N_CALLS = 6, 128, 96, 96, 64, 3
GAMMA, TAU, LR = c51_cases.GAMMA, 0.01, 1e-3
LOSS_TOL = dict(rtol=1e-4, atol=1e-7)
PARAM_TOL = dict(rtol=1e-3, atol=1e-5)
HEAD_SCALE = 3.0                     # wider head weights than nn.Linear's: distinct action values, peaked distributions
SAT_ACTION, SAT_ATOM, SAT_BIAS = 1, 40, 20.0


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


# ------------------------------------------------------------------------------------------------ inputs
def engine_keys(dueling, noisy):
    """The oracle's parameter names in the engine's flat order: l1, head weights [V ; A], head biases [, sigmas]."""
    if noisy:
        return ["l1.weight", "l1.bias", "V.weight_mu", "A.weight_mu", "V.bias_mu", "A.bias_mu", "V.weight_sigma", "A.weight_sigma",
                "V.bias_sigma", "A.bias_sigma"]
    if dueling:
        return ["l1.weight", "l1.bias", "V.weight", "A.weight", "V.bias", "A.bias"]
    return ["l1.weight", "l1.bias", "l2.weight", "l2.bias"]


def to_flat(p, dueling, noisy):
    return np.concatenate([np.asarray(p[k], F32).reshape(-1) for k in engine_keys(dueling, noisy)])


def from_flat(flat, like, dueling, noisy):
    out, o = {}, 0
    for k in engine_keys(dueling, noisy):
        n = like[k].size
        out[k] = flat[o:o + n].reshape(like[k].shape)
        o += n
    assert o == flat.size
    return out


def make_params(seed, nA, atoms, dueling, noisy):
    g = np.random.default_rng(seed)
    p = dict(synth.linear_params(g, "l1", H, O))
    if not dueling:
        p.update(synth.linear_params(g, "l2", nA * atoms, H, HEAD_SCALE))
        return p
    for name, rows in (("V", atoms), ("A", nA * atoms)):
        lin = synth.linear_params(g, name, rows, H, HEAD_SCALE)
        if not noisy:
            p.update(lin)
            continue
        p[name + ".weight_mu"], p[name + ".bias_mu"] = lin[name + ".weight"], lin[name + ".bias"]
        p[name + ".weight_sigma"] = g.uniform(0.02, 0.08, (rows, H)).astype(F32)          # distinct values: exercises d/d sigma
        p[name + ".bias_sigma"] = g.uniform(0.02, 0.08, rows).astype(F32)
    return p


@functools.lru_cache(maxsize=None)
def inputs(support, nA, B, dueling, noisy, seed, saturated=False):
    atoms, vmin, vmax = support
    tab, rows = c51_cases.structured_table(seed, N_TAB, O, nA, atoms, vmin, vmax, GAMMA)
    p = make_params(seed + 1, nA, atoms, dueling, noisy)
    if saturated:                     # one atom of one action's block at p > 1 - 1e-6, its others at p < 1e-6
        p["l2.bias"] = p["l2.bias"].copy()
        p["l2.bias"][SAT_ACTION * atoms + SAT_ATOM] += F32(SAT_BIAS)
    idx = [c51_cases.batch_indices(seed + 2, rows, N_TAB, B, k) for k in range(N_CALLS)]
    eps = None
    if noisy:                         # per call the three forwards' noise: online(s'), target(s'), online(s); V then A, in then out
        g = np.random.default_rng(seed + 3)
        eps = [[{h: (gcases.noisy_f(g.standard_normal(H)), gcases.noisy_f(g.standard_normal(r))) for h, r in (("V", atoms), ("A", nA * atoms))}
                for _ in range(3)] for _ in range(N_CALLS)]
    return dict(tab=tab, rows=rows, params=p, idx=idx, eps=eps)


def eps_flat(per_call):
    return np.concatenate([np.concatenate([one[h][j] for h in ("V", "A") for j in (0, 1)]) for one in per_call]).astype(F32)


def fill(orc, tab):
    for i in range(N_TAB):
        orc.add(tab["obs"][i], tab["act"][i], float(tab["rew"][i]), tab["next_obs"][i], bool(tab["done"][i]))


def margins(orc, idx, double, eps, width):
    """(smallest gap between the two best next-state action values / support width, whether every probability of the taken
    action keeps off the loss's gate) on the rows `idx`, from the oracle's parameters as they are now."""
    obs, act, _, nobs, _ = orc.buffer.sample(idx)
    e = eps if eps is not None else (None, None, None)
    q = orc.net.forward(orc.q, nobs, e[0])[1] if double else orc.net.forward(orc.q_t, nobs, e[1])[1]
    top = np.sort(q.astype(np.float64), axis=1)
    p = orc.net.forward(orc.q, obs, e[2])[0][np.arange(len(idx)), act.astype(np.int64).reshape(-1)].astype(np.float64)
    near = lambda x: ((x >= 0.5e-5) & (x <= 2e-5)).any()
    return float((top[:, -1] - top[:, -2]).min() / width), not (near(p) or near(1 - p))


@functools.lru_cache(maxsize=None)
def oracle_run(support, nA, B, double, dueling, noisy, seed, saturated=False):
    """Three learn calls of the oracle: losses, final parameters, and the discontinuity margins of every call."""
    from oracle import algos
    atoms, vmin, vmax = support
    inp = inputs(support, nA, B, dueling, noisy, seed, saturated)
    orc = algos.C51DQN(inp["params"], O, nA, LR, CAP, atoms, vmin, vmax, dueling=dueling, noisy=noisy)
    fill(orc, inp["tab"])
    gaps, gates, losses = [], [], []
    for k in range(N_CALLS):
        e = inp["eps"][k] if noisy else None
        gap, off_gate = margins(orc, inp["idx"][k], double, e, vmax - vmin)
        gaps.append(gap)
        gates.append(off_gate)
        losses.append(orc.learn_with(inp["idx"][k], GAMMA, TAU, double=double, noisy_eps=e if noisy else (None, None, None)))
    return dict(losses=losses, q=orc.q, q_t=orc.q_t, gap=min(gaps), off_gate=all(gates))


def assert_margins(want, label):
    assert want["gap"] > 1e-3, "%s: next-state action values within %.2e of the support width: choose another seed" % (label, want["gap"])
    assert want["off_gate"], "%s: a probability of a taken action sits at the loss's 1e-5 gate: choose another seed" % label


def make_engine(N, support, nA, dueling, noisy, n_learners=1):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_DQN, O, nA, CAP, discrete=True, batch_max=B_MAX, c51=support, dueling=dueling, noisy=noisy, n_learners=n_learners)


def load(N, e, inp, dueling, noisy, learner=0):
    from tests.hip_helpers import records
    flat = to_flat(inp["params"], dueling, noisy)
    for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
        e.set_params(0, flat, kind, learner)
    e.add_batch(records([inp["tab"]]), learners=np.full(N_TAB, learner, np.int32))


def assert_params(N, e, want, dueling, noisy, label, learner=0):
    for kind, ref in ((N.PARAM_ONLINE, want["q"]), (N.PARAM_TARGET, want["q_t"])):
        got = from_flat(e.get_params(0, kind, learner), ref, dueling, noisy)
        for k in ref:
            np.testing.assert_allclose(got[k], ref[k], err_msg="%s %s %s" % (label, "target" if kind else "online", k), **PARAM_TOL)


def run_and_compare(N, support, nA, B, double, dueling, noisy, seed, saturated=False):
    want = oracle_run(support, nA, B, double, dueling, noisy, seed, saturated)
    label = "atoms %d [%g, %g] nA %d B %d" % (support + (nA, B))
    assert_margins(want, label)
    inp = inputs(support, nA, B, dueling, noisy, seed, saturated)
    e = make_engine(N, support, nA, dueling, noisy)
    load(N, e, inp, dueling, noisy)
    for k in range(N_CALLS):
        ne = eps_flat(inp["eps"][k])[None] if noisy else None
        st = e.learn(B, gamma=GAMMA, tau=TAU, critic_lr=LR, clip_norm=0.0, idx=inp["idx"][k], double_dqn=double, noisy_eps=ne, want_stats=True)
        np.testing.assert_allclose(st[0, 0, N.STAT_CRITIC_LOSS], want["losses"][k], err_msg="%s call %d" % (label, k), **LOSS_TOL)
    assert_params(N, e, want, dueling, noisy, label)
    e.close()


# ------------------------------------------------------------------------------------------------ the cases
S51, S51N, S16, S24, S28, S64, S2, S3 = c51_cases.SUPPORTS
# (support, actions, batch, Double, Dueling, seed): every support with two or three of {2, 3, 7} actions (7 up to 51 atoms),
# batches 1, 5, 33 (one row in the second 32-row chunk) and 64, Double (combine before pick_action) on and off, Dueling on
# the overshoot and 64-atom supports among others
CASES = [
    (S51, 3, 64, False, False, 180), (S51, 7, 33, True, True, 1061),
    (S51N, 2, 5, True, False, 102), (S51N, 7, 64, False, False, 2883),
    (S16, 3, 33, False, False, 104), (S16, 2, 64, True, True, 945),
    (S24, 3, 64, True, True, 1506), (S24, 7, 33, False, False, 107), (S24, 2, 1, True, False, 128),
    (S28, 3, 5, False, True, 109), (S28, 7, 64, True, False, 1426),
    (S64, 3, 33, True, True, 131), (S64, 2, 64, False, False, 172),
    (S2, 3, 33, False, False, 133), (S2, 2, 64, True, True, 334),
    (S3, 3, 1, False, True, 115), (S3, 7, 64, True, False, 256),
]
NOISY_CASE = (S24, 3, 33, True, True, 917)
CHUNK_CASE = (S24, 3, 64, True, True, 1506)
SATURATED_CASE = (S51, 3, 33, False, False, 118)
PER_SEEDS = {S51: 143, S24: 206}
# the population's seeds: learner p has POP_SEED + p, but the four held against their oracles have seeds that keep the margins
POP_SEED, POP_CHECKED = 121000, {0: 121053, 7: 121055, 8: 121066, -1: 121069}


def case_id(c):
    return "a%d[%g,%g]-nA%d-B%d%s%s" % (c[0] + (c[1], c[2], "-double" if c[3] else "", "-dueling" if c[4] else ""))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_supports_actions_batches(N, case):
    support, nA, B, double, dueling, seed = case
    run_and_compare(N, support, nA, B, double, dueling, False, seed)


def test_noisy_dueling_double_on_an_overshoot_support(N):
    """NoisyLinear heads: noisy_split and the V block's offset depend on `atoms`; the noise of the three forwards goes to
    learn(noisy_eps=...) in DQN_with_tricks.py's layout and, the same values, to the oracle."""
    support, nA, B, double, dueling, seed = NOISY_CASE
    e = make_engine(N, support, nA, dueling, True)
    assert e.noisy_eps_size() == 2 * H + support[0] + nA * support[0]
    e.close()
    run_and_compare(N, support, nA, B, double, dueling, True, seed)


@pytest.mark.parametrize("rows,cps", [("64", None), ("16", "4"), ("32", "2")])
def test_row_chunk_schedules(N, rows, cps, monkeypatch):
    """64-row chunks (two passes of the one-wave-per-row phases), and workgroups that walk four 16-row or two 32-row chunks
    and add them up in one slab: the same numbers as the default schedule, to the same tolerances."""
    monkeypatch.setenv("FRL_RC", rows)
    if cps is not None:
        monkeypatch.setenv("FRL_CPS", cps)
    support, nA, B, double, dueling, seed = CHUNK_CASE
    e = make_engine(N, support, nA, dueling, False)
    rc = e.lds_bytes()[1]
    e.close()
    if rc != int(rows):
        pytest.skip("FRL_RC=%s: the engine reports %d-row chunks" % (rows, rc))
    run_and_compare(N, support, nA, B, double, dueling, False, seed)


def test_saturated_probabilities(N):
    """One action's block holds one atom at p > 1 - 1e-6 and fifty at p < 1e-6: rows that took it are clamped on both sides of
    the loss's gate and give no gradient; the block also wins every next-state argmax, so next_dist is one atom's mass."""
    support, nA, B, double, dueling, seed = SATURATED_CASE
    from oracle import algos
    inp = inputs(support, nA, B, dueling, False, seed, True)
    orc = algos.C51DQN(inp["params"], O, nA, LR, CAP, *support)
    fill(orc, inp["tab"])
    obs, act, _, nobs, _ = orc.buffer.sample(np.concatenate(inp["idx"]))
    took = act.reshape(-1) == SAT_ACTION
    assert 3 <= took.sum() <= took.size - 3                                  # both kinds of row are in the batches
    p = orc.net.forward(orc.q, obs)[0][:, SAT_ACTION]
    assert (p[:, SAT_ATOM] > 1 - 1e-6).all() and (np.delete(p, SAT_ATOM, axis=1) < 1e-6).all()
    q = np.sort(orc.net.forward(orc.q_t, nobs)[1], axis=1)
    assert ((q[:, -1] - q[:, -2]) > 0.1 * (support[2] - support[1])).all()
    want = oracle_run(support, nA, B, double, dueling, False, seed, True)
    assert want["off_gate"]
    run_and_compare(N, support, nA, B, double, dueling, False, seed, saturated=True)


@functools.lru_cache(maxsize=None)
def per_oracle(support, nA, B, seed):
    """The oracle's side of the PER case: per call (rows, weights, loss, tree sum, tree max), then the parameters.  Asserts that
    every call samples every kind of row and keeps the margins."""
    from oracle import algos
    from oracle.buffer import PERBuffer
    atoms, vmin, vmax = support
    inp = inputs(support, nA, B, False, False, seed)
    us = [np.random.default_rng(seed + 10 + k).random(B) for k in range(N_CALLS)]
    orc = algos.C51DQN(inp["params"], O, nA, LR, CAP, atoms, vmin, vmax)
    per = PERBuffer(CAP, O, 1)
    orc.buffer = per.buffer
    fill(per, inp["tab"])
    want = []
    for k in range(N_CALLS):
        idx, w = per.sample_with(us[k])
        for kd, rs in inp["rows"].items():
            assert set(rs) & set(idx.tolist()), "call %d samples no %s row: choose another seed" % (k, kd)
        gap, off_gate = margins(orc, idx, True, None, vmax - vmin)
        assert gap > 1e-3 and off_gate, "call %d: %.2e of the support width, off the gate %s: choose another seed" % (k, gap, off_gate)
        loss = orc.learn_with(idx, GAMMA, TAU, double=True, is_weight=w)
        per.update_priorities(idx, orc.last_td)
        want.append((idx, w, loss, per.sumtree.sum(), per.sumtree.max()))
    return us, want, dict(q=orc.q, q_t=orc.q_t)


@pytest.mark.parametrize("support", [S51, S24], ids=["a51", "a24"])
def test_per_weights_and_errors(N, support):
    """PER: per_sample -> learn(per=True) -> per_update with the device's own cross-entropy errors, the only place the per-row
    errors show from outside (a row's mass in its neighbour's bin 0 moves them).  Tree sum and max against the oracle's PERBuffer
    at the rtol test_dqn_with_tricks_double_per_nstep uses for it."""
    from tests.hip_helpers import records
    from freerl_amd.engine import Engine
    nA, B, seed = 3, 64, PER_SEEDS[support]
    inp = inputs(support, nA, B, False, False, seed)
    us, want, final = per_oracle(support, nA, B, seed)
    e = Engine(N.ALGO_DQN, O, nA, CAP, discrete=True, batch_max=B_MAX, c51=support)
    e.per_enable(0.5, 0.4, 0.001, 0.01)
    flat = to_flat(inp["params"], False, False)
    for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
        e.set_params(0, flat, kind)
    e.add_batch(records([inp["tab"]]))
    for k in range(N_CALLS):
        idx, w = e.per_sample(B, uniforms=us[k])
        np.testing.assert_array_equal(idx[0], want[k][0])
        np.testing.assert_allclose(w[0], want[k][1], rtol=2e-6)
        st = e.learn(B, gamma=GAMMA, tau=TAU, critic_lr=LR, clip_norm=0.0, double_dqn=True, per=True, want_stats=True)
        e.per_update(B)
        np.testing.assert_allclose(st[0, 0, N.STAT_CRITIC_LOSS], want[k][2], **LOSS_TOL)
        ps = e.per_state()
        np.testing.assert_allclose(ps["sum"], want[k][3], rtol=2e-4)
        np.testing.assert_allclose(ps["max"], want[k][4], rtol=2e-4)
    assert_params(N, e, final, False, False, "per")
    e.close()


@pytest.mark.parametrize("P", [9, 40])
def test_population_across_the_groups_of_eight(N, P):
    """The kernel places its workgroups in groups of eight units: 9 and 40 learners, each with its own table, parameters
    and rows, at batch 33 on an overshoot support.  Learners 0, 7, 8 and the last against their own oracles; every learner
    bit for bit against an engine of its own."""
    support, nA, B, double, dueling = S24, 3, 33, True, True
    checked = sorted({0, 7, 8, P - 1})
    seeds = [POP_SEED + p for p in range(P)]
    for p in checked:
        seeds[p] = POP_CHECKED[p if p < P - 1 else -1]
    for p in checked:
        assert_margins(oracle_run(support, nA, B, double, dueling, False, seeds[p]), "learner %d" % p)
    ins = [inputs(support, nA, B, dueling, False, s) for s in seeds]
    e = make_engine(N, support, nA, dueling, False, n_learners=P)
    for p in range(P):
        load(N, e, ins[p], dueling, False, learner=p)
    losses = []
    for k in range(N_CALLS):
        st = e.learn(B, gamma=GAMMA, tau=TAU, critic_lr=LR, clip_norm=0.0, idx=np.stack([i["idx"][k] for i in ins])[:, None],
                     double_dqn=double, want_stats=True)
        losses.append(st[:, 0, N.STAT_CRITIC_LOSS].copy())
    for p in checked:
        want = oracle_run(support, nA, B, double, dueling, False, seeds[p])
        np.testing.assert_allclose([l[p] for l in losses], want["losses"], err_msg="learner %d" % p, **LOSS_TOL)
        assert_params(N, e, want, dueling, False, "learner %d" % p, learner=p)
    for p in range(P):
        one = make_engine(N, support, nA, dueling, False)
        load(N, one, ins[p], dueling, False)
        for k in range(N_CALLS):
            st = one.learn(B, gamma=GAMMA, tau=TAU, critic_lr=LR, clip_norm=0.0, idx=ins[p]["idx"][k], double_dqn=double, want_stats=True)
            assert st[0, 0, N.STAT_CRITIC_LOSS] == losses[k][p], "learner %d call %d" % (p, k)
        for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
            np.testing.assert_array_equal(e.get_params(0, kind, p), one.get_params(0, kind), err_msg="learner %d" % p)
        one.close()
    e.close()
