"""The DQN update (kernels_dqn2.hip's one-launch kernel and kernels_dqn.hip, its row-chunk twin) where more than one learner
can tell a wrong address from a right one: prioritised-replay weights into the update at three learners (per = 1, the
reference's broadcast arithmetic, and per = 2, per-row weights), the workgroup split frl_learn picks on its own at 16 and 17
learners, and 520 learners — more 77 KB workgroups than a 256-CU part holds at once.

Every learner has its OWN transition table and its OWN parameters; the watched learners run against oracles (oracle/algos.py:
DQN.learn_with) on exactly their rows.  Tolerances are test_gpu_parity's: losses 1e-4 relative per call, parameters rtol 5e-4
/ atol 5e-6, Adam's first moment rtol 1e-3 / atol 1e-7.  DQN_file/DQN.py:104-128, DQN_with_tricks.py:242-284."""
import functools

import numpy as np
import pytest

from tests import per_cases
from tests.golden import synth
from tests.hip_helpers import flat_params, records, unflat_params
from tests.test_gpu_parity import LOSS_RTOL, assert_params_close

pytestmark = pytest.mark.gpu

F32 = np.float32
O, NA, H = 8, 4, 128
GAMMA, TAU, LR = 0.99, 0.01, 1e-3
NAMES = ["l1", "l2"]
PER = dict(alpha=0.6, beta=0.4, beta_increment=0.001, epsilon=0.01)


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


@pytest.fixture(params=["rowchunk", "fused", "fused_split"])
def dqn_path(request, monkeypatch):
    """tests/test_gpu_parity.py's fixture: draw_kernel -> dqn_grad_kernel -> adam_fused_kernel, or dqn_fused_kernel with one
    workgroup per learner / with the batch's 64-row chunks on several."""
    monkeypatch.setenv("FRL_DQN_FUSED", "0" if request.param == "rowchunk" else "1")
    monkeypatch.setenv("FRL_DQN_SPLIT", "1" if request.param == "fused" else "4")
    return request.param


def _fill(buf, tab):
    for i in range(len(tab["rew"])):
        buf.add(tab["obs"][i], tab["act"][i][0], float(tab["rew"][i]), tab["next_obs"][i], bool(tab["done"][i]))


def _plain_params(seed):
    return synth.mlp_params(seed, [("l1", H, O), ("l2", NA, H)])


def _dueling_params(seed):
    return synth.mlp_params(seed, [("l1", H, O), ("V", 1, H), ("A", NA, H)])


def _engine_layout(prm):
    """The engine's two-layer view of a Dueling net: head rows [V ; A]."""
    if "V.weight" not in prm:
        return prm
    return {"l1.weight": prm["l1.weight"], "l1.bias": prm["l1.bias"], "l2.weight": np.vstack([prm["V.weight"], prm["A.weight"]]),
            "l2.bias": np.concatenate([prm["V.bias"], prm["A.bias"]])}


def _oracle_layout(flat, like):
    got = unflat_params(flat, _engine_layout(like), NAMES)
    if "V.weight" not in like:
        return got
    return {"l1.weight": got["l1.weight"], "l1.bias": got["l1.bias"], "V.weight": got["l2.weight"][:1], "V.bias": got["l2.bias"][:1],
            "A.weight": got["l2.weight"][1:], "A.bias": got["l2.bias"][1:]}


def _assert_learner(N, e, orc, p, calls, label):
    assert_params_close(_oracle_layout(e.get_params(0, N.PARAM_ONLINE, learner=p), orc.q), orc.q, label + "/Qnet")
    assert_params_close(_oracle_layout(e.get_params(0, N.PARAM_TARGET, learner=p), orc.q_t), orc.q_t, label + "/Qnet_target")
    got_m = _oracle_layout(e.get_params(0, N.PARAM_ADAM_M, learner=p), orc.q)
    for k in got_m:
        np.testing.assert_allclose(got_m[k], orc.opt.m[k], rtol=1e-3, atol=1e-7, err_msg="%s adam m %s" % (label, k))
    assert e.opt_step(0, learner=p) == calls, label


# ------------------------------------------------------------------------------------------------ PER weights into the update
PER_P, PER_CAP, PER_ROWS, PER_B, PER_BM, PER_ROUNDS = 3, 256, 200, 100, 128, 3


@functools.lru_cache(maxsize=None)
def per_oracle(per):
    """The oracles' own sequence, one DQN + PERBuffer per learner: skewed priorities from host TD errors, then PER_ROUNDS of
    sample (uniforms by per_cases' margin rule on the oracle's tree), learn with the weights, priorities from the oracle's own
    TD errors.  Asserts what the case is there for: every batch repeats rows, and the learners' mean weights differ."""
    from oracle import algos
    from oracle.buffer import PERBuffer
    out = []
    for p in range(PER_P):
        tab, prm = synth.transitions(51000 + p, PER_ROWS, O, 1, n_discrete=NA), _plain_params(52000 + p)
        orc = algos.DQN(prm, O, NA, LR, PER_CAP)
        pb = PERBuffer(PER_CAP, O, 1, **PER)
        orc.buffer = pb.buffer
        _fill(pb, tab)
        g = np.random.default_rng(53000 + p)
        skew_idx = synth.indices(54000 + p, PER_ROWS, PER_B)
        skew_td = (np.exp((0.3 + 1.1 * p) * g.standard_normal(PER_B)) * np.where(g.random(PER_B) < 0.5, -1.0, 1.0)).astype(F32)
        pb.update_priorities(skew_idx, skew_td)
        rounds, draws, rejected = [], 0, 0
        for k in range(PER_ROUNDS):
            u, d, r = per_cases.margin_uniforms(pb.sumtree.tree, PER_B, g)
            draws, rejected = draws + d, rejected + r
            idx, w = pb.sample_with(u)
            assert len(set(idx.tolist())) < PER_B, "learner %d round %d: no repeated row" % (p, k)
            loss = orc.learn_with(idx, GAMMA, TAU, double=True, is_weight=w, per_row=(per == 2))
            pb.update_priorities(idx, orc.last_td)
            rounds.append(dict(u=u, idx=idx, w=w, loss=loss, sum=pb.sumtree.sum(), max=pb.sumtree.max()))
        assert rejected <= per_cases.REJECT_CAP * draws
        out.append(dict(tab=tab, prm=prm, orc=orc, skew_idx=skew_idx, skew_td=skew_td, rounds=rounds))
    for k in range(PER_ROUNDS):
        means = sorted(float(o["rounds"][k]["w"].mean()) for o in out)
        # per = 1 scales a learner's whole loss by its mean weight: 0.5 % apart is fifty times LOSS_RTOL
        assert min(b / a for a, b in zip(means, means[1:])) > 1.005, "round %d: mean weights %r too close to tell learners apart" % (k, means)
    return out


@pytest.mark.parametrize("per", [1, 2])
def test_per_weights_reach_the_update_of_their_own_learner(N, dqn_path, per):
    """per_sample -> learn(per, Double) -> per_update with the device's own TD errors, three learners, batch 100 (ragged inside
    a 64-row chunk and inside a 16-row tile) under a pitch of 128.  per = 1 gives every row its learner's MEAN weight, per = 2
    its own: another learner's weights, or a row's weight read at the wrong pitch, move the loss."""
    from freerl_amd.engine import Engine
    want = per_oracle(per)
    e = Engine(N.ALGO_DQN, O, NA, PER_CAP, discrete=True, batch_max=PER_BM, n_learners=PER_P)
    e.per_enable(PER["alpha"], PER["beta"], PER["beta_increment"], PER["epsilon"])
    for p, o in enumerate(want):
        flat = flat_params(o["prm"], NAMES)
        e.set_params(0, flat, N.PARAM_ONLINE, learner=p); e.set_params(0, flat, N.PARAM_TARGET, learner=p)
        recs = records([o["tab"]])
        e.add_batch(recs, learners=np.full(len(recs), p, np.int32))
    e.per_update(PER_B, idx=np.stack([o["skew_idx"] for o in want]), td_error=np.stack([o["skew_td"] for o in want]))
    for k in range(PER_ROUNDS):
        idx, w = e.per_sample(PER_B, uniforms=np.stack([o["rounds"][k]["u"] for o in want]))
        st = e.learn(PER_B, gamma=GAMMA, tau=TAU, critic_lr=LR, clip_norm=0.0, double_dqn=True, per=per, want_stats=True)
        e.per_update(PER_B)
        for p, o in enumerate(want):
            r, lab = o["rounds"][k], "per=%d %s learner %d round %d" % (per, dqn_path, p, k)
            np.testing.assert_array_equal(idx[p], r["idx"], err_msg=lab)
            # round 0's tree holds host TD errors only (test_per_buffer_sumtree_on_device's 2e-6).  Later trees hold the device's:
            # priorities within 2e-4 (below) -> p / total within 4e-4 -> ^-beta (beta < 0.41) and the division by the largest
            # weight: 2 * 0.41 * 4e-4 = 3.3e-4
            np.testing.assert_allclose(w[p], r["w"], rtol=2e-6 if k == 0 else 3.3e-4, err_msg=lab)
            np.testing.assert_allclose(st[p, 0, N.STAT_CRITIC_LOSS], r["loss"], rtol=LOSS_RTOL, err_msg=lab)
            ps = e.per_state(p)
            np.testing.assert_allclose(ps["sum"], r["sum"], rtol=2e-4, err_msg=lab)      # (float32 TD errors feed powf: the C51 PER test's bound)
            np.testing.assert_allclose(ps["max"], r["max"], rtol=2e-4, err_msg=lab)
    for p, o in enumerate(want):
        _assert_learner(N, e, o["orc"], p, PER_ROUNDS, "dqn_per%d/%s/%d" % (per, dqn_path, p))
    e.close()


# ------------------------------------------------------------------------------------------------ populations
def _population(N, P, watch, batch, capacity, rows, calls, seed, *, dueling=False, clip=0.0):
    """Engine and oracles of a population: every learner its own seeded table, parameters and rows; -> losses [calls][P]."""
    from freerl_amd.engine import Engine
    from oracle import algos
    e = Engine(N.ALGO_DQN, O, NA, capacity, discrete=True, batch_max=batch, n_learners=P, dueling=dueling)
    g = np.random.default_rng(seed)
    n_flat = e.num_params(0)
    orcs, recs = {}, []
    for p in range(P):
        tab = synth.transitions(seed + 1000 + p, rows, O, 1, n_discrete=NA)
        recs.append(records([tab]))
        if p in watch:
            prm = (_dueling_params if dueling else _plain_params)(seed + 3000 + p)
            flat = flat_params(_engine_layout(prm), NAMES)
            orcs[p] = algos.DQN(prm, O, NA, LR, capacity, dueling=dueling)
            orcs[p].clip = clip
            _fill(orcs[p], tab)
        else:
            flat = (g.standard_normal(n_flat) * 0.1).astype(F32)
        assert flat.size == n_flat
        e.set_params(0, flat, N.PARAM_ONLINE, learner=p); e.set_params(0, flat, N.PARAM_TARGET, learner=p)
    e.add_batch(np.concatenate(recs), learners=np.repeat(np.arange(P, dtype=np.int32), rows))
    return e, orcs


def _run_population(N, e, orcs, P, batch, rows, calls, seed, clip, label):
    losses = np.zeros((calls, P), F32)
    for k in range(calls):
        idx = np.stack([synth.indices(seed + 5000 + 1000 * k + p, rows, batch) for p in range(P)])
        st = e.learn(batch, gamma=GAMMA, tau=TAU, critic_lr=LR, clip_norm=clip, double_dqn=True, idx=idx[:, None, :], want_stats=True)
        losses[k] = st[:, 0, N.STAT_CRITIC_LOSS]
        for p, orc in orcs.items():
            orc.learn_with(idx[p], GAMMA, TAU, double=True)
            np.testing.assert_allclose(losses[k, p], orc.losses[-1], rtol=LOSS_RTOL, err_msg="%s learner %d call %d" % (label, p, k))
    for p, orc in orcs.items():
        _assert_learner(N, e, orc, p, calls, "%s/%d" % (label, p))
    return losses


@pytest.mark.parametrize("P,rows_per_workgroup", [(16, 64), (17, 256)])
def test_unforced_split_at_the_16_17_learner_boundary(N, monkeypatch, P, rows_per_workgroup):
    """No FRL_DQN_SPLIT: dqn_split_for gives up to 16 learners one 64-row chunk per workgroup (the last to arrive reduces and
    steps) and 17 learners one workgroup each.  Learners 0, 15 and 16 against their oracles, three calls at batch 256."""
    for v in ("FRL_DQN_SPLIT", "FRL_DQN_FUSED"):
        monkeypatch.delenv(v, raising=False)
    watch = [p for p in (0, 15, 16) if p < P]
    e, orcs = _population(N, P, watch, 256, 1024, 600, 3, 61000 + P)
    chained, _, rows = e.learn_path(256)
    assert chained and rows == rows_per_workgroup, "P = %d: learn_path(256) reports %r" % (P, (chained, rows))
    losses = _run_population(N, e, orcs, P, 256, 600, 3, 61000 + P, 0.0, "dqn_split P=%d" % P)
    assert np.all(np.isfinite(losses))
    e.close()


@pytest.mark.parametrize("head", ["plain_fused", "dueling"])
def test_more_workgroups_than_the_chip_holds(N, monkeypatch, head):
    """520 learners: at two 77 KB workgroups per CU a 256-CU part holds 512, so learners 512 .. 519 run in a second round.
    Batch 100, Double, clip_norm 0.5, three calls; the last of the first round, the first of the second and the ends against
    their oracles (losses, Qnet, target, Adam's m and step count); every learner's loss finite and unlike every other's."""
    P, B, CAP, ROWS, CALLS, CLIP = 520, 100, 128, 120, 3, 0.5
    dueling = head == "dueling"
    if dueling:
        for v in ("FRL_DQN_SPLIT", "FRL_DQN_FUSED"):
            monkeypatch.delenv(v, raising=False)
    else:
        monkeypatch.setenv("FRL_DQN_FUSED", "1")
        monkeypatch.setenv("FRL_DQN_SPLIT", "1")
    watch = (0, 519) if dueling else (0, 255, 511, 512, 519)
    seed = 73000 if dueling else 71000
    e, orcs = _population(N, P, watch, B, CAP, ROWS, CALLS, seed, dueling=dueling, clip=CLIP)
    chained, _, rows = e.learn_path(B)
    assert chained and rows == B, "P = %d did not select one workgroup per learner: %r" % (P, (chained, rows))
    losses = _run_population(N, e, orcs, P, B, ROWS, CALLS, seed, CLIP, "dqn_%s P=%d" % (head, P))
    assert np.all(np.isfinite(losses)), "a learner nobody watches produced a non-finite loss"
    for k in range(CALLS):
        assert len(set(losses[k].tolist())) == P, "call %d: two learners report the same loss" % k
    e.close()
