"""GPU: frl_her_relabel / her_relabel_kernel (csrc/kernels_her.hip) against tests/her_oracle.py and against the rows the reference's
DDPG_simple_try_HER.py loop added to its own buffer (tests/golden/her.npz), bit for bit over the whole ring, and the `her` training
loop against the reference's (tests/golden/loop_her_pendulum.npz).

Rewards in mode `shaping` are compared EXACTLY: the kernel's float64 products and sums are not fused (its reward function is compiled
with floating-point contraction off), so they are the oracle's operations one for one."""
import os
import random
import re

import numpy as np
import pytest
import torch

from tests import her_oracle as oracle
from tests.golden import synth
from tests.golden.make_loop_golden import Recorder

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CAP = 200                     # L = 40 with k = 4, R = 200 appends 154 rows: 194 <= 200
DIMS = {"s3g3a1": (3, 3, 1, oracle.SCRIPT_WEIGHTS), "s5g2a2": (5, 2, 2, (1.0, 0.3))}
K = 4


def _N():
    from freerl_amd import _native as N
    return N


@pytest.fixture(scope="module")
def engines():
    from freerl_amd.engine import Engine
    N = _N()
    made = {}

    def get(dims, P):
        if (dims, P) not in made:
            S, G, A, _ = DIMS[dims]
            made[dims, P] = Engine(N.ALGO_DDPG, S + G, A, CAP, n_learners=P, hidden=128, batch_max=64, seed=3)
        return made[dims, P]
    yield get
    for e in made.values():
        e.close()


def _records(lay, obs, act, rew, nobs, done):
    n = obs.shape[0]
    rec = np.zeros((n, lay.width), np.float32)
    rec[:, lay.obs_off[0]:lay.obs_off[0] + obs.shape[1]] = obs
    rec[:, lay.act_off[0]:lay.act_off[0] + act.shape[1]] = act
    rec[:, lay.rew_off] = rew
    rec[:, lay.next_obs_off[0]:lay.next_obs_off[0] + nobs.shape[1]] = nobs
    rec[:, lay.done_off] = done
    return rec


def _episode(rng, L, S, G, A):
    """An episode's stored rows: obs_t = [state_t | goal], next_obs_t = [state_t+1 | goal], policy actions in (-1, 1), env actions in
    (-2, 2); states N(0, 0.5) so that costs fall on both sides of the tolerance."""
    states = (0.5 * rng.standard_normal((L + 1, S))).astype(np.float32)
    goal = (0.5 * rng.standard_normal(G)).astype(np.float32)
    obs = np.concatenate((states[:-1], np.tile(goal, (L, 1))), 1)
    nobs = np.concatenate((states[1:], np.tile(goal, (L, 1))), 1)
    act = rng.uniform(-1, 1, (L, A)).astype(np.float32)
    env_act = rng.uniform(-2, 2, (L, A)).astype(np.float32)
    rew = rng.standard_normal(L).astype(np.float32)
    done = (rng.uniform(size=L) < 0.2).astype(np.float32)
    return obs, act, rew, nobs, done, env_act


def _prefill(eng, rng):
    """Every ring full of known rows (cursor back at 0, size = capacity) -> the expected ring image [P][CAP][width]."""
    img = rng.standard_normal((eng.P, CAP, eng.width)).astype(np.float32)
    for p in range(eng.P):
        eng.set_cursor(p, 0, 0)
    eng.add_batch(img.reshape(-1, eng.width), np.repeat(np.arange(eng.P), CAP))
    eng.flush()
    return img


def _run(eng, rng, dims, episodes, R, *, mode="her", with_env_actions=True, order=None):
    """episodes: {learner: (L, cursor before the real rows, size before them)}.  Real rows through add, one relabel call with injected
    picks, then the whole ring, the cursors and rows_out against the oracle."""
    N = _N()
    S, G, A, W = DIMS[dims]
    lay = eng.layout
    img = _prefill(eng, rng)
    order = list(episodes) if order is None else order
    picks, env_actions, want_rows, want_cursor = [], [], [], {}
    pyrng = random.Random(int(rng.integers(1 << 30)))
    for p in order:
        L, c0, size0 = episodes[p]
        obs, act, rew, nobs, done, env_act = _episode(rng, L, S, G, A)
        eng.set_cursor(p, c0, size0)
        real = _records(lay, obs, act, rew, nobs, done)
        eng.add_batch(real, np.full(L, p))
        pk = oracle.in_order_picks(L, K, R, pyrng)
        o, a, r, o2, d = oracle.relabel(obs, act, nobs, pk, S=S, G=G, k=K, R=R, mode=mode, weights=W, tolerance=0.5,
                                        env_actions=env_act if with_env_actions else None)
        new = _records(lay, o, a, r, o2, d)
        total = oracle.total(L, K, R)
        assert new.shape[0] == total and L + total <= CAP
        for i in range(L):
            img[p, (c0 + i) % CAP] = real[i]
        for t in range(total):
            img[p, (c0 + L + t) % CAP] = new[t]
        picks.append(pk); env_actions.append(env_act); want_rows.append(total)
        want_cursor[p] = ((c0 + L + total) % CAP, min(min(size0 + L, CAP) + total, CAP))
    rows = eng.her_relabel(order, [episodes[p][0] for p in order], state_dim=S, goal_dim=G, sample_num=K, sample_range=R,
                           mode=N.HER_SPARSE if mode == "her" else N.HER_SHAPING, weights=W, tolerance=0.5,
                           env_actions=np.concatenate(env_actions) if with_env_actions else None, picks=np.concatenate(picks))
    assert rows.tolist() == want_rows
    for p in range(eng.P):
        got = eng.read_rows(p, 0, CAP)
        assert got.tobytes() == img[p].tobytes(), "learner %d: rows %s differ" % (p, np.nonzero((got != img[p]).any(1))[0][:8])
        if p in want_cursor:
            assert eng.cursor(p) == want_cursor[p], (p, eng.cursor(p), want_cursor[p])
    return img


@pytest.mark.parametrize("R", [2, 200])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 40])
@pytest.mark.parametrize("dims", sorted(DIMS))
def test_relabel_is_bit_exact_one_learner(engines, dims, L, R):
    eng = engines(dims, 1)
    rng = np.random.default_rng(1000 * L + R)
    total = oracle.total(L, K, R)
    _run(eng, rng, dims, {0: (L, CAP - (L + 1) // 2, CAP)}, R)                   # (a) the source rows straddle the ring's end (L = 1: sit at it)
    _run(eng, rng, dims, {0: (L, CAP - L - (total + 1) // 2, CAP)}, R)           # (b) the destination rows straddle it
    _run(eng, rng, dims, {0: (L, 0, 0)}, R)                                      # a fresh ring: size grows by L + total


@pytest.mark.parametrize("dims", sorted(DIMS))
def test_three_learners_one_call(engines, dims):
    eng = engines(dims, 3)
    rng = np.random.default_rng(7)
    # different L per learner, listed out of order; learner 1 sits out of the second call and its ring must not change
    _run(eng, rng, dims, {0: (3, CAP - 2, CAP), 1: (40, CAP - 100, CAP), 2: (5, 17, 60)}, 200, order=[2, 0, 1])
    _run(eng, rng, dims, {2: (40, CAP - 20, CAP), 0: (4, CAP - 5, 100)}, 2, order=[2, 0])


@pytest.mark.parametrize("dims", sorted(DIMS))
def test_stored_actions_and_shaping(engines, dims):
    eng = engines(dims, 1)
    rng = np.random.default_rng(11)
    _run(eng, rng, dims, {0: (40, CAP - 7, CAP)}, 200, with_env_actions=False)                    # env_actions = NULL: the stored action
    img = _run(eng, rng, dims, {0: (40, 3, 50)}, 200, mode="shaping")                             # rewards exact (module docstring)
    rew = img[0, 43:43 + 154, eng.layout.rew_off]
    assert (rew < 0).all() and len(np.unique(rew)) > 100
    _run(eng, rng, dims, {0: (5, CAP - 3, CAP)}, 2, mode="shaping", with_env_actions=False)


def test_reference_rows(engines):
    """The reference loop's own buffer: real rows through policy.add, the relabel with the recorded picks and env actions."""
    from freerl_amd.DDPG_simple_try_HER import DDPG, HindsightReplay
    fx = np.load(os.path.join(GOLD, "her.npz"))
    L, k, R, E, S, G = (int(v) for v in fx["dims"])
    per = oracle.total(L, k, R)
    policy = DDPG([S + G, 1], True, 1e-3, 1e-3, 1000, torch.device("cuda"), seed=0)
    p0 = 0
    for e in range(E):
        base = e * (L + per)
        for t in range(base, base + L):
            policy.add(fx["obs"][t], fx["act"][t], fx["rew"][t], fx["next_obs"][t], bool(fx["done"][t]))
        rows = policy._e.her_relabel([0], [L], state_dim=S, goal_dim=G, sample_num=k, sample_range=R,
                                     env_actions=fx["env_actions"][e * L:(e + 1) * L], picks=fx["picks"][p0:p0 + per])
        assert rows.tolist() == [per]
        p0 += per
    n = len(fx["rew"])
    assert policy._e.cursor() == (n, n) and len(policy.buffer) == n == 776
    lay = policy._e.layout
    want = _records(lay, fx["obs"], fx["act"], fx["rew"], fx["next_obs"], fx["done"].astype(np.float32))
    assert policy._e.read_rows(0, 0, n).tobytes() == want.tobytes()
    # the class surface over the same call: HindsightReplay with rng='host' draws the recorded picks from `random`
    policy2 = DDPG([S + G, 1], True, 1e-3, 1e-3, 1000, torch.device("cuda"), seed=0)
    her = HindsightReplay(policy2, S, G)
    random.seed(0)
    for e in range(E):
        base = e * (L + per)
        for t in range(L):
            policy2.add(fx["obs"][base + t], fx["act"][base + t], fx["rew"][base + t], fx["next_obs"][base + t], bool(fx["done"][base + t]))
            her.step(fx["obs"][base + t], fx["env_actions"][e * L + t], fx["next_obs"][base + t])
        assert her.end_episode() == per and len(her) == 0
    assert policy2._e.read_rows(0, 0, n).tobytes() == want.tobytes()


def test_device_draws():
    from freerl_amd.engine import Engine
    N = _N()
    P, L, S, G, A, cap = 256, 8, 3, 3, 1, 40
    total = oracle.total(L, K, 200)
    assert total == 26
    eng = Engine(N.ALGO_DDPG, S + G, A, cap, n_learners=P, hidden=128, batch_max=16, seed=5)
    lay = eng.layout
    rng = np.random.default_rng(3)
    eps = [_episode(rng, L, S, G, A) for _ in range(P)]
    real = np.concatenate([_records(lay, o, a, r, o2, d) for o, a, r, o2, d, _ in eps])
    eng.add_batch(real, np.repeat(np.arange(P), L))

    def relabel_and_infer():
        rows = eng.her_relabel(np.arange(P), np.full(P, L), state_dim=S, goal_dim=G, sample_num=K, sample_range=200)
        assert rows.tolist() == [total] * P
        offsets = np.zeros((P, total), np.int64)
        for p in range(P):
            assert eng.cursor(p) == (L + total, L + total)
            ring = eng.read_rows(p, 0, L + total)
            obs, act, _, nobs, _, _ = eps[p]
            assert ring[:L].tobytes() == real[p * L:(p + 1) * L].tobytes()
            t = 0
            for i, n in enumerate(oracle.counts(L, K, 200)):
                for s in range(n):
                    row = ring[L + t]
                    g = row[lay.obs_off[0] + S:lay.obs_off[0] + S + G]
                    j = [jj for jj in range(L) if (nobs[jj, :G] == g).all()]
                    assert len(j) == 1, (p, i, s)
                    offsets[p, t] = j[0] - i
                    # the row is consistent with the pick actually used
                    want = _records(lay, np.concatenate((obs[i, :S], g))[None], act[i][None], oracle.reward(g, obs[i, :S]),
                                    np.concatenate((nobs[i, :S], g))[None], 0.0)
                    assert row.tobytes() == want[0].tobytes(), (p, i, s)
                    t += 1
        return offsets

    first = relabel_and_infer()
    t = 0
    for i, n in enumerate(oracle.counts(L, K, 200)):
        m = L - i
        block = first[:, t:t + n]
        assert (block >= 0).all() and (block < m).all()
        if m < K:
            assert (block == np.arange(m)).all()                    # every candidate, in order
        else:
            assert all(len(set(row)) == K for row in block.tolist())
        t += n
    # i = 0: each of the 8 offsets is in a uniform 4-subset with probability 1/2 - Binomial(256, 1/2), 5 sigma = 40
    chosen = np.array([(first[:, :K] == o).any(1).sum() for o in range(L)])
    assert (np.abs(chosen - 128) <= 40).all(), chosen
    assert len({tuple(r) for r in first.tolist()}) > P // 2          # learners draw their own picks
    for p in range(P):
        eng.set_cursor(p, L, L)
    second = relabel_and_infer()
    assert (first != second).any(1).sum() > P // 2                   # ... and so does every call
    eng.close()


def _code(N, fn):
    try:
        fn()
    except N.FrlError as ex:
        m = re.match(r"freerl_hip error (\d+): (.+)", str(ex))
        assert m and len(m.group(2)) > 10, str(ex)
        return int(m.group(1)), m.group(2)
    return 0, ""


def test_refusals_leave_ring_and_cursors_alone():
    from freerl_amd.engine import Engine
    N = _N()
    INVALID, STATE = 1, 4
    eng = Engine(N.ALGO_DDPG, 6, 1, 16, n_learners=2, hidden=128, batch_max=16)
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((10, eng.width)).astype(np.float32)
    eng.add_batch(rows, [0] * 5 + [1] * 5)
    before = [eng.read_rows(p, 0, 16).tobytes() for p in range(2)], [eng.cursor(p) for p in range(2)]
    base = dict(state_dim=3, goal_dim=3, sample_num=4, sample_range=200)
    cases = [
        ("L > size", [0], [6], {}, STATE, "stored rows"),
        ("L + total > capacity", [0], [5], {}, INVALID, "capacity"),               # 5 + 14 rows in a ring of 16
        ("S + G != obs_dim", [0], [2], dict(state_dim=3, goal_dim=2, weights=[1.0, 1.0]), INVALID, "obs_dim"),
        ("G > S", [0], [2], dict(state_dim=2, goal_dim=4, weights=[1.0] * 4), INVALID, "goal_dim"),
        ("k = 9", [0], [2], dict(sample_num=9), INVALID, "sample_num"),
        ("a learner twice", [0, 0], [2, 2], {}, INVALID, "twice"),
        ("range 0", [0], [2], dict(sample_range=0), INVALID, "sample_range"),
        ("L = 0", [1], [0], {}, INVALID, "no steps"),
        ("a pick outside its candidates", [1], [2], dict(picks=[0, 2, 0]), INVALID, "pick"),
    ]
    for name, learners, lengths, over, code, word in cases:
        got, msg = _code(N, lambda: eng.her_relabel(learners, lengths, **dict(base, **over)))
        assert got == code and word in msg, (name, got, msg)
        assert ([eng.read_rows(p, 0, 16).tobytes() for p in range(2)], [eng.cursor(p) for p in range(2)]) == before, name
    assert eng.her_relabel([1], [2], picks=[0, 1, 0], **base).tolist() == [3]        # the same engine still serves a good call
    eng.close()
    # a prioritised engine: rows written in place would have no priorities
    per = Engine(N.ALGO_DDPG, 6, 1, 16, hidden=128, batch_max=16)
    per.per_enable()
    per.add_batch(rows[:4])
    before = per.read_rows(0, 0, 16).tobytes(), per.cursor(0)
    got, msg = _code(N, lambda: per.her_relabel([0], [2], **base))
    assert got == STATE and "priority" in msg and (per.read_rows(0, 0, 16).tobytes(), per.cursor(0)) == before
    per.close()
    # an engine of another algorithm
    dqn = Engine(N.ALGO_DQN, 6, 3, 16, discrete=True, hidden=128, batch_max=16)
    got, msg = _code(N, lambda: dqn.her_relabel([0], [2], **base))
    assert got == STATE and "frl_her_relabel" in msg
    dqn.close()


def test_her_training_loop_follows_the_reference(tmp_path):
    from freerl_amd import envs as E
    from freerl_amd import train
    fx = np.load(os.path.join(GOLD, "loop_her_pendulum.npz"))
    rows_fx = np.load(os.path.join(GOLD, "her.npz"))
    FLAGS = str(fx["flags"])                      # the flags the reference script was run with
    assert "--env_name PendulumShort-v1 --seed 0 --max_episodes 4" in FLAGS and "--device cpu" in FLAGS
    argv = FLAGS.replace("--device cpu", "--device cuda").split() + ["--results_root", str(tmp_path / "results")]
    log = dict(actions=[], rewards=[])
    env = Recorder(E.make("PendulumShort-v1", prefer_gymnasium=False), log)
    out = train.run("her", argv, env=env, log=lambda *a: None)
    acts, rews = np.stack(log["actions"]), np.stack(log["rewards"])
    assert acts.shape == fx["actions"].shape, (acts.shape, fx["actions"].shape)
    worst = float(np.max(np.abs(acts - fx["actions"])))
    assert worst < 2e-3, "env actions diverge from the reference loop: max abs diff %g" % worst
    np.testing.assert_allclose(rews, fx["rewards"], rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(out["returns"], fx["returns"], rtol=1e-3, atol=1e-3)
    files = sorted(os.listdir(out["model_dir"]))
    assert (str(fx["npy_name"]), str(fx["ckpt_name"])) == ("DDPG_simple_HER_seed_0.npy", "DDPG.pt")
    assert str(fx["npy_name"]) in files and str(fx["ckpt_name"]) in files, files
    assert os.path.basename(out["model_dir"]).startswith("DDPG_simple_HER_")
    sd = torch.load(os.path.join(out["model_dir"], "DDPG.pt"))
    synth.check_digest("ckpt", {k: v.numpy() for k, v in sd.items()}, fx, 5e-3, 5e-4, "loop_her_pendulum")
    # the buffer: 776 rows, their stored rewards and done flags identical to the reference's
    buf = out["policy"].buffer
    assert len(buf) == 776 and out["policy"]._e.cursor() == (776, 776)
    np.testing.assert_array_equal(buf.rewards[:776], rows_fx["rew"])
    np.testing.assert_array_equal(buf.dones[:776], rows_fx["done"].astype(bool))
