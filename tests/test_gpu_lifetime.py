"""Buffers that the host API allocates after frl_create — the act scratch shared by frl_act, frl_act_explore and frl_gail_reward,
frl_ppo_learn's scratch, the priority trees, an env pool's staging — and frl_destroy, on the smallest shapes that reach the regrow
paths: a result computed before a buffer grew is reproduced bit for bit after it did, and every algorithm is created, driven
through its lazy paths and destroyed a few times over.  Who frees what, and what a failed allocation leaves behind, is pinned on the
CPU (tests/test_host_mem.py): free device memory is device-wide and says nothing on a shared GPU, so it is not looked at here."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P, O, NA, A, H, CAP, BM = 2, 5, 3, 2, 32, 64, 8


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.build()
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


def _engine(N, algo, obs=O, act=A, **kw):
    from freerl_amd.engine import Engine
    return Engine(algo, obs, act, CAP, **dict(dict(n_learners=P, hidden=H, batch_max=BM), **kw))


def _rand_params(e, N, scale=0.3, seed=0):
    g = np.random.default_rng(seed)
    for p in range(e.P):
        for net in range(e.n_nets):
            flat = (g.standard_normal(e.num_params(net)) * scale).astype(np.float32)
            e.set_params(net, flat, N.PARAM_ONLINE, learner=p)
            e.set_params(net, flat, N.PARAM_TARGET, learner=p)


def _rows(n, cols, seed):
    return np.random.default_rng(seed).standard_normal((P, n, cols)).astype(np.float32)


def test_act_regrow(N):
    """frl_act at 3, 70 (several row chunks; input and output buffers regrow) and 3 rows per learner again."""
    e = _engine(N, N.ALGO_DQN, act=NA, discrete=True)
    _rand_params(e, N)
    big = _rows(70, O, 1)
    small = np.ascontiguousarray(big[:, :3])
    q0 = e.act(0, N.ACT_RAW, small, out_dim=NA)
    q1 = e.act(0, N.ACT_RAW, big, out_dim=NA)
    q2 = e.act(0, N.ACT_RAW, small, out_dim=NA)
    e.close()
    assert np.all(np.isfinite(q1)) and np.all(q0 != 0) and not np.array_equal(q0[0], q0[1])
    np.testing.assert_array_equal(q0, q2)
    np.testing.assert_array_equal(q0, q1[:, :3])


def test_act_explore_regrow(N):
    """frl_act_explore at 4, 40 and 4 rows: the OU state is reallocated at every change, the act scratch grows once."""
    e = _engine(N, N.ALGO_DDPG)
    _rand_params(e, N)
    big = _rows(40, O, 2)
    small = np.ascontiguousarray(big[:, :4])
    kw = dict(kind=N.EXPLORE_NONE, max_action=2.0, out_dim=A)      # (a power of two: max_action * stored is exact)
    s0, v0 = e.act_explore(N.ACT_TANHHEAD, small, **kw)
    s1, v1 = e.act_explore(N.ACT_TANHHEAD, big, **kw)
    s2, v2 = e.act_explore(N.ACT_TANHHEAD, small, **kw)
    a = e.act(0, N.ACT_TANHHEAD, small, out_dim=A)
    e.close()
    assert np.all(np.isfinite(s1)) and np.all(s0 != 0) and np.all(np.abs(s0) < 1)
    np.testing.assert_array_equal(s0, s2)
    np.testing.assert_array_equal(v0, v2)
    np.testing.assert_array_equal(s0, s1[:, :4])
    np.testing.assert_array_equal(s0, a)
    np.testing.assert_array_equal(v0, np.float32(2.0) * a)


def test_act_between_gail_rewards(N):
    """frl_gail_reward and frl_act share one scratch: a larger frl_act between two reward calls regrows it under them."""
    e = _engine(N, N.ALGO_GAIL, hidden_act=N.ACT_LEAKY_RELU)
    _rand_params(e, N)
    rows = _rows(3, O + A, 3)
    r0 = e.gail_reward(rows, gp=0)
    logits = e.act(0, N.ACT_RAW, _rows(20, O + A, 4), out_dim=1)
    r1 = e.gail_reward(rows, gp=0)
    e.close()
    assert r0.shape == (P, 3) and np.all(np.isfinite(r0)) and np.all(r0 != 0) and np.all(np.isfinite(logits))
    np.testing.assert_array_equal(r0, r1)


def test_ppo_scratch_regrow(N):
    """frl_ppo_learn at horizon 16, 48 and 16 from the same parameters, rows and permutations: both scratch buffers regrow for
    the second call, and the third repeats the first's loss trace."""
    K, MB = 2, 8
    e = _engine(N, N.ALGO_PPO, extra_cols=A + 1)
    g = np.random.default_rng(5)
    start = [(g.standard_normal(e.num_params(net)) * 0.1).astype(np.float32) for net in range(2)]
    rec = g.standard_normal((48, e.width)).astype(np.float32) * 0.5
    lay = e.layout
    rec[:, lay.done_off] = 0
    rec[:, lay.extra_off:lay.extra_off + A] = -1.0              # stored log-probabilities
    rec[:, lay.extra_off + A] = g.random(48) < 0.1              # adv_done
    perms = {T: np.stack([[g.permutation(T) for _ in range(K)] for _ in range(P)]) for T in (16, 48)}

    def learn(T):
        for p in range(P):
            for net in range(2):
                e.set_params(net, start[net], N.PARAM_ONLINE, learner=p)
                for kind in (N.PARAM_ADAM_M, N.PARAM_ADAM_V):
                    e.set_params(net, np.zeros_like(start[net]), kind, learner=p)
                e.set_opt_step(net, 0, learner=p)
            e.set_cursor(p, 0, 0)
        e.add_batch(np.concatenate([rec] * P), learners=np.repeat(np.arange(P), 48))
        return e.ppo_learn(T, MB, K, gamma=0.99, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3,
                           perms=perms[T], want_trace=True)["trace"].copy()
    t0, t1, t2 = learn(16), learn(48), learn(16)
    e.close()
    assert t0.shape == (P, K * 2, 2) and t1.shape == (P, K * 6, 2)
    assert np.all(np.isfinite(t0)) and np.all(np.isfinite(t1)) and np.all(t0[:, :, 1] > 0)
    np.testing.assert_array_equal(t0, t2)


def test_replay_only_per(N):
    """Buffer.py's PER_Buffer on its own: frl_per_enable also allocates the sample's home on a replay-only engine."""
    e = _engine(N, N.ALGO_REPLAY_ONLY, act=NA, discrete=True)
    e.per_enable()
    g = np.random.default_rng(6)
    e.add_batch(g.standard_normal((P * 10, e.width)).astype(np.float32), learners=np.repeat(np.arange(P), 10))
    e.flush()
    idx, w = e.per_sample(BM)
    assert idx.min() >= 0 and idx.max() < 10 and np.all(np.isfinite(w)) and np.all(w > 0)
    e.per_update(BM, idx, g.standard_normal((P, BM)).astype(np.float32))
    for p in range(P):
        st = e.per_state(p)
        assert np.isfinite(st["sum"]) and st["sum"] > 0 and np.isfinite(st["max"]) and st["max"] > 0
    with pytest.raises(N.FrlError, match="freerl_hip error 4"):            # FRL_ERR_STATE
        e.per_enable()
    e.close()


class _Env:
    """The gymnasium protocol's bare bones for a callback pool of the test's own shapes."""

    def __init__(self, discrete):
        self.observation_space = types.SimpleNamespace(shape=(O,))
        self.action_space = types.SimpleNamespace(n=NA) if discrete else types.SimpleNamespace(shape=(A,), high=np.ones(A, np.float32))
        self.t = 0

    def reset(self, seed=None):
        self.t = 0
        return np.zeros(O, np.float32), {}

    def step(self, action):
        self.t += 1
        return np.full(O, 0.1 * self.t, np.float32), 1.0, False, False, {}


# frl_algo -> (Engine keywords, frl_act's (mode, input columns, out_dim), frl_act_explore's (mode, kind) or None)
LIFETIME = {
    "ALGO_REPLAY_ONLY": (dict(act_dim=NA, discrete=True), None, None),
    "ALGO_DQN": (dict(act_dim=NA, discrete=True), ("ACT_RAW", O, NA), ("ACT_ARGMAX", "EXPLORE_EPS_GREEDY")),
    "ALGO_DDPG": ({}, ("ACT_TANHHEAD", O, A), ("ACT_TANHHEAD", "EXPLORE_GAUSS")),
    "ALGO_TD3": (dict(twin_critic=True), ("ACT_TANHHEAD", O, A), ("ACT_TANHHEAD", "EXPLORE_OU")),
    "ALGO_SAC": (dict(twin_critic=True), ("ACT_RAW", O, A), ("ACT_SAC_SAMPLE", "EXPLORE_NONE")),
    "ALGO_MADDPG": (dict(obs_dim=[O, O], act_dim=[A, A]), ("ACT_TANHHEAD", O, A), None),
    "ALGO_PPO": (dict(extra_cols=A + 1), ("ACT_RAW", O, A), ("ACT_TANHHEAD", "EXPLORE_NONE")),
    "ALGO_SAC_DISCRETE": (dict(act_dim=NA, twin_critic=True), ("ACT_ARGMAX", O, 1), None),
    "ALGO_REINFORCE": (dict(act_dim=NA), ("ACT_ARGMAX", O, 1), None),
    "ALGO_ENVELOPE_DQN": (dict(act_dim=NA, discrete=True, reward_dim=2), ("ACT_RAW", O + 2, NA * 2), None),
    "ALGO_ENVELOPE_DDPG": (dict(reward_dim=2), ("ACT_TANHHEAD", O + 2, A), None),
    "ALGO_GAIL": (dict(hidden_act=3), ("ACT_RAW", O + A, 1), None),
}


@pytest.mark.parametrize("name", sorted(LIFETIME))
def test_create_and_destroy(N, name):
    """Five rounds of create, one call of each path that allocates lazily for this algorithm, destroy: every call returns FRL_OK
    (the wrappers raise otherwise)."""
    from freerl_amd.engine import Engine
    from freerl_amd.envpool import CallbackEnvPool, rollout
    assert len(LIFETIME) == N.ALGO_GAIL - N.ALGO_REPLAY_ONLY + 1
    kw, act, explore = LIFETIME[name]
    kw = dict(dict(obs_dim=O, act_dim=A, n_learners=P, hidden=H, batch_max=BM), **kw)
    obs_dim, act_dim = kw.pop("obs_dim"), kw.pop("act_dim")
    algo = getattr(N, name)
    for rnd in range(5):
        e = Engine(algo, obs_dim, act_dim, CAP, **kw)
        if act:
            out = e.act(0, getattr(N, act[0]), _rows(3 + rnd, act[1], rnd), out_dim=act[2])
            assert np.all(np.isfinite(out))
        if explore:
            store, _ = e.act_explore(getattr(N, explore[0]), _rows(4 + rnd, O, rnd), kind=getattr(N, explore[1]), epsilon=0.5, sigma=0.1,
                                     out_dim=A)
            assert np.all(np.isfinite(store))
        if algo == N.ALGO_GAIL:
            assert np.all(np.isfinite(e.gail_reward(_rows(3, O + A, rnd), gp=0)))
        if algo in (N.ALGO_DQN, N.ALGO_TD3):          # the pool's staging is bound by its first rollout step
            pool = CallbackEnvPool([_Env(algo == N.ALGO_DQN) for _ in range(P)])
            got = rollout(e, pool, 1, envs_per_learner=1, learn_every=0, batch=BM)
            assert got["env_steps"] == P
            pool.close()
            for p in range(P):
                e.set_cursor(p, 0, 0)                 # (priorities are assigned by add: PER starts on an empty buffer)
        if e.n_agents == 1:
            e.per_enable()
            e.add_batch(np.zeros((P, e.width), np.float32), learners=np.arange(P))
            e.flush()
            assert e.per_state(0)["sum"] > 0
        e.sync()
        assert e._L.frl_destroy(e._h) == 0
        e._h = None
