"""CPU: tests/her_oracle.py against the rows the reference's DDPG_simple_try_HER.py loop added to its buffer (tests/golden/her.npz,
recorded by tests/golden/make_her_golden.py), bit for bit - the real rows' rewards and every column of the relabelled rows - and the
host-side pieces of freerl_amd/DDPG_simple_try_HER.py that need no device."""
import inspect
import os
import random

import numpy as np
import pytest

from tests import her_oracle as oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "her.npz"))


def _episodes(fx):
    L, K, R, E, S, G = (int(v) for v in fx["dims"])
    per = oracle.total(L, K, R)
    for e in range(E):
        base = e * (L + per)
        yield e, base, L, K, R, S, G, per


def test_real_rows_rewards(fx):
    for e, base, L, K, R, S, G, per in _episodes(fx):
        assert not fx["relabelled"][base:base + L].any() and fx["relabelled"][base + L:base + L + per].all()
        for t in range(base, base + L):                 # calcu_reward(goal, obs) of the observation before the step, goal as the script held it
            assert oracle.reward(fx["goals"][e], fx["obs"][t, :S]) == fx["rew"][t], t
            np.testing.assert_array_equal(fx["obs"][t, S:], fx["goals"][e].astype(np.float32))
    assert len(fx["rew"]) == 776


def test_relabelled_rows_bit_for_bit(fx):
    p0 = 0
    for e, base, L, K, R, S, G, per in _episodes(fx):
        sl = slice(base, base + L)
        o, a, r, o2, d = oracle.relabel(fx["obs"][sl], fx["act"][sl], fx["next_obs"][sl], fx["picks"][p0:p0 + per], S=S, G=G, k=K, R=R,
                                        env_actions=fx["env_actions"][e * L:(e + 1) * L])
        p0 += per
        out = slice(base + L, base + L + per)
        for name, got in (("obs", o), ("act", a), ("rew", r), ("next_obs", o2)):
            assert got.dtype == np.float32 and got.tobytes() == fx[name][out].tobytes(), (e, name)
        assert not fx["done"][out].any() and not d.any()
    assert p0 == len(fx["picks"])


def test_the_env_action_quirk_is_in_the_fixture(fx):
    """A relabelled row stores the env-unit noised action of its step, the real row of the same step the policy output."""
    e, base, L, K, R, S, G, per = next(_episodes(fx))
    first = fx["act"][base + L]                        # relabelled row 0 belongs to step 0
    assert first.tobytes() == fx["env_actions"][0].tobytes() and first.tobytes() != fx["act"][base].tobytes()


def test_host_picks_consume_random_like_the_script(fx):
    from freerl_amd import DDPG_simple_try_HER as H
    L, K, R, E = (int(v) for v in fx["dims"][:4])
    random.seed(0)
    got = np.concatenate([H.host_picks(L, K, R) for _ in range(E)])
    np.testing.assert_array_equal(got, fx["picks"])
    # ... and generate_goals, under the script's signature, picks the same transitions from a cached episode
    random.seed(0)
    cache = [(None, None, None, np.arange(3.0) + 10 * t) for t in range(L)]
    for i in (0, 17, L - K, L - K + 1, L - 1):
        state = random.getstate()
        goals = H.generate_goals(i, cache, K, R)
        random.setstate(state)
        m = min(R, L - i)
        offs = list(range(m)) if m < K else random.sample(range(m), K)
        assert [int(g[0]) // 10 - i for g in goals] == offs


def test_calcu_reward_and_the_surface():
    from freerl_amd import DDPG_simple_try_HER as H
    from freerl_amd import TD3, train
    assert H.DDPG is TD3.DDPG
    g, s = np.array([1.0, 0.0, 0.0]), np.array([0.5, 0.5, 1.0])
    assert H.calcu_reward(g, s, None) == -1 and H.calcu_reward(g, s, None, mode="shaping") == -(0.25 + 0.25 + 0.1 * 1.0)
    assert H.calcu_reward(g, np.array([0.9, 0.1, 0.5]), None) == 0
    with pytest.raises(Exception):
        H.calcu_reward(g, s, None, mode="other")
    # the operands' dtype carries the arithmetic: float32 arrays (the script's first episode) give the float32 cost
    g32, s32 = np.array([1, 0, 0], np.float32), np.array([0.3, 0.7, 1.9], np.float32)
    d = g32 - s32
    want = -(d[0] ** 2 + d[1] ** 2 + 0.1 * d[2] ** 2)
    got = H.calcu_reward(g32, s32, None, mode="shaping")
    assert type(got) is type(want) and got == want and got != H.calcu_reward(g32.astype(np.float64), s32.astype(np.float64), None, mode="shaping")
    assert list(inspect.signature(H.calcu_reward).parameters) == ["new_goal", "state", "action", "mode"]
    assert list(inspect.signature(H.generate_goals).parameters) == ["i", "episode_cache", "sample_num", "sample_range"]
    assert list(inspect.signature(H.gene_new_sas).parameters) == ["new_goals", "transition"]
    sig = inspect.signature(H.HindsightReplay.__init__).parameters
    assert list(sig)[1:9] == ["policy", "state_dim", "goal_dim", "sample_num", "sample_range", "mode", "relabel_action", "rng"]
    assert (sig["sample_num"].default, sig["sample_range"].default, sig["mode"].default, sig["relabel_action"].default, sig["rng"].default) == \
        (4, 200, "her", "env", "host")
    st, a, st2 = H.gene_new_sas(np.array([7.0, 8.0, 9.0]), (np.arange(6.0), np.array([0.3]), None, np.arange(6.0) + 10))
    assert st.tolist() == [0, 1, 2, 7, 8, 9] and st2.tolist() == [10, 11, 12, 7, 8, 9] and a.tolist() == [0.3]
    args = train.build_parser("her").parse_args([])
    assert (args.policy_name, args.tau, args.actor_lr, args.critic_lr, args.start_steps, args.env_name) == \
        ("DDPG_simple_HER", 0.01, 1e-3, 1e-3, 500, "Pendulum-v1")
    assert issubclass(train._HERHooks, train._Hooks)
