"""CPU: SpreadEnv(continuous_actions=False) — the Discrete(5) action space MAAC_discrete.py trains on.  Index k steps the discrete env
exactly as the one-hot of k steps the continuous one; the default stays continuous, in the class and in make_parallel."""
import numpy as np
import pytest

from freerl_amd.envs import Box, Discrete, SpreadEnv, make_parallel


def test_spread_env_discrete_actions():
    a, b = SpreadEnv(3), SpreadEnv(3, continuous_actions=False)
    assert isinstance(a.action_space("agent_0"), Box) and a.action_space("agent_0").shape == (5,)
    assert isinstance(b.action_space("agent_1"), Discrete) and b.action_space("agent_1").n == 5
    assert a.observation_space("agent_0").shape == b.observation_space("agent_0").shape == (18,)
    oa, _ = a.reset(seed=4)
    ob, _ = b.reset(seed=4)
    for ag in a.agents:
        assert np.array_equal(oa[ag], ob[ag])
    g = np.random.default_rng(0)
    seen = set()
    for _ in range(25):
        ks = {ag: int(g.integers(5)) for ag in a.agents}
        seen.update(ks.values())
        ra, rb = a.step({ag: np.eye(5, dtype=np.float32)[k] for ag, k in ks.items()}), b.step({ag: np.array(k) for ag, k in ks.items()})
        for ag in a.agents:
            assert np.array_equal(ra[0][ag], rb[0][ag]) and ra[1][ag] == rb[1][ag] and ra[2][ag] == rb[2][ag] and ra[3][ag] == rb[3][ag]
    assert seen == set(range(5)) and all(ra[3].values())


def test_make_parallel_passes_the_keyword_and_keeps_its_default():
    env = make_parallel("simple_spread_v3", N=5, prefer_pettingzoo=False, continuous_actions=False)
    assert isinstance(env.action_space("agent_4"), Discrete) and env.observation_space("agent_0").shape == (30,)
    assert isinstance(make_parallel("simple_spread_v3", prefer_pettingzoo=False).action_space("agent_0"), Box)


@pytest.mark.parametrize("k,force", [(0, (0.0, 0.0)), (1, (-1.0, 0.0)), (2, (1.0, 0.0)), (3, (0.0, -1.0)), (4, (0.0, 1.0))])
def test_each_index_pushes_its_own_way(k, force):
    """no-op, left, right, down, up: after one step from rest an agent's velocity has the sign of its action's force"""
    env = SpreadEnv(2, continuous_actions=False)
    env.reset(seed=1)
    obs, *_ = env.step({ag: np.array(k) for ag in env.agents})
    vel = obs["agent_0"][:2]
    assert np.sign(vel[0]) == np.sign(force[0]) and np.sign(vel[1]) == np.sign(force[2 - 1])
