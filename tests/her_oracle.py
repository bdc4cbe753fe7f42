"""NumPy oracle of hindsight relabelling (DDPG_file/DDPG_simple_try_HER.py:247-286,421-428): the rows an episode's end appends,
from the episode's stored rows and the picks.  Rewards in float64 from float32 values, every product and sum rounded on its own,
left to right - what the script's Python arithmetic does on its float64 arrays."""
import numpy as np

SCRIPT_WEIGHTS = (1.0, 1.0, 0.1)


def counts(L, k, R):
    """n_i = min(k, R, L - i) for i = 0 .. L-1."""
    return [min(k, R, L - i) for i in range(L)]


def total(L, k, R):
    return sum(counts(L, k, R))


def in_order_picks(L, k, R, rng):
    """Offsets j - i in output order: all candidates in order when m_i < k, else k distinct ones from `rng` (a random.Random)."""
    out = []
    for i in range(L):
        m = min(R, L - i)
        out.extend(range(m) if m < k else rng.sample(range(m), k))
    return np.asarray(out, dtype=np.int32)


def cost(goal, state, weights=SCRIPT_WEIGHTS):
    """sum_c w_c (g_c - s_c)^2, float64, left to right; goal / state are promoted exactly from whatever they hold."""
    c = None
    for j, w in enumerate(weights):
        d = np.float64(goal[j]) - np.float64(state[j])
        t = np.float64(w) * (d * d)
        c = t if c is None else c + t
    return c


def reward(goal, state, mode="her", weights=SCRIPT_WEIGHTS, tolerance=0.5):
    c = cost(goal, state, weights)
    if mode == "shaping":
        return np.float32(-c)
    assert mode == "her"
    return np.float32(0.0 if c < tolerance else -1.0)


def relabel(obs, act, next_obs, picks, *, S, G, k=4, R=200, mode="her", weights=SCRIPT_WEIGHTS, tolerance=0.5, env_actions=None):
    """obs / next_obs [L][S + G], act [L][A] float32: the episode's stored rows in time order.  picks: the offsets in output order.
    -> (obs, act, reward, next_obs, done) of the relabelled rows, float32, [total][...]."""
    obs, act, next_obs = np.asarray(obs, np.float32), np.asarray(act, np.float32), np.asarray(next_obs, np.float32)
    L = obs.shape[0]
    a_src = act if env_actions is None else np.asarray(env_actions, np.float32).reshape(L, -1)
    o, a, r, o2 = [], [], [], []
    p = 0
    for i, n in enumerate(counts(L, k, R)):
        m = min(R, L - i)
        for s in range(n):
            off = int(picks[p]); p += 1
            assert 0 <= off < m, (i, s, off, m)
            g = next_obs[i + off, :G]
            o.append(np.concatenate((obs[i, :S], g)))
            o2.append(np.concatenate((next_obs[i, :S], g)))
            a.append(a_src[i])
            r.append(reward(g, obs[i, :S], mode, weights, tolerance))
    assert p == len(picks)
    n = len(o)
    return (np.asarray(o, np.float32).reshape(n, S + G), np.asarray(a, np.float32).reshape(n, -1), np.asarray(r, np.float32),
            np.asarray(o2, np.float32).reshape(n, S + G), np.zeros(n, np.float32))
