"""`DDPG_file/DDPG_simple_try_HER.py`: goal-conditioned DDPG with hindsight experience replay ("future" strategy).

The script's class part is DDPG_simple.py's unchanged, so `DDPG` is the existing class with `dim_info = [2 * obs_dim, act_dim]`;
`calcu_reward`, `generate_goals` and `gene_new_sas` keep the script's signatures and results.  What the engine adds is the replay
side: `HindsightReplay.end_episode()` writes the relabelled rows of a finished episode inside the GPU-resident ring with one launch
(frl_her_relabel) instead of one `policy.add` per row (:421-428).

Semantics kept from the script, and worth knowing:
  * a stored observation is [state | goal]; the achieved goal of a transition is next_state[:goal_dim] (the script's `[:3]`);
  * the reward of a REAL step is calcu_reward(goal, obs) of the observation BEFORE the step (:397), its stored action the policy output
    in (-1, 1), its done flag `terminated`;
  * a RELABELLED row stores `transition[1]`, the env-unit, noised, clipped action `action_` (:398,425-428) - not the policy output the
    real row of the same step stores.  `relabel_action='env'` (the default) keeps that; `'policy'` re-uses the stored action;
  * candidates of step i are steps i .. min(i + sample_range, L) - 1; fewer than sample_num: all, in order; otherwise
    random.sample (sample_num == candidates is a shuffle);
  * relabelled rewards are computed by the kernel in float64 from the float32 values the ring holds.  The script does the same
    arithmetic on float64 arrays from its second episode on; in its first episode goal and observation are float32 arrays and NumPy
    computes the cost in float32, which can differ in the last bits (mode 'shaping') or flip the threshold when the cost is within
    float32 rounding of the tolerance (mode 'her').

Generalised: any goal_dim <= state_dim, cost weights, tolerance and mode are arguments (the script's values are the defaults).
"""
import random

import numpy as np

from . import _native as N
from .TD3 import DDPG, Agent  # noqa: F401

MODES = {"her": N.HER_SPARSE, "shaping": N.HER_SHAPING}
SCRIPT_WEIGHTS = (1.0, 1.0, 0.1)          # the cost's weights (:254); their count is the script's goal width
SCRIPT_TOLERANCE = 0.5                    # :258


def _cost(goal, state, weights=SCRIPT_WEIGHTS):
    """sum_c w_c (goal_c - state_c)^2, left to right.  The operands' own dtypes carry the arithmetic (float32 arrays give a float32
    cost, as in the script's first episode); a unit weight multiplies nothing, so that it promotes nothing either."""
    total = None
    for c, w in enumerate(weights):
        term = (goal[c] - state[c]) ** 2
        if w != 1.0:
            term = w * term
        total = term if total is None else total + term
    return total


def calcu_reward(new_goal, state, action, mode='her'):
    """The script's reward of reaching `new_goal` from `state` (its signature; `action` is not used): 'her' gives 0 inside the tolerance
    and -1 outside, 'shaping' the negated cost."""
    if mode not in MODES:
        raise ValueError("mode is 'her' or 'shaping', not %r" % (mode,))
    cost = _cost(new_goal, state)
    if mode == 'shaping':
        return -cost
    return 0 if cost < SCRIPT_TOLERANCE else -1


def _offsets(m, sample_num):
    """Which of a step's m candidates are used: all in order when there are fewer than sample_num, else a random.sample of the index
    range - the same draws as random.sample of the candidate list itself, shifted by the list's origin."""
    return list(range(m)) if m < sample_num else random.sample(range(m), sample_num)


def generate_goals(i, episode_cache, sample_num=4, sample_range=200):
    """The achieved goals (next observation's first three entries) of the future transitions picked for step i of the cached episode
    of (obs, action, reward, next_obs) tuples; the script's signature."""
    m = min(sample_range, len(episode_cache) - i)
    return [np.array(episode_cache[i + o][3][:len(SCRIPT_WEIGHTS)]) for o in _offsets(m, sample_num)]


def gene_new_sas(new_goals, transition):
    """(obs, action, next_obs) of `transition` with the goal part of both observations replaced by `new_goals`; the script's signature."""
    n = len(SCRIPT_WEIGHTS)
    obs, action, next_obs = transition[0], transition[1], transition[3]
    return np.concatenate((obs[:n], new_goals)), action, np.concatenate((next_obs[:n], new_goals))


def host_picks(length, sample_num, sample_range):
    """The offsets j - i of an episode's relabelled rows in output order, consuming Python's `random` exactly as the script's loop
    over generate_goals does: one random.sample per step that has at least sample_num candidates."""
    picks = []
    for i in range(length):
        picks.extend(_offsets(min(sample_range, length - i), sample_num))
    return np.asarray(picks, dtype=np.int32)


class HindsightReplay:
    """The episode cache and the relabel loop of the script (:380,398,421-428,442) for learner 0 of `policy`'s engine - the policy
    classes are single-learner.  A population engine relabels all its learners' episodes in one launch through Engine.her_relabel.

    .step(obs, env_action, next_obs) after every policy.add of a real step (only the env action is kept: the observations are
    already in the ring, the two arguments are taken for parity with the script's cache); .end_episode() when the episode is over,
    before env.reset - it relabels inside the ring and returns the number of rows written.  rng='host' draws the picks from
    Python's `random` like the script, rng='device' leaves them to the kernel's Philox stream."""

    def __init__(self, policy, state_dim, goal_dim, sample_num=4, sample_range=200, mode='her', relabel_action='env', rng='host', *,
                 weights=None, tolerance=SCRIPT_TOLERANCE):
        if mode not in MODES:
            raise ValueError("mode is 'her' or 'shaping', not %r" % (mode,))
        if relabel_action not in ('env', 'policy') or rng not in ('host', 'device'):
            raise ValueError("relabel_action is 'env' or 'policy', rng is 'host' or 'device'")
        if weights is None:
            if goal_dim != len(SCRIPT_WEIGHTS):
                raise ValueError("the script's cost weights are for goal_dim 3: pass weights for goal_dim %d" % goal_dim)
            weights = SCRIPT_WEIGHTS
        self._e = policy._e
        self.state_dim, self.goal_dim, self.sample_num, self.sample_range = int(state_dim), int(goal_dim), int(sample_num), int(sample_range)
        self.mode, self.relabel_action, self.rng = mode, relabel_action, rng
        self.weights, self.tolerance = np.asarray(weights, dtype=np.float64), float(tolerance)
        self._env_actions = []

    def __len__(self):
        return len(self._env_actions)

    def step(self, obs, env_action, next_obs):
        self._env_actions.append(np.asarray(env_action, dtype=np.float32).reshape(-1))

    def end_episode(self):
        L = len(self._env_actions)
        if L == 0:
            return 0
        picks = host_picks(L, self.sample_num, self.sample_range) if self.rng == 'host' else None
        acts = np.stack(self._env_actions) if self.relabel_action == 'env' else None
        rows = self._e.her_relabel([0], [L], state_dim=self.state_dim, goal_dim=self.goal_dim, sample_num=self.sample_num,
                                   sample_range=self.sample_range, mode=MODES[self.mode], weights=self.weights, tolerance=self.tolerance,
                                   env_actions=acts, picks=picks)
        self._env_actions = []
        return int(rows[0])
