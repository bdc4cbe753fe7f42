"""`MAPPO` with invalid-action masking and a global-state critic, with the reference's class surface
(MAPPO_file/MAPPO_for_mask_action_state.py:227-420), backed by the HIP engine: `freerl_amd.MAPPO_for_mask_action`'s engine created
through frl_create_ex with a state block behind every record's mask blocks, updated by kernels_mappo_state.hip.

    MAPPO(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None, state_dim=None)
    select_action(obs, avail_actions) / add(..., adv_dones, avail_actions, state) / learn(minibatch_size, ...)

Kept as the reference has it (DESIGN.md "MAPPO_for_mask_action_state"): every critic reads [all agents' observations | state], with
feature_norm over the whole concatenation (:140-155); V(s') is the critic on [next_obs | state] with the SAME state row as V(s), not a
next state (:322-323); in the critic's step the observations are indexed by the shuffled permutation and the state is not (:371-373),
so row r of the one minibatch is [obs[perm[r]] | state[r]] regressed on v_target[perm[r]].  That is a defect of the reference that
does not raise, hence the default; `state_rows="sample"` pairs every row with its own state instead.  With `state_dim=None` the class
is built and filled like the masked one and `learn()` raises ValueError, as the reference's 9-way unpack of 8-tuple buffers does (:310).
Everything else is `freerl_amd.MAPPO_for_mask_action.MAPPO`'s: the masked policy, the whole capacity in one minibatch, zero rows,
counters-only clear, two Adams per agent, `lr_decay`, `evaluate_action` ignoring the mask; with is_continue=True the masks are stored
and never read and the state is used.

Deviation: `add` with `state=None`, or a state of another length, raises ValueError when a `state_dim` is set; NumPy would store NaN
(or broadcast a scalar) in the reference's buffer.  This class is not re-exported over `freerl_amd.MAPPO`.
"""
import numpy as np

from . import _native as N
from ._core import F32
from .MAPPO_for_mask_action import MAPPO as MaskedMAPPO

STATE_ROWS = {"position": N.STATE_ROWS_POSITION, "sample": N.STATE_ROWS_SAMPLE}


class MAPPO(MaskedMAPPO):
    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None, state_dim=None, *, state_rows="position",
                 rng="host", hidden=128, seed=0):
        if state_rows not in STATE_ROWS:
            raise ValueError("state_rows %r: 'position' (the reference's pairing) or 'sample'" % (state_rows,))
        self.state_dim = state_dim               # (:251)
        self._state_dim = 0 if state_dim is None else int(state_dim)
        self._state_rows = STATE_ROWS[state_rows] if self._state_dim else N.STATE_ROWS_POSITION
        super().__init__(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick, rng=rng, hidden=hidden, seed=seed)
        self._state_col = self._e.state_info()[1]

    def _critic_in(self, j):
        return sum(self._od) + self._state_dim   # the global observation and the global state (:124-127)

    def add(self, obs, action, reward, next_obs, done, action_log_pi, adv_dones, avail_actions, state=None):
        """the joint record [obs | act | rew | done | next_obs | log-probs | adv_done | mask block per agent | state]"""
        if self._state_dim:
            s = None if state is None else np.asarray(state, dtype=F32).reshape(-1)
            if s is None or s.size != self._state_dim:
                raise ValueError("add: state of %s values, state_dim is %d" % ("no" if s is None else s.size, self._state_dim))
            self._rec[self._state_col:self._state_col + self._state_dim] = s
        super().add(obs, action, reward, next_obs, done, action_log_pi, adv_dones, avail_actions)

    def learn(self, minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta=None):
        if self.state_dim is None:               # 8-tuple buffers under a 9-way unpack (:310)
            raise ValueError("not enough values to unpack (expected 9, got 8)")
        super().learn(minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta)
