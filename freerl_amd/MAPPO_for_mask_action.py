"""`MAPPO` with invalid-action masking, with the reference's class surface (MAPPO_file/MAPPO_for_mask_action.py:223-412), backed by
the HIP engine: `freerl_amd.MAPPO`'s engine with one mask block per agent in every record, updated by kernels_mappo_mask.hip.

    MAPPO(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None)
    select_action(obs, avail_actions) / add(..., adv_dones, avail_actions) / learn(minibatch_size, ...)

Kept as the reference has it (DESIGN.md "MAPPO_for_mask_action"): the policy is CategoricalMasked over the raw logits (closed actions
at -1e8, torch's normalisation order, the log-prob not clamped, no entropy or gradient in a closed action); `learn` runs over the
WHOLE capacity in one minibatch per epoch whatever the cursor says and ignores `minibatch_size` (Buffer_for_PPO_mask.all() returns
the capacity, :303-304); rows never written are zeros with an all-closed mask; `clear()` resets the counters only, so rows of earlier
episodes take part again; two Adams per agent behind clip_grad_norm_(..., 0.5) and a working `lr_decay`, as in IPPO.py;
`evaluate_action` takes the argmax of the raw logits and ignores the mask; with is_continue=True the masks are stored and never read.
Critic, GAE, v_target, adv_norm, the n-column surrogate and regression are `freerl_amd.MAPPO`'s.  This class is not re-exported over
`freerl_amd.MAPPO`; `MAPPO_for_mask_action_state.py` is `freerl_amd.MAPPO_for_mask_action_state`, a subclass of this one.
"""
import numpy as np
import torch

from . import _native as N
from ._core import F32, OptimizerView
from .MAPPO import MultiAgentPPO


class MAPPO(MultiAgentPPO):
    _algo = N.ALGO_MAPPO
    _file = "MAPPO.pth"

    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None, *, rng="host", hidden=128, seed=0):
        self._mask_cols = 0 if is_continue else sum(int(v[1]) for v in dim_info.values())
        # learn() takes the whole capacity as one minibatch (:303-304)
        super().__init__(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick, rng=rng, hidden=hidden,
                         minibatch_max=max(int(horizon), 2), seed=seed)
        if is_continue:      # stored, never read (:229, :343-347): they stay on the host
            self._avail = {aid: np.zeros((max(self.horizon, 1), a), dtype=bool) for aid, a in zip(self.agent_ids, self._ad)}
        else:
            self._e.action_mask_set(True)

    def _critic_in(self, j):
        return sum(self._od)                     # the global observation (:124)

    def _optimizers(self, agent, j, actor_lr, critic_lr):
        eps = 1e-5 if self.trick["adam_eps"] else 1e-8                     # :165-170 (`ac_optimizer` is built there and never stepped)
        agent.actor_optimizer = OptimizerView(self._e, 2 * j, actor_lr, eps=eps)
        agent.critic_optimizer = OptimizerView(self._e, 2 * j + 1, critic_lr, eps=eps)

    def select_action(self, obs, avail_actions):
        if self.is_continue:                     # Normal(mean, std).sample(): the masks are not read (:250-254)
            return super().select_action(obs)
        actions, log_pis = {}, {}
        for j, aid in enumerate(self.agent_ids):
            o = np.asarray(obs[aid], dtype=F32).reshape(1, 1, -1)
            m = np.asarray(avail_actions[aid], dtype=bool).reshape(1, 1, -1)
            # CategoricalMasked(...).sample(): argmax(p / q), q ~ Exp(1), one draw of the row's shape (:256-259)
            q = torch.empty(1, self._ad[j]).exponential_(1).numpy() if self._rng != "device" else None
            a, lp = self._e.act_masked(2 * j, o, m, eps=q, want_logp=True)
            actions[aid], log_pis[aid] = np.int64(a[0, 0]), np.float32(lp[0, 0])
        return actions, log_pis

    def add(self, obs, action, reward, next_obs, done, action_log_pi, adv_dones, avail_actions):
        """the joint record [obs | act | rew | done | next_obs | log-probs | adv_done | mask block per agent]"""
        lay, r = self._e.layout, self._rec
        if self.is_continue:
            row = self._e.cursor(0)[0]
            for aid in self.agent_ids:
                self._avail[aid][row] = np.asarray(avail_actions[aid], dtype=bool).reshape(-1)
        else:
            c = lay.extra_off + 2 * self.num_agents
            for j, aid in enumerate(self.agent_ids):
                r[c:c + self._ad[j]] = np.asarray(avail_actions[aid], dtype=bool).reshape(-1)
                c += self._ad[j]
        super().add(obs, action, reward, next_obs, done, action_log_pi, adv_dones)

    def learn(self, minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta=None):
        a0 = self.agents[self.agent_ids[0]]
        self._learn(self.horizon, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta, actor_lr=a0.actor_optimizer.lr,
                    critic_lr=a0.critic_optimizer.lr, adam_eps=a0.actor_optimizer.param_groups[0]["eps"], clip_norm=0.5)

    def lr_decay(self, episode_num, max_episodes):                         # :389-396
        lr_a_now = self.actor_lr * (1 - episode_num / max_episodes)
        lr_c_now = self.critic_lr * (1 - episode_num / max_episodes)
        for agent in self.agents.values():
            for p in agent.actor_optimizer.param_groups:
                p["lr"] = lr_a_now
            for p in agent.critic_optimizer.param_groups:
                p["lr"] = lr_c_now
