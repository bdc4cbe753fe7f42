"""`IPPO` with the reference's class surface (MAPPO_file/IPPO.py:155-347): independent PPO learners, one per agent, on the engine
`freerl_amd.MAPPO` uses (kernels_mappo.hip) with the own-observation critic.

    IPPO(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None)

The critic of agent i takes agent i's observation, the advantage and value target are agent i's column, adv_norm is per column, and
each agent has two Adams behind clip_grad_norm_(..., 0.5), eps 1e-5 with trick['adam_eps'].  Reference defect not kept:
`Critic.id_num` (IPPO.py:119-126) is a class-level counter, so a second `IPPO(...)` in one process indexes past `dim_info`; here a
critic's width is its agent's own index's.
"""
from . import _native as N
from ._core import OptimizerView
from .MAPPO import MultiAgentPPO


class IPPO(MultiAgentPPO):
    _algo = N.ALGO_IPPO
    _file = "IPPO.pth"

    def _critic_in(self, j):
        return self._od[j]

    def _optimizers(self, agent, j, actor_lr, critic_lr):
        eps = 1e-5 if self.trick["adam_eps"] else 1e-8                     # IPPO.py:164-169
        agent.actor_optimizer = OptimizerView(self._e, 2 * j, actor_lr, eps=eps)
        agent.critic_optimizer = OptimizerView(self._e, 2 * j + 1, critic_lr, eps=eps)

    def learn(self, minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta=None):
        a0 = self.agents[self.agent_ids[0]]
        self._learn(minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta, actor_lr=a0.actor_optimizer.lr,
                    critic_lr=a0.critic_optimizer.lr, adam_eps=a0.actor_optimizer.param_groups[0]["eps"], clip_norm=0.5)

    def lr_decay(self, episode_num, max_episodes):                         # IPPO.py:324-331
        lr_a_now = self.actor_lr * (1 - episode_num / max_episodes)
        lr_c_now = self.critic_lr * (1 - episode_num / max_episodes)
        for agent in self.agents.values():
            for p in agent.actor_optimizer.param_groups:
                p["lr"] = lr_a_now
            for p in agent.critic_optimizer.param_groups:
                p["lr"] = lr_c_now
