"""`HAPPO` with the reference's class surface (MAPPO_file/HAPPO.py:228-483): MAPPO's nets and joint ring on the engine
`freerl_amd.MAPPO` uses, updated by `frl_happo_learn` (kernels_happo.hip): the agents are visited in a random order, and a later
agent's surrogate is weighted row by row with the product of the earlier agents' new-over-old policy ratios over the whole horizon.

    HAPPO(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None)

Every critic reads the concatenation of all agents' observations; advantages, value targets, adv_norm, the n-column surrogate and
critic regression and the ValueClip that changes nothing are MAPPO's (DESIGN.md "MAPPO / IPPO"); each agent has IPPO's two Adams behind
clip_grad_norm_(..., 0.5), eps 1e-5 with trick['adam_eps'], and `lr_decay` works.  With host rng `learn` consumes the generators as
the reference does: one `torch.randperm(num_agents)`, then K `np.random.permutation(horizon)` per visited agent in visiting order.
Reference defect not kept (DESIGN.md "HAPPO"): the discrete branch takes the new log-probabilities on the loop's last minibatch only
(HAPPO.py:449-450); here both kinds take them over the whole horizon in time order, as the continuous branch does.
"""
import numpy as np
import torch

from . import _native as N
from .IPPO import IPPO
from .MAPPO import MAPPO, MultiAgentPPO


class HAPPO(MultiAgentPPO):
    _algo = N.ALGO_HAPPO
    _file = "HAPPO.pth"
    _critic_in = MAPPO._critic_in                # the global observation (HAPPO.py:199)
    _optimizers = IPPO._optimizers               # two Adams per agent (HAPPO.py:237-242)
    lr_decay = IPPO.lr_decay                     # HAPPO.py:460-467

    def learn(self, minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta=None):
        order = perms = None
        if self._rng != "device":
            # HAPPO.py:375 draws the order, then :398 one permutation per epoch of the agent being visited; `perms` is indexed by agent id
            order = torch.randperm(self.num_agents).numpy()
            perms = np.zeros((1, self.num_agents, K_epochs, self.horizon), dtype=np.int64)
            for i in order:
                for k in range(K_epochs):
                    perms[0, i, k] = np.random.permutation(self.horizon)
        a0 = self.agents[self.agent_ids[0]]
        out = self._e.happo_learn(self.horizon, minibatch_size, K_epochs, gamma=gamma, lmbda=lmbda, clip=clip_param,
                                  ent_coef=entropy_coefficient, adv_norm=self.trick["adv_norm"], value_clip=self.trick["ValueClip"],
                                  huber_delta=huber_delta if self.trick["huber_loss"] else None, perms=perms, agent_order=order,
                                  want_trace=getattr(self, "track_loss", False), actor_lr=a0.actor_optimizer.lr,
                                  critic_lr=a0.critic_optimizer.lr, adam_eps=a0.actor_optimizer.param_groups[0]["eps"], clip_norm=0.5)
        self.last_trace = out.get("trace")
