"""`MAPPO` with the reference's class surface (MAPPO_file/MAPPO.py:220-508), backed by the HIP engine: every agent's actor and
critic and ONE joint rollout ring live in one engine, and `learn` is one launch chain (kernels_mappo.hip) for all of them.

    MAPPO(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None)

Kept as the reference has it (DESIGN.md "MAPPO / IPPO"): every critic reads the concatenation of all agents' observations; every
actor's surrogate is the mean over ALL agents' advantage columns and every critic regresses all agents' value targets; adv_norm runs
over the whole matrix; ValueClip changes nothing; one Adam per agent over actor + critic at lr = actor_lr, eps 1e-5 whatever
trick['adam_eps'] says, no gradient clipping, `critic_lr` never read.  `lr_decay` raises: the reference's reads
`agent.actor_optimizer` (MAPPO.py:488), which this file's Agent does not have.  ObsNorm, reward_norm and reward_scaling belong to the
loop (freerl_amd/normalization.py), as in the script.  `freerl_amd.IPPO` is the independent-learner file on the same engine.
"""
import math
import os

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, F32, OptimizerView, init_layers, resolve_device
from .Buffer import _RingView

TRICK_DEFAULT = dict(adv_norm=False, ObsNorm=False, reward_norm=False, reward_scaling=False, orthogonal_init=False, adam_eps=False,
                     lr_decay=False, ValueClip=False, huber_loss=False, LayerNorm=False, feature_norm=False)
RELU_GAIN = math.sqrt(2.0)            # nn.init.calculate_gain('relu'): net_init's default (MAPPO.py:101-120)


class AgentBuffer(_RingView):
    """`buffers[agent_id]`: agent j's view of the joint ring (the reference keeps one Buffer_for_PPO per agent, written in lock-step)"""

    def __init__(self, engine, j, device, capacity):
        self._attach(engine, 0, j, device)
        self.capacity = int(capacity)

    def clear(self):
        self._e.set_cursor(0, 0, 0)


class Agent:
    """Actor + Critic of one agent (MAPPO.py:220-230 / IPPO.py:155-169): torch's generator is consumed as their constructors do
    (actor's three layers, its orthogonal re-draws, then the critic's)"""

    def __init__(self, engine, j, obs_dim, action_dim, critic_in, is_continue, trick, hidden):
        head = "mean_layer" if is_continue else "l3"
        al = [("l1", hidden, obs_dim), ("l2", hidden, hidden), (head, action_dim, hidden)]
        cl = [("l1", hidden, critic_in), ("l2", hidden, hidden), ("l3", 1, hidden)]
        ortho = bool(trick["orthogonal_init"])
        fa = init_layers(al, orthogonal=[RELU_GAIN, RELU_GAIN, 0.01] if ortho else None)
        fc = init_layers(cl, orthogonal=[RELU_GAIN] * 3 if ortho else None)
        engine.set_params(2 * j, np.concatenate([fa, np.zeros(action_dim, F32)]) if is_continue else fa)      # log_std zeros
        engine.set_params(2 * j + 1, fc)
        self.actor = DeviceNet(engine, 2 * j, al, extra=("log_std", (1, action_dim)) if is_continue else None,
                               act_mode=N.ACT_TANHHEAD if is_continue else N.ACT_RAW)
        self.critic = DeviceNet(engine, 2 * j + 1, cl)


class MultiAgentPPO:
    """What MAPPO and IPPO share: the engine, the joint ring, select / evaluate / add / save / load"""
    _algo = None
    _file = None
    _mask_cols = 0                               # mask columns behind a record's adv_done columns (MAPPO_for_mask_action.py)
    _state_dim, _state_rows = 0, 0               # state columns behind those, and their pairing (MAPPO_for_mask_action_state.py)

    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None, *, rng="host", hidden=128,
                 minibatch_max=256, seed=0):
        self.trick = dict(TRICK_DEFAULT, **(trick or {}))
        self.agent_ids = list(dim_info.keys())
        self._od = [int(dim_info[a][0]) for a in self.agent_ids]
        self._ad = [int(dim_info[a][1]) for a in self.agent_ids]
        hip_id, self.device = resolve_device(device)
        self.horizon = int(horizon)
        self.is_continue = is_continue
        self.num_agents = len(self.agent_ids)
        stored = self._stored = sum(self._ad) if is_continue else self.num_agents
        self._e = Engine(self._algo, self._od, self._ad, max(self.horizon, 2), hidden=hidden, batch_max=max(minibatch_max, 1),
                         extra_cols=stored + self.num_agents + self._mask_cols + self._state_dim, discrete=not is_continue, device_id=hip_id,
                         seed=seed, state_dim=self._state_dim, state_rows=self._state_rows)
        self._e.net_norm_set(self.trick["feature_norm"], self.trick["LayerNorm"])
        self.agents, self.buffers = {}, {}
        for j, aid in enumerate(self.agent_ids):
            self.agents[aid] = Agent(self._e, j, self._od[j], self._ad[j], self._critic_in(j), is_continue, self.trick, hidden)
            self._optimizers(self.agents[aid], j, actor_lr, critic_lr)
            self.buffers[aid] = AgentBuffer(self._e, j, self.device, self.horizon)
        if self.trick["lr_decay"]:
            self.actor_lr, self.critic_lr = actor_lr, critic_lr
        self._rng = rng
        self._rec = np.zeros(self._e.width, dtype=F32)
        self.last_trace = None

    def select_action(self, obs):
        actions, log_pis = {}, {}
        for j, aid in enumerate(self.agent_ids):
            o = np.asarray(obs[aid], dtype=F32).reshape(1, 1, -1)
            if self.is_continue:                 # Normal(mean, std).sample(): one randn draw of the mean's shape
                eps = torch.randn(1, self._ad[j]).numpy()
                a, lp = self._e.act(2 * j, N.ACT_PPO_SAMPLE, o, eps=eps, out_dim=self._ad[j], want_logp=True)
                actions[aid], log_pis[aid] = a[0, 0], lp[0, 0]
            else:                                # Categorical(probs).sample(): argmax(p / q), q ~ Exp(1)
                q = torch.empty(1, self._ad[j]).exponential_(1).numpy()
                a, lp = self._e.act(2 * j, N.ACT_CAT_SAMPLE, o, eps=q, want_logp=True)
                actions[aid], log_pis[aid] = np.int64(a[0, 0, 0]), np.float32(lp[0, 0, 0])
        return actions, log_pis

    def evaluate_action(self, obs):
        actions = {}
        for j, aid in enumerate(self.agent_ids):
            o = np.asarray(obs[aid], dtype=F32).reshape(1, 1, -1)
            if self.is_continue:
                actions[aid] = self._e.act(2 * j, N.ACT_TANHHEAD, o, out_dim=self._ad[j])[0, 0]
            else:
                actions[aid] = np.int64(self._e.act(2 * j, N.ACT_ARGMAX, o)[0, 0, 0])
        return actions

    def add(self, obs, action, reward, next_obs, done, action_log_pi, adv_dones):
        """Every agent's buffer is written in lock-step: one joint record [obs | act | rew | done | next_obs | log-probs | adv_done]"""
        lay, r = self._e.layout, self._rec
        lp = lay.extra_off
        for j, aid in enumerate(self.agent_ids):
            r[lay.obs_off[j]:lay.obs_off[j] + lay.obs_dim[j]] = np.asarray(obs[aid], dtype=F32).reshape(-1)
            r[lay.act_off[j]:lay.act_off[j] + lay.act_dim[j]] = np.asarray(action[aid], dtype=F32).reshape(-1)
            r[lay.rew_off + j] = reward[aid]
            r[lay.done_off + j] = float(done[aid])
            r[lay.next_obs_off[j]:lay.next_obs_off[j] + lay.obs_dim[j]] = np.asarray(next_obs[aid], dtype=F32).reshape(-1)
            r[lp:lp + lay.act_dim[j]] = np.asarray(action_log_pi[aid], dtype=F32).reshape(-1)
            lp += lay.act_dim[j]
            r[lay.extra_off + self._stored + j] = float(adv_dones[aid])
        self._e.add(0, r)

    def _learn(self, minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta, **opt):
        perms = None
        if self._rng != "device":                # one np.random.permutation per (agent, epoch), agent-major
            perms = np.stack([np.stack([np.random.permutation(self.horizon) for _ in range(K_epochs)]) for _ in self.agent_ids])[None]
        out = self._e.mappo_learn(self.horizon, minibatch_size, K_epochs, gamma=gamma, lmbda=lmbda, clip=clip_param,
                                  ent_coef=entropy_coefficient, adv_norm=self.trick["adv_norm"], value_clip=self.trick["ValueClip"],
                                  huber_delta=huber_delta if self.trick["huber_loss"] else None, perms=perms,
                                  want_trace=getattr(self, "track_loss", False), **opt)
        self.last_trace = out.get("trace")

    def save(self, model_dir):
        torch.save({name: agent.actor.state_dict() for name, agent in self.agents.items()}, os.path.join(model_dir, self._file))

    @classmethod
    def load(cls, dim_info, is_continue, model_dir, trick=None):
        policy = cls(dim_info, is_continue=is_continue, actor_lr=0, critic_lr=0, horizon=0, device="cpu", trick=trick)
        data = torch.load(os.path.join(model_dir, cls._file))
        for agent_id, agent in policy.agents.items():
            agent.actor.load_state_dict(data[agent_id])
        return policy


class MAPPO(MultiAgentPPO):
    _algo = N.ALGO_MAPPO
    _file = "MAPPO.pth"

    def _critic_in(self, j):
        return sum(self._od)                     # the global observation (MAPPO.py:191)

    def _optimizers(self, agent, j, actor_lr, critic_lr):
        # ONE Adam over actor + critic parameters: lr = actor_lr, eps 1e-5 (MAPPO.py:229-230).  Adam is elementwise, so the engine's two
        # per-net steps with these settings are that step; the view stands for both nets (its step count: the actor's)
        agent.ac_optimizer = OptimizerView(self._e, 2 * j, actor_lr, eps=1e-5)

    def learn(self, minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta=None):
        lr = self.agents[self.agent_ids[0]].ac_optimizer.lr
        self._learn(minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta, actor_lr=lr, critic_lr=lr,
                    adam_eps=1e-5, clip_norm=0.0)

    def lr_decay(self, episode_num, max_episodes):
        raise NotImplementedError("MAPPO.lr_decay reads agent.actor_optimizer (MAPPO_file/MAPPO.py:488), which MAPPO.py's Agent does not "
                                  "have: the reference raises AttributeError there, and its script forces the trick off")
