"""`MASAC` with the reference's class surface (MAAC_file/MASAC.py:141-302), backed by the HIP engine (FRL_ALGO_MASAC,
kernels_masac.hip): every agent's tanh-Gaussian actor (a `mean_layer` and a `log_std_layer` on a shared trunk), twin critic on
[all obs | all actions], their targets, ONE joint replay ring and one `Alpha` per agent live in one engine.  `learn` is the
reference's loop with entropy_way_c = entropy_way_a = action_way = '1' and adaptive alpha (its shipped settings): per agent, in
order, a fresh index draw, the critic step, the actor step through ALL online actors, the alpha step; then every target moves.

Host-RNG mode (`rng="host"`, or `"auto"` on a small buffer) consumes NumPy's and torch's global generators in the reference's
order — per updating agent one `np.random.choice`, n target-actor draws [B, A_j], n online-actor draws, one entropy draw — and
`select_action` one [1, A_j] draw per agent, so a seeded run follows a seeded reference run.

`is_continue=False` raises ValueError at construction: the reference constructs, then fails in `select_action` with
AttributeError (`Agent.argmax` does not exist, MASAC.py:185).  `MAAC.py` / `MAAC_discrete.py` (the attention critics built on this
class) are not ported."""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, F32, OptimizerView, host_draw, init_layers, resolve_device
from .Buffer import Buffer


def actor_layers(obs_dim, action_dim, hidden):
    """[(name, out, in)] of Actor (MASAC.py:32-38) in state_dict order; the engine stores the last two as one head of 2 A rows and
    takes / gives them in this order (frl_params_get / _set)."""
    return [("l1", hidden, obs_dim), ("l2", hidden, hidden), ("mean_layer", action_dim, hidden), ("log_std_layer", action_dim, hidden)]


def critic_layers(total_dim, hidden):
    """Critic (MASAC.py:72-83): Q1 then Q2"""
    return [("l1", hidden, total_dim), ("l2", hidden, hidden), ("l3", 1, hidden),
            ("l1_2", hidden, total_dim), ("l2_2", hidden, hidden), ("l3_2", 1, hidden)]


class ActorNet(DeviceNet):
    """`agent.actor` / `agent.actor_target`: called as the reference's module, `actor(obs, deterministic=False, with_logprob=True)`
    -> (action, log_pi); the draw comes from torch's generator ([rows, A], as Normal.rsample's)."""

    def __init__(self, engine, net, layers, act_dim, kind=N.PARAM_ONLINE):
        super().__init__(engine, net, layers, kind=kind, act_mode=N.ACT_RAW)
        self._A = act_dim

    def __call__(self, obs, deterministic=False, with_logprob=True):
        x = np.asarray(torch.as_tensor(obs).detach().cpu().numpy(), dtype=F32)
        head = self._e.act(self._net, N.ACT_RAW, x[None], out_dim=2 * self._A, use_target=(self._kind == N.PARAM_TARGET))[0]
        mean, log_std = torch.from_numpy(head[:, :self._A].copy()), torch.from_numpy(head[:, self._A:].copy()).clamp(-20, 2)
        std = log_std.exp()
        u = mean if deterministic else mean + std * torch.randn(mean.shape)
        log_pi = None
        if with_logprob:
            log_pi = torch.distributions.Normal(mean, std).log_prob(u).sum(dim=1, keepdim=True)
            log_pi = log_pi - (2 * (np.log(2) - u - torch.nn.functional.softplus(-2 * u))).sum(dim=1, keepdim=True)
        return torch.tanh(u), log_pi


class CriticNet(DeviceNet):
    """`agent.critic` / `agent.critic_target`: `critic(obs_list, act_list)` -> (q1, q2), each [rows, 1]"""

    def __call__(self, s, a):
        to_np = lambda ts: [np.asarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=F32) for t in ts]
        x = np.concatenate(to_np(list(s)) + to_np(list(a)), axis=1)
        tgt = self._kind == N.PARAM_TARGET
        return tuple(torch.from_numpy(self._e.act(self._net, N.ACT_RAW, x[None], out_dim=1, head=h, use_target=tgt)[0]) for h in (0, 1))


class Agent:
    """Agent (MASAC.py:99-121); torch RNG order: the actor's l1, l2, mean_layer, log_std_layer, then the critic's six layers."""

    def __init__(self, engine, j, obs_dim, action_dim, total_dim, actor_lr, critic_lr, hidden):
        al, cl = actor_layers(obs_dim, action_dim, hidden), critic_layers(total_dim, hidden)
        fa, fc = init_layers(al), init_layers(cl)
        for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
            engine.set_params(2 * j, fa, kind)
            engine.set_params(2 * j + 1, fc, kind)
        self.actor = ActorNet(engine, 2 * j, al, action_dim)
        self.critic = CriticNet(engine, 2 * j + 1, cl)
        self.actor_target = ActorNet(engine, 2 * j, al, action_dim, kind=N.PARAM_TARGET)
        self.critic_target = CriticNet(engine, 2 * j + 1, cl, kind=N.PARAM_TARGET)
        self.actor_optimizer = OptimizerView(engine, 2 * j, actor_lr)
        self.critic_optimizer = OptimizerView(engine, 2 * j + 1, critic_lr)


class Alpha:
    """Alpha (MASAC.py:124-139) of one agent: `.alpha`, `.log_alpha` read the engine's values, `.set(alpha)` writes them (and
    resets its Adam state)."""

    def __init__(self, engine, agent, action_dim, alpha_lr=0.0001, alpha=0.01):
        self._e, self._agent = engine, agent
        self.alpha_lr = alpha_lr
        self.target_entropy = -action_dim
        self.set(alpha)

    def set(self, alpha):
        la = np.float32(np.log(alpha))                   # torch.tensor(np.log(alpha), dtype=float32); .exp() in float32
        self._e.set_alpha_state_agent(self._agent, [la, 0.0, 0.0, float(torch.tensor(la).exp())], 0)

    @property
    def log_alpha(self):
        return torch.tensor(float(self._e.alpha_state_agent(self._agent)[0][0]))

    @property
    def alpha(self):
        return torch.tensor(float(self._e.alpha_state_agent(self._agent)[0][3]))


class MASAC:
    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick=None, *, rng="auto", hidden=128,
                 batch_max=1024, seed=0):
        if not is_continue:
            raise ValueError("MASAC: only continuous actions work in the reference (its discrete branch calls Agent.argmax, MASAC.py:185)")
        self.attention = False
        self.agent_ids = list(dim_info.keys())
        od = [dim_info[a][0] for a in self.agent_ids]
        ad = [dim_info[a][1] for a in self.agent_ids]
        hip_id, self.device = resolve_device(device)
        self._e = Engine(N.ALGO_MASAC, od, ad, max(int(buffer_size), 1), hidden=hidden, batch_max=batch_max, device_id=hip_id, seed=seed,
                         twin_critic=True)
        total = sum(od) + sum(ad)
        self.agents, self.buffers = {}, {}
        for j, aid in enumerate(self.agent_ids):
            self.agents[aid] = Agent(self._e, j, od[j], ad[j], total, actor_lr, critic_lr, hidden)
            self.buffers[aid] = Buffer(buffer_size, od[j], ad[j], self.device, _engine=self._e, _agent=j)
        self.adaptive_alpha = True
        self.alphas = {aid: Alpha(self._e, j, ad[j], alpha=0.01) for j, aid in enumerate(self.agent_ids)}
        self.entropy_way_c = self.entropy_way_a = self.action_way = "1"
        self.is_continue = is_continue
        self.agent_x = self.agent_ids[0]
        self._rng = rng
        self._ad = ad
        self._rec = np.zeros(self._e.width, dtype=F32)
        self.last_losses = None

    def select_action(self, obs):
        actions = {}
        for j, aid in enumerate(self.agent_ids):
            o = np.asarray(obs[aid], dtype=F32).reshape(1, 1, -1)
            eps = torch.randn(1, self._ad[j]).numpy()               # Normal.rsample's draw (MASAC.py:54)
            actions[aid] = self._e.act(2 * j, N.ACT_SAC_SAMPLE, o, eps=eps, out_dim=self._ad[j])[0, 0]
        return actions

    def evaluate_action(self, obs):
        actions = {}
        for j, aid in enumerate(self.agent_ids):
            o = np.asarray(obs[aid], dtype=F32).reshape(1, 1, -1)
            actions[aid] = self._e.act(2 * j, N.ACT_TANHHEAD, o, out_dim=self._ad[j])[0, 0]
        return actions

    def add(self, obs, action, reward, next_obs, done):
        """Every agent's buffer is written in lock-step (MASAC.py:201-203): one joint record."""
        lay, r = self._e.layout, self._rec
        for j, aid in enumerate(self.agent_ids):
            r[lay.obs_off[j]:lay.obs_off[j] + lay.obs_dim[j]] = np.asarray(obs[aid], dtype=F32).reshape(-1)
            r[lay.act_off[j]:lay.act_off[j] + lay.act_dim[j]] = np.asarray(action[aid], dtype=F32).reshape(-1)
            r[lay.rew_off + j] = reward[aid]
            r[lay.done_off + j] = float(done[aid])
            r[lay.next_obs_off[j]:lay.next_obs_off[j] + lay.obs_dim[j]] = np.asarray(next_obs[aid], dtype=F32).reshape(-1)
        self._e.add(0, r)

    def sample(self, batch_size):
        """(obs, action, reward, next_obs, done, next_action, next_log_pi) dicts for one index draw (MASAC.py:205-216)."""
        total = len(self.buffers[self.agent_x])
        indices = np.random.choice(total, batch_size, replace=False)
        obs, action, reward, next_obs, done, next_action, next_log_pi = {}, {}, {}, {}, {}, {}, {}
        for aid in self.agent_ids:
            obs[aid], action[aid], reward[aid], next_obs[aid], done[aid] = self.buffers[aid].sample(indices)
            next_action[aid], next_log_pi[aid] = self.agents[aid].actor_target(next_obs[aid])
        return obs, action, reward, next_obs, done, next_action, next_log_pi

    def learn(self, batch_size, gamma, tau):
        n, total = len(self.agent_ids), len(self.buffers[self.agent_x])
        idx = noise = None
        if host_draw(self._rng, total, batch_size):
            # the reference's draw order, per updating agent i (MASAC.py:224,254,261): one np.random.choice; one rsample per target
            # actor j; one per online actor j; the second forward of actor i
            am = max(self._ad)
            idx = np.zeros((1, n, batch_size), np.int64)
            noise = np.zeros((1, n, 2 * n + 1, batch_size, am), F32)
            for i in range(n):
                idx[0, i] = np.random.choice(total, batch_size, replace=False)
                for s in range(2 * n):
                    noise[0, i, s, :, :self._ad[s % n]] = torch.randn(batch_size, self._ad[s % n]).numpy()
                noise[0, i, 2 * n, :, :self._ad[i]] = torch.randn(batch_size, self._ad[i]).numpy()
        a0 = self.agents[self.agent_x]
        st = self._e.learn(batch_size, gamma=gamma, tau=tau, actor_lr=a0.actor_optimizer.lr, critic_lr=a0.critic_optimizer.lr,
                           alpha_lr=self.alphas[self.agent_x].alpha_lr, idx=idx, noise=noise, want_stats=getattr(self, "track_loss", False))
        if st is not None:
            self.last_losses = {aid: (float(st[0, j, N.STAT_CRITIC_LOSS]), float(st[0, j, N.STAT_ACTOR_LOSS]))
                                for j, aid in enumerate(self.agent_ids)}

    def update_target(self, tau):
        for net in range(self._e.n_nets):
            q, t = self._e.get_params(net, N.PARAM_ONLINE), self._e.get_params(net, N.PARAM_TARGET)
            self._e.set_params(net, t * np.float32(1.0 - tau) + q * np.float32(tau), N.PARAM_TARGET)

    def save(self, model_path):
        torch.save(OrderedDict((name, agent.actor.state_dict()) for name, agent in self.agents.items()), os.path.join(model_path, "MASAC.pth"))

    @staticmethod
    def load(dim_info, is_continue, model_dir, **kw):
        policy = MASAC(dim_info, is_continue=is_continue, actor_lr=0, critic_lr=0, buffer_size=0, device="cpu", **kw)
        data = torch.load(os.path.join(model_dir, "MASAC.pth"))
        for agent_id, agent in policy.agents.items():
            agent.actor.load_state_dict(data[agent_id])
        return policy
