"""`ENVELOPE_DDPG` (envelope multi-objective learning, Yang et al. 2019, on a deterministic actor-critic) with the reference's class
surface (ENVELOPE_MORL_file/ENVELOPE_DDPG.py:93-332), backed by the HIP engine.

    policy = ENVELOPE_DDPG(dim_info=[obs_dim, action_dim, reward_dim], is_continue, actor_lr, critic_lr, buffer_size, device, beta,
                           max_episodes)
    policy.select_action(obs) / evaluate_action(obs, preference)
    policy.add(obs, action, reward, next_obs, done, gamma) / sample(batch_size)
    policy.learn(batch_size, gamma, tau, weight_num, update_freq) / update_target(tau) / .loss / .beta / .priority_mem
    policy.save(model_dir) / ENVELOPE_DDPG.load(dim_info, is_continue, model_dir)

`learn()` is one launch chain over batch_size x weight_num rows (kernels_envelope_ddpg.hip): the critic step, the actor step through
the updated critic, both soft updates; the replay ring, the four nets and Adam's state stay on the GPU.  What the reference does on
the host stays on the host, call for call, so that a seeded run consumes the same draws: the preferences of `select_action` and
`add` come from `torch.randn`, the sampled rows (`np.random.choice` over the priorities) and `learn()`'s weights
(`np.random.randn`) from NumPy's global stream, and the homotopy on `beta` is the reference's Python-float arithmetic.

`max_rows` is the engine's batch_max: the most rows (batch_size x weight_num) one `learn()` may use; the default is the script's
256 x 128.

Reference behaviour kept as it is: the TD target takes a' from the ONLINE actor (:284), so `actor_target` is
maintained but never read; the actor's loss is the plain mean over the critic's objectives, not weighted by the preference
(:303); `update_freq` is unused; the priority deque and the ring fall out of step once the ring wraps.  One defect is an error
here: `is_continue=False` (the reference prints a message and fails on an unbound name) raises ValueError.
"""
import os
from collections import deque

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, OptimizerView, init_layers, resolve_device
from .Buffer import MO_Buffer
from .ENVELOPE_DQN import _prioritised_draw, _random_preference

HIDDEN = 256        # Actor's / Critic's default widths (ENVELOPE_DDPG.py:41,66)


class Agent:
    """Agent (ENVELOPE_DDPG.py:93-115): actor, critic, their Adam optimizers, and deep copies as targets."""

    def __init__(self, engine, obs_dim, action_dim, reward_dim, actor_lr, critic_lr, hidden):
        la = [("l1", hidden, obs_dim + reward_dim), ("l2", hidden, hidden), ("l3", action_dim, hidden)]
        lc = [("l1", hidden, obs_dim + action_dim + reward_dim), ("l2", hidden, hidden), ("l3", reward_dim, hidden)]
        for net, layers in ((0, la), (1, lc)):                          # torch RNG: actor l1-l3, then critic l1-l3
            flat = init_layers(layers)
            engine.set_params(net, flat, N.PARAM_ONLINE)
            engine.set_params(net, flat, N.PARAM_TARGET)
        self.actor = DeviceNet(engine, 0, la, act_mode=N.ACT_TANHHEAD)
        self.critic = DeviceNet(engine, 1, lc)
        self.actor_optimizer = OptimizerView(engine, 0, actor_lr)
        self.critic_optimizer = OptimizerView(engine, 1, critic_lr)
        self.actor_target = DeviceNet(engine, 0, la, kind=N.PARAM_TARGET, act_mode=N.ACT_TANHHEAD)
        self.critic_target = DeviceNet(engine, 1, lc, kind=N.PARAM_TARGET)

    def update_actor(self, loss):
        raise NotImplementedError("zero_grad/backward/clip/step are fused into ENVELOPE_DDPG.learn() on the GPU")

    update_critic = update_actor


class ENVELOPE_DDPG:
    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, beta, max_episodes, trick=None, *,
                 hidden=HIDDEN, max_rows=256 * 128, seed=0):
        obs_dim, action_dim, reward_dim = dim_info
        if not is_continue:
            raise ValueError("ENVELOPE_DDPG's actor outputs a continuous action (ENVELOPE_DDPG.py:159-167): discrete actions go "
                             "through ENVELOPE_DQN.ENVELOPE")
        hip_id, self.device = resolve_device(device)
        cap = max(int(buffer_size), 1)
        self._e = Engine(N.ALGO_ENVELOPE_DDPG, obs_dim, action_dim, cap, hidden=hidden, batch_max=int(max_rows), device_id=hip_id,
                         seed=seed, reward_dim=reward_dim)
        self.agent = Agent(self._e, obs_dim, action_dim, reward_dim, actor_lr, critic_lr, hidden)
        self.buffer = MO_Buffer(cap, obs_dim, action_dim, reward_dim, self.device, _engine=self._e)
        self.is_continue = is_continue
        self.obs_dim = obs_dim
        self.reward_dim = reward_dim
        self.action_dim = action_dim
        self.priority_mem = deque(maxlen=int(buffer_size))
        self.update_cnt = 0
        # the homotopy on beta (:132-138)
        self.homotopy = True
        self.beta = beta
        self.beta_init = beta
        self.beta_uplim = 1.00
        self.tau = 1000.
        self.beta_expbase = float(np.power(self.tau * (self.beta_uplim - self.beta), 1. / max_episodes))
        self.beta_delta = self.beta_expbase / self.tau
        self.loss = None
        self.actor_loss = None

    # ------------------------------------------------------------------ acting
    def select_action(self, obs):
        """A fresh random preference, then the actor's output under it (:143-167)."""
        return self.evaluate_action(obs, _random_preference(self.reward_dim))

    def evaluate_action(self, obs, preference):
        obs = torch.as_tensor(obs, dtype=torch.float32).reshape(1, -1)
        preference = torch.as_tensor(preference, dtype=torch.float32).reshape(1, -1)
        return self.agent.actor(obs, preference).numpy().squeeze(0)

    # ------------------------------------------------------------------ buffer
    def add(self, obs, action, reward, next_obs, done, gamma):
        """Store the transition and push its priority |w.r + gamma w.critic(s', actor(s', w), w) - w.critic(s, a, w)| + 1e-5 under a
        fresh random preference, on the ONLINE nets (:183-238); `done` here is `terminated`, and advances the homotopy on beta."""
        self.buffer.add(obs, action, reward, next_obs, done)
        preference = _random_preference(self.reward_dim)
        w = preference.reshape(1, -1)
        obs = torch.as_tensor(obs, dtype=torch.float32).reshape(1, -1)
        act = torch.as_tensor(action, dtype=torch.float32).reshape(1, -1)
        wr = preference.dot(torch.as_tensor(np.asarray(reward), dtype=torch.float32).reshape(-1))
        if not done:
            next_obs = torch.as_tensor(next_obs, dtype=torch.float32).reshape(1, -1)
            next_act = self.agent.actor(next_obs, w)
            q = self.agent.critic(torch.cat([obs, next_obs]), torch.cat([act, next_act]), w.repeat(2, 1))     # both rows in one launch
            wq = preference.dot(q[0])
            p = abs(wr + gamma * preference.dot(q[1]) - wq)
        else:
            wq = preference.dot(self.agent.critic(obs, act, w)[0])
            if self.homotopy:
                self.beta += self.beta_delta
                self.beta_delta = (self.beta - self.beta_init) * self.beta_expbase + self.beta_init - self.beta
            p = abs(wr - wq)
        p += 1e-5
        self.priority_mem.append(p.numpy())

    def _draw(self, batch_size):
        return _prioritised_draw(len(self.buffer), self.priority_mem, batch_size)

    def sample(self, batch_size):
        """Rows drawn without replacement with probability proportional to `priority_mem` (:241-250)."""
        return self.buffer.sample(self._draw(batch_size))

    # ------------------------------------------------------------------ learn
    def learn(self, batch_size, gamma, tau, weight_num, update_freq):
        """One critic step and one actor step on batch_size x weight_num rows, then both soft target updates (:254-308)."""
        indices = self._draw(batch_size)
        self.last_indices = indices
        w_batch = np.random.randn(weight_num, self.reward_dim)
        w_batch = np.abs(w_batch) / np.linalg.norm(w_batch, ord=1, axis=1, keepdims=True)
        self.last_weights = w_batch.astype(np.float32)
        out = self._e.envelope_ddpg_learn(indices.size, weight_num, gamma=gamma, tau=tau, actor_lr=self.agent.actor_optimizer.lr,
                                          critic_lr=self.agent.critic_optimizer.lr, beta=self.beta, idx=indices,
                                          weights=self.last_weights, want_loss=True)
        self.loss = torch.tensor(out["critic_loss"][0])
        self.actor_loss = torch.tensor(out["actor_loss"][0])

    def update_target(self, tau):
        """theta_target = tau * theta + (1 - tau) * theta_target for the critic and the actor (:310-316); learn() already does this
        on the device."""
        for net in (1, 0):
            th = self._e.get_params(net, N.PARAM_ONLINE)
            tg = self._e.get_params(net, N.PARAM_TARGET)
            self._e.set_params(net, tg * np.float32(1.0 - tau) + th * np.float32(tau), N.PARAM_TARGET)

    def soft_update(self, target, source, tau):
        pairs = {id(self.agent.critic_target): (self.agent.critic, 1), id(self.agent.actor_target): (self.agent.actor, 0)}
        src, net = pairs.get(id(target), (None, None))
        if src is None or source is not src:
            raise ValueError("soft_update moves agent.critic_target towards agent.critic, or agent.actor_target towards agent.actor")
        th = self._e.get_params(net, N.PARAM_ONLINE)
        tg = self._e.get_params(net, N.PARAM_TARGET)
        self._e.set_params(net, tg * np.float32(1.0 - tau) + th * np.float32(tau), N.PARAM_TARGET)

    # ------------------------------------------------------------------ checkpoints
    def save(self, model_dir):
        torch.save(self.agent.actor.state_dict(), os.path.join(model_dir, "ENVELOPE_DDPG.pt"))

    @staticmethod
    def load(dim_info, is_continue, model_dir, trick=None, **kw):
        policy = ENVELOPE_DDPG(dim_info, is_continue, 0, 0, 0, device=torch.device("cpu"), trick=trick, beta=0, max_episodes=1, **kw)
        policy.agent.actor.load_state_dict(torch.load(os.path.join(model_dir, "ENVELOPE_DDPG.pt")))
        return policy
