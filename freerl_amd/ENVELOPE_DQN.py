"""`ENVELOPE` (envelope multi-objective Q-learning, Yang et al. 2019) with the reference's class surface
(ENVELOPE_MORL_file/ENVELOPE_DQN.py:77-278), backed by the HIP engine.

    policy = ENVELOPE(dim_info=[obs_dim, action_dim, reward_dim], is_continue, Qnet_lr, buffer_size, device, beta, max_episodes)
    policy.select_action(obs) / evaluate_action(obs, preference)
    policy.add(obs, action, reward, next_obs, done, gamma) / sample(batch_size)
    policy.learn(batch_size, gamma, tau, weight_num, update_freq) / update_target(tau) / .loss / .beta / .priority_mem
    policy.save(model_dir) / ENVELOPE.load(dim_info, is_continue, model_dir)

`learn()` is one launch chain over batch_size x weight_num rows (kernels_envelope.hip); the replay ring, both nets and Adam's state
stay on the GPU.  What the reference does on the host stays on the host, call for call, so that a seeded run consumes the same
draws: the preferences of `select_action` and `add` come from `torch.randn`, the sampled rows (`np.random.choice` over the
priorities) and `learn()`'s weights (`np.random.randn`) from NumPy's global stream, and the homotopy on `beta` is the reference's
Python-float arithmetic.  `add()` runs its two forwards (on obs and next_obs) as the two rows of one `frl_act` call.

`max_rows` is the engine's batch_max: the most rows (batch_size x weight_num) one `learn()` may use; the default is the script's
256 x 128.

Reference behaviour kept as it is: `clip_grad_norm_` runs before `backward()` and clips nothing, so there is no
clipping; once the ring wraps, `priority_mem` (a deque, oldest first) and the ring's slots fall out of step, and `sample` pairs
them by position all the same; `update_freq` is unused.  One defect is an error here: `is_continue=True` (the reference prints a
message and fails on an unbound name) raises ValueError.
"""
import os
from collections import deque

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, OptimizerView, init_layers, resolve_device
from .Buffer import MO_Buffer

HIDDEN = 256        # MLP's default widths (ENVELOPE_DQN.py:37)


class EnvelopeNet(DeviceNet):
    """`agent.Qnet` / `agent.Qnet_target` (MLP, ENVELOPE_DQN.py:36-59): Qnet(obs, preference) -> [rows, action_dim, reward_dim]."""

    def __init__(self, engine, layers, action_dim, reward_dim, kind=N.PARAM_ONLINE):
        super().__init__(engine, 0, layers, kind=kind)
        self.action_dim, self.reward_dim = action_dim, reward_dim

    def __call__(self, obs, preference):
        return super().__call__(obs, preference).reshape(-1, self.action_dim, self.reward_dim)


class Agent:
    """Agent (ENVELOPE_DQN.py:62-74): Qnet, Qnet_target (a deep copy), Adam(Qnet.parameters(), lr)."""

    def __init__(self, engine, obs_dim, action_dim, reward_dim, Qnet_lr, hidden):
        layers = [("l1", hidden, obs_dim + reward_dim), ("l2", hidden, hidden), ("l3", action_dim * reward_dim, hidden)]
        flat = init_layers(layers)                                      # torch RNG: l1, l2, l3
        engine.set_params(0, flat, N.PARAM_ONLINE)
        engine.set_params(0, flat, N.PARAM_TARGET)
        self.Qnet = EnvelopeNet(engine, layers, action_dim, reward_dim)
        self.Qnet_target = EnvelopeNet(engine, layers, action_dim, reward_dim, kind=N.PARAM_TARGET)
        self.Qnet_optimizer = OptimizerView(engine, 0, Qnet_lr)

    def update_Qnet(self, loss):
        raise NotImplementedError("zero_grad/backward/step are fused into ENVELOPE.learn() on the GPU")


def _random_preference(reward_dim):
    """torch.randn(reward_dim), |.| / L1 norm (ENVELOPE_DQN.py:110-111, 158-159)."""
    preference = torch.randn(reward_dim)
    return torch.abs(preference) / torch.norm(preference, p=1)


def _prioritised_draw(total_size, priority_mem, batch_size):
    """np.random.choice without replacement, p proportional to the priorities (ENVELOPE_DQN.py:191-195, ENVELOPE_DDPG.py:241-245)."""
    batch_size = min(total_size, batch_size)
    priority_mem = np.array(priority_mem)
    return np.random.choice(range(total_size), batch_size, replace=False, p=priority_mem / priority_mem.sum())


class ENVELOPE:
    def __init__(self, dim_info, is_continue, Qnet_lr, buffer_size, device, beta, max_episodes, trick=None, *, hidden=HIDDEN,
                 max_rows=256 * 128, seed=0):
        obs_dim, action_dim, reward_dim = dim_info
        if is_continue:
            raise ValueError("ENVELOPE takes the argmax over discrete actions (ENVELOPE_DQN.py:116-124): a continuous "
                             "environment goes through the script's dis_to_con mapping with is_continue=False")
        hip_id, self.device = resolve_device(device)
        cap = max(int(buffer_size), 1)
        self._e = Engine(N.ALGO_ENVELOPE_DQN, obs_dim, action_dim, cap, discrete=True, hidden=hidden, batch_max=int(max_rows),
                         device_id=hip_id, seed=seed, reward_dim=reward_dim)
        self.agent = Agent(self._e, obs_dim, action_dim, reward_dim, Qnet_lr, hidden)
        self.buffer = MO_Buffer(cap, obs_dim, 1, reward_dim, self.device, _engine=self._e)
        self.is_continue = is_continue
        self.obs_dim = obs_dim
        self.reward_dim = reward_dim
        self.action_dim = action_dim
        self.priority_mem = deque(maxlen=int(buffer_size))
        self.update_cnt = 0
        # the homotopy on beta (:91-97)
        self.homotopy = True
        self.beta = beta
        self.beta_init = beta
        self.beta_uplim = 1.00
        self.tau = 1000.
        self.beta_expbase = float(np.power(self.tau * (self.beta_uplim - self.beta), 1. / max_episodes))
        self.beta_delta = self.beta_expbase / self.tau
        self.loss = None

    # ------------------------------------------------------------------ acting
    def _q(self, obs_rows, preference):
        """Q(obs, w) of the online net for each row of `obs_rows` under one preference -> torch [rows, action_dim, reward_dim]."""
        x = np.asarray(obs_rows, dtype=np.float32).reshape(-1, self.obs_dim)
        w = np.broadcast_to(preference.numpy().reshape(1, -1), (x.shape[0], self.reward_dim))
        out = self._e.act(0, N.ACT_RAW, np.concatenate([x, w], axis=1)[None], out_dim=self.action_dim * self.reward_dim)
        return torch.from_numpy(out[0]).reshape(-1, self.action_dim, self.reward_dim)

    def select_action(self, obs):
        """A fresh random preference, then argmax_a w . Q(obs, w)[a] (:102-125)."""
        return self.evaluate_action(obs, _random_preference(self.reward_dim))

    def evaluate_action(self, obs, preference):
        preference = torch.as_tensor(preference, dtype=torch.float32).reshape(1, -1)
        q = self._q(obs, preference[0]).reshape(-1, self.reward_dim)        # action_dim x reward_dim
        q = q @ preference.reshape(-1, 1)
        return q.argmax().numpy()

    # ------------------------------------------------------------------ buffer
    def add(self, obs, action, reward, next_obs, done, gamma):
        """Store the transition and push its priority |w.r + gamma w.Q(s')[a*] - w.Q(s)[a]| + 1e-5 under a fresh random
        preference (:139-188); `done` here is `terminated`, and advances the homotopy on beta."""
        self.buffer.add(obs, action, reward, next_obs, done)
        preference = _random_preference(self.reward_dim)
        rows = [obs] if done else [obs, next_obs]
        qs = self._q(np.stack([np.asarray(r, dtype=np.float32).reshape(-1) for r in rows]), preference)
        wq = preference.dot(qs[0, int(action)])
        wr = preference.dot(torch.as_tensor(np.asarray(reward), dtype=torch.float32).reshape(-1))
        if not done:
            reQ_ext = qs[1]                                                     # action_dim x reward_dim
            prod = reQ_ext @ preference
            hq = reQ_ext[torch.argmax(prod)]
            p = abs(wr + gamma * preference.dot(hq) - wq)
        else:
            if self.homotopy:
                self.beta += self.beta_delta
                self.beta_delta = (self.beta - self.beta_init) * self.beta_expbase + self.beta_init - self.beta
            p = abs(wr - wq)
        p += 1e-5
        self.priority_mem.append(p.numpy())

    def _draw(self, batch_size):
        return _prioritised_draw(len(self.buffer), self.priority_mem, batch_size)

    def sample(self, batch_size):
        """Rows drawn without replacement with probability proportional to `priority_mem` (:191-200)."""
        return self.buffer.sample(self._draw(batch_size))

    # ------------------------------------------------------------------ learn
    def learn(self, batch_size, gamma, tau, weight_num, update_freq):
        """One envelope update on batch_size x weight_num rows, then the soft target update (:204-255)."""
        indices = self._draw(batch_size)
        self.last_indices = indices
        w_batch = np.random.randn(weight_num, self.reward_dim)
        w_batch = np.abs(w_batch) / np.linalg.norm(w_batch, ord=1, axis=1, keepdims=True)
        self.last_weights = w_batch.astype(np.float32)
        out = self._e.envelope_learn(indices.size, weight_num, gamma=gamma, tau=tau, lr=self.agent.Qnet_optimizer.lr,
                                     beta=self.beta, idx=indices, weights=self.last_weights, want_loss=True)
        self.loss = torch.tensor(out["loss"][0])

    def update_target(self, tau):
        """theta_target = tau * theta + (1 - tau) * theta_target (:257-266); learn() already does this on the device."""
        th = self._e.get_params(0, N.PARAM_ONLINE)
        tg = self._e.get_params(0, N.PARAM_TARGET)
        self._e.set_params(0, tg * np.float32(1.0 - tau) + th * np.float32(tau), N.PARAM_TARGET)

    def soft_update(self, target, source, tau):
        if target is not self.agent.Qnet_target or source is not self.agent.Qnet:
            raise ValueError("soft_update moves agent.Qnet_target towards agent.Qnet")
        self.update_target(tau)

    # ------------------------------------------------------------------ checkpoints
    def save(self, model_dir):
        torch.save(self.agent.Qnet.state_dict(), os.path.join(model_dir, "ENVELOPE_DQN.pt"))

    @staticmethod
    def load(dim_info, is_continue, model_dir, trick=None, **kw):
        policy = ENVELOPE(dim_info, is_continue, 0, 0, device=torch.device("cpu"), trick=trick, beta=0, max_episodes=1, **kw)
        policy.agent.Qnet.load_state_dict(torch.load(os.path.join(model_dir, "ENVELOPE_DQN.pt")))
        return policy
