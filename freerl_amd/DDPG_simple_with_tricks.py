"""`DDPG` with PopArt (Preserving Outputs Precisely while Adaptively Rescaling Targets, van Hasselt et al. 2016) with the reference's
class surface (DDPG_file/DDPG_simple_with_tricks.py:95-304), backed by the HIP engine.

    policy = DDPG(dim_info=[obs_dim, action_dim], is_continue, actor_lr, critic_lr, buffer_size, device, trick={'popart': True})
    policy.select_action(obs) / evaluate_action(obs)
    policy.add(obs, action, reward, next_obs, done) / sample(batch_size)
    policy.learn(batch_size, gamma, tau) / update_target(tau)
    policy.agent.actor / .critic / .actor_target / .critic_target / .critic_PopArt
    policy.save(model_dir) / DDPG.load(dim_info, is_continue, model_dir, trick)

`learn()` is one launch chain (kernels_popart.hip): the TD targets under the old statistics, the statistics' step and the popped upper
layer, the lower critic's and the upper layer's steps, the actor's step through both, the soft updates.  The nets, the upper layer
{W, b}, the statistics {sigma, mu, nu} and every Adam state stay on the GPU; `agent.critic_PopArt` reads and writes them there.

`trick['popart']` false (or `trick` None) is DDPG_simple's update with clip_grad_norm_ 0.5: the class then IS `freerl_amd.DDPG.DDPG`.

Departures (DESIGN.md "PopArt DDPG"): `is_continue=False` raises ValueError (the reference reaches `self.agent.argmax`, which does not
exist); a call whose `nu - mu_new^2` is not positive keeps `sigma` instead of dividing by zero; `PopArt.__init__`'s module-global `device` is not
needed.
"""
import os

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, OptimizerView, draw_indices, host_draw, init_layers, resolve_device
from .Buffer import Buffer
from .TD3 import DDPG as _PlainDDPG
from .TD3 import actor_layers, critic_layers

HIDDEN = 128        # Actor's / Critic's default widths (DDPG_simple_with_tricks.py:45,59)
BETA, UPPER_LR = 0.99999, 1e-3      # PopArt.beta, PopArt.lr (:119-120)


class _Scalar:
    """`upper_layer.output_linear.weight` / `.bias`: one float of the learner's PopArt block, shaped as nn.Linear(1, 1) has it."""

    def __init__(self, engine, slot, shape):
        self._e, self._slot, self._shape = engine, slot, shape

    @property
    def data(self):
        return torch.full(self._shape, float(self._e.popart_get()[self._slot]))

    @data.setter
    def data(self, value):
        v = self._e.popart_get()
        v[self._slot] = float(torch.as_tensor(value).reshape(-1)[0])
        self._e.popart_set(v)

    def detach(self):
        return self.data


class _OutputLinear:
    def __init__(self, engine):
        self.weight, self.bias = _Scalar(engine, 0, (1, 1)), _Scalar(engine, 1, (1,))


class UpperLayer:
    """UpperLayer (:95-104): nn.Linear(1, 1), W = 1 and b = 0 at first."""

    def __init__(self, engine):
        self._e = engine
        self.output_linear = _OutputLinear(engine)

    def __call__(self, x):
        v = self._e.popart_get()
        return torch.as_tensor(x) * float(v[0]) + float(v[1])

    forward = __call__

    def state_dict(self):
        return {"output_linear.weight": self.output_linear.weight.data, "output_linear.bias": self.output_linear.bias.data}


class PopArt:
    """PopArt (:106-187) as the caller sees it: the statistics, the upper layer, normalize / denormalize and the two outputs.  art, pop,
    update_stats, backward and step are inside DDPG.learn() on the GPU."""

    def __init__(self, engine, lower, lower_target, critic_lr):
        self._e = engine
        self.mode = "POPART"
        self.lower_layers, self.lower_layers_target = lower, lower_target
        self.upper_layer = UpperLayer(engine)
        self.beta, self.lr = BETA, UPPER_LR
        self.opt_lower = OptimizerView(engine, 1, critic_lr)

    def _stat(self, slot):
        return torch.tensor(float(self._e.popart_get()[slot]), dtype=torch.float)

    sigma = property(lambda self: self._stat(2))
    mu = property(lambda self: self._stat(3))
    nu = property(lambda self: self._stat(4))

    def normalize(self, y):
        return (torch.as_tensor(y) - self.mu) / self.sigma

    def denormalize(self, y):
        return self.sigma * torch.as_tensor(y) + self.mu

    def output(self, x, u):
        return self.upper_layer(self.lower_layers(x, u))

    def output_target(self, x, u):
        return self.upper_layer(self.lower_layers_target(x, u))

    def forward(self, o, a, y):
        raise NotImplementedError("art / pop / backward / step are fused into DDPG.learn() on the GPU")


class Agent:
    """Agent (:189-213) with trick['popart']: actor, critic (PopArt's lower layers), their targets, critic_PopArt."""

    def __init__(self, engine, obs_dim, action_dim, dim_info, actor_lr, critic_lr, hidden):
        al, cl = actor_layers(obs_dim, action_dim, hidden), critic_layers(sum(dim_info), hidden, False)
        fa = init_layers(al)            # torch RNG order: actor l1..l3, critic l1..l3 (:191-192), then the upper layer's Linear(1, 1) (:113)
        fc = init_layers(cl)
        torch.nn.Linear(1, 1)           # (drawn, then overwritten by ones_ / zeros_: :98-101)
        for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
            engine.set_params(0, fa, kind)
            engine.set_params(1, fc, kind)
        self.actor = DeviceNet(engine, 0, al, act_mode=N.ACT_TANHHEAD)
        self.critic = DeviceNet(engine, 1, cl)
        self.actor_optimizer = OptimizerView(engine, 0, actor_lr)
        self.actor_target = DeviceNet(engine, 0, al, kind=N.PARAM_TARGET, act_mode=N.ACT_TANHHEAD)
        self.critic_target = DeviceNet(engine, 1, cl, kind=N.PARAM_TARGET)
        self.critic_PopArt = PopArt(engine, self.critic, self.critic_target, critic_lr)

    def update_actor(self, loss):
        raise NotImplementedError("zero_grad/backward/clip/step are fused into DDPG.learn() on the GPU")

    update_critic = update_actor


class DDPG:
    def __new__(cls, dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick=None, **kw):
        if not (trick or {}).get("popart"):      # DDPG_simple's update (:261-271, :277-278) with the 0.5 clip of update_actor / update_critic
            plain = _PlainDDPG(dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick=trick, **kw)
            return plain
        return super().__new__(cls)

    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick=None, *, hidden=HIDDEN, batch_max=1024,
                 seed=0, rng="auto"):
        obs_dim, action_dim = dim_info
        if not is_continue:
            raise ValueError("DDPG's actor outputs a continuous action; with is_continue=False the reference's select_action reaches "
                             "self.agent.argmax, which does not exist (DDPG_simple_with_tricks.py:233)")
        if rng not in ("auto", "host", "device"):
            raise ValueError("rng must be 'auto', 'host' or 'device', got %r" % (rng,))
        hip_id, self.device = resolve_device(device)
        self._e = Engine(N.ALGO_DDPG_POPART, obs_dim, action_dim, max(int(buffer_size), 1), hidden=hidden, batch_max=int(batch_max),
                         device_id=hip_id, seed=seed)
        self.agent = Agent(self._e, obs_dim, action_dim, dim_info, actor_lr, critic_lr, hidden)
        self.buffer = Buffer(buffer_size, obs_dim, act_dim=action_dim, device=self.device, _engine=self._e)
        self.is_continue = is_continue
        self.trick = trick
        self._rng = rng
        self._act_dim = action_dim
        self.last_out = None          # learn()'s statistics, in the order of _native.POPART_OUT
        self.last_indices = None      # the rows of the last host-drawn batch

    # ------------------------------------------------------------------ acting
    def select_action(self, obs):
        """actor(obs) in (-1, 1), float32 [action_dim] (:227-234)."""
        return self._e.act(0, N.ACT_TANHHEAD, np.asarray(obs, dtype=np.float32).reshape(1, 1, -1), out_dim=self._act_dim)[0, 0]

    def evaluate_action(self, obs):
        return self.select_action(obs)

    # ------------------------------------------------------------------ buffer
    def add(self, obs, action, reward, next_obs, done):
        self.buffer.add(obs, action, reward, next_obs, done)

    def sample(self, batch_size):
        return self.buffer.sample(draw_indices(len(self.buffer), batch_size))

    # ------------------------------------------------------------------ learn
    def learn(self, batch_size, gamma, tau):
        total = len(self.buffer)
        idx = None
        if host_draw(self._rng, total, batch_size):
            idx = self.last_indices = draw_indices(total, batch_size)      # np.random.choice (:247)
        pa = self.agent.critic_PopArt
        self.last_out = self._e.popart_ddpg_learn(batch_size, gamma=gamma, tau=tau, actor_lr=self.agent.actor_optimizer.lr,
                                                  critic_lr=pa.opt_lower.lr, upper_lr=pa.lr, beta=pa.beta, idx=idx)[0]

    def update_target(self, tau):
        """theta_target = tau * theta + (1 - tau) * theta_target for the lower critic and the actor (:283-292); learn() already does this on
        the device."""
        for net in (1, 0):
            th = self._e.get_params(net, N.PARAM_ONLINE)
            tg = self._e.get_params(net, N.PARAM_TARGET)
            self._e.set_params(net, tg * np.float32(1.0 - tau) + th * np.float32(tau), N.PARAM_TARGET)

    # ------------------------------------------------------------------ checkpoints
    def save(self, model_dir):
        torch.save(self.agent.actor.state_dict(), os.path.join(model_dir, "DDPG.pt"))

    @staticmethod
    def load(dim_info, is_continue, model_dir, trick=None, **kw):
        policy = DDPG(dim_info, is_continue, 0, 0, 0, device=torch.device("cpu"), trick=trick, **kw)
        policy.agent.actor.load_state_dict(torch.load(os.path.join(model_dir, "DDPG.pt")))
        return policy
