"""`SAC` with the reference's class surface (SAC_file/SAC.py:129-282), backed by the HIP engine.

    SAC(dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick)   # trick dict required (SAC.py:181)

`is_continue=False` builds SAC_file/SAC_add_discrete.py's discrete SAC (its `hands_on` networks, :137-177): a softmax
actor, twin critics with one value per action, Categorical sampling (kernels_sacd.hip).  Two reference defects handled:
its `learn()` branches on a module-global `is_continue` that only exists when the script runs as `__main__` (here the
instance's flag decides), and its discrete `evaluate_action` (:266-268) hands the raw ndarray to the actor and raises
(here: the argmax of the probabilities, without Batch_ObsNorm, as the continuous branch does).
"""
import os

import numpy as np
import torch

from . import _native as N
from ._core import BatchObsNormView, DeviceNet, Engine, OptimizerView, draw_indices, host_draw, init_layers, resolve_device
from .Buffer import Buffer
from .TD3 import critic_layers


class Agent:
    def __init__(self, engine, obs_dim, action_dim, dim_info, actor_lr, critic_lr, hidden):
        al = [("l1", hidden, obs_dim), ("l2", hidden, hidden), ("mean_layer", action_dim, hidden)]
        cl = critic_layers(sum(dim_info), hidden, True)
        fa = np.concatenate([init_layers(al), np.zeros(action_dim, np.float32)])   # log_std = zeros (SAC.py:66)
        fc = init_layers(cl)
        for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
            engine.set_params(0, fa, kind)
            engine.set_params(1, fc, kind)
        extra = ("log_std", (1, action_dim))
        self.actor = DeviceNet(engine, 0, al, extra=extra, act_mode=N.ACT_TANHHEAD)
        self.critic = DeviceNet(engine, 1, cl)
        self.actor_target = DeviceNet(engine, 0, al, extra=extra, kind=N.PARAM_TARGET, act_mode=N.ACT_TANHHEAD)
        self.critic_target = DeviceNet(engine, 1, cl, kind=N.PARAM_TARGET)
        self.actor_optimizer = OptimizerView(engine, 0, actor_lr)
        self.critic_optimizer = OptimizerView(engine, 1, critic_lr)

    def update_actor(self, loss):
        raise NotImplementedError("zero_grad/backward/clip/step are fused into learn() on the GPU")

    update_critic = update_actor


class SoftmaxNet(DeviceNet):
    """`agent.actor` of the discrete SAC (Actor_discrete_hands_on, SAC_add_discrete.py:137-150): calling it returns the
    action probabilities, softmax of the head's logits."""

    def __call__(self, *inputs):
        return torch.softmax(super().__call__(*inputs), dim=1)


class AgentDiscrete:
    """Agent of SAC_add_discrete.py (:179-207) with the hands_on nets: actor l1..l3, critic l1..l6 (two heads on obs only)."""

    def __init__(self, engine, obs_dim, action_dim, actor_lr, critic_lr, hidden):
        al = [("l1", hidden, obs_dim), ("l2", hidden, hidden), ("l3", action_dim, hidden)]
        cl = [("l1", hidden, obs_dim), ("l2", hidden, hidden), ("l3", action_dim, hidden),
              ("l4", hidden, obs_dim), ("l5", hidden, hidden), ("l6", action_dim, hidden)]
        fa = init_layers(al)                                             # actor first, then critic (:185-187)
        fc = init_layers(cl)
        for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):                    # deepcopy targets (:192-193)
            engine.set_params(0, fa, kind)
            engine.set_params(1, fc, kind)
        self.actor = SoftmaxNet(engine, 0, al)
        self.critic = DeviceNet(engine, 1, cl)
        self.actor_target = SoftmaxNet(engine, 0, al, kind=N.PARAM_TARGET)
        self.critic_target = DeviceNet(engine, 1, cl, kind=N.PARAM_TARGET)
        self.actor_optimizer = OptimizerView(engine, 0, actor_lr)
        self.critic_optimizer = OptimizerView(engine, 1, critic_lr)

    def update_actor(self, loss):
        raise NotImplementedError("zero_grad/backward/clip/step are fused into learn() on the GPU")

    update_critic = update_actor


class Alpha:
    """Alpha (SAC.py:154-169): log_alpha scalar + Adam(lr 1e-4); `.alpha` reads the engine's value."""

    def __init__(self, engine, action_dim, alpha_lr=0.0001, alpha=0.2, is_continue=True):
        self._e = engine
        self.alpha_lr = alpha_lr
        if is_continue:
            self.target_entropy = -action_dim                            # SAC.py:160
        else:                                                            # SAC_add_discrete.py:218: a float32 tensor
            self.target_entropy = 0.6 * (-torch.log(torch.tensor(1.0 / action_dim)))
        engine.set_alpha_state([np.log(alpha), 0.0, 0.0, alpha], 0)

    @property
    def log_alpha(self):
        return torch.tensor(float(self._e.alpha_state()[0][0]))

    @property
    def alpha(self):
        return torch.tensor(float(self._e.alpha_state()[0][3]))


class SAC:
    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick=None, *, rng="auto",
                 hidden=128, batch_max=1024, seed=0):
        obs_dim, action_dim = dim_info
        if trick is None:
            raise TypeError("SAC needs the `trick` dict (the reference indexes it, SAC.py:181)")
        hip_id, self.device = resolve_device(device)
        algo = N.ALGO_SAC if is_continue else N.ALGO_SAC_DISCRETE
        self._e = Engine(algo, obs_dim, action_dim, max(int(buffer_size), 1), twin_critic=True, hidden=hidden,
                         batch_max=batch_max, device_id=hip_id, seed=seed)
        if is_continue:
            self.agent = Agent(self._e, obs_dim, action_dim, dim_info, actor_lr, critic_lr, hidden)
        else:
            self.discrete_type = {"hands_on": True, "other": False}    # SAC_add_discrete.py:231-233
            self.agent = AgentDiscrete(self._e, obs_dim, action_dim, actor_lr, critic_lr, hidden)
        # Buffer act_dim: the action width, or 1 (the stored index) for discrete actions (SAC_add_discrete.py:236)
        self.buffer = Buffer(buffer_size, obs_dim, act_dim=action_dim if is_continue else 1, device=self.device, _engine=self._e)
        self.is_continue = is_continue
        self.trick = trick
        if trick.get("Batch_ObsNorm"):                                   # SAC.py:181-182
            self._e.obsnorm_enable(True)
            self.batch_size_obs_norm = BatchObsNormView(self._e)
        self.adaptive_alpha = True                                       # SAC.py:185
        self.alphas = Alpha(self._e, action_dim, alpha=0.01, is_continue=is_continue)   # SAC.py:188
        self._rng = rng
        self._act_dim = action_dim
        self.last_losses = None

    def select_action(self, obs):
        """tanh(mean + std*eps), eps from torch's generator like Normal.rsample (SAC.py:192-198).  Discrete:
        Categorical(probs).sample() (SAC_add_discrete.py:249-259), which draws `empty(1, nA).exponential_(1)` and takes
        argmax(p / q)."""
        if not self.is_continue:
            q = torch.empty(1, self._act_dim).exponential_(1).numpy()
            a = self._e.act(0, N.ACT_CAT_SAMPLE, np.asarray(obs, dtype=np.float32).reshape(1, 1, -1), eps=q)
            return np.int64(a[0, 0, 0])
        eps = torch.randn(1, self._act_dim).numpy() if self._rng != "device" else \
            np.random.default_rng().standard_normal((1, self._act_dim)).astype(np.float32)
        return self._e.act(0, N.ACT_SAC_SAMPLE, np.asarray(obs, dtype=np.float32).reshape(1, 1, -1), eps=eps,
                           out_dim=self._act_dim)[0, 0]

    def evaluate_action(self, obs):                                      # tanh(mean) (SAC.py:200-204)
        if not self.is_continue:                  # argmax of the probabilities (SAC_add_discrete.py:266-268, see the module doc)
            return np.int64(self._e.act(0, N.ACT_ARGMAX, np.asarray(obs, dtype=np.float32).reshape(1, 1, -1),
                                        normalize=False)[0, 0, 0])
        return self._e.act(0, N.ACT_TANHHEAD, np.asarray(obs, dtype=np.float32).reshape(1, 1, -1), out_dim=self._act_dim,
                           normalize=False)[0, 0]        # the reference does not apply Batch_ObsNorm here

    def add(self, obs, action, reward, next_obs, done):
        self.buffer.add(obs, action, reward, next_obs, done)

    def sample(self, batch_size):
        return self.buffer.sample(draw_indices(len(self.buffer), batch_size))

    def learn(self, batch_size, gamma, tau):                             # SAC.py:222-260
        total = len(self.buffer)
        batch = min(total, batch_size)
        idx = noise = None
        if host_draw(self._rng, total, batch_size):
            idx = draw_indices(total, batch_size)
        if idx is not None and self.is_continue:
            noise = np.zeros((1, 1, 2, batch, self._act_dim), np.float32)
            noise[0, 0, 0] = torch.randn(batch, self._act_dim).numpy()   # actor_target rsample (SAC.py:227)
            noise[0, 0, 1] = torch.randn(batch, self._act_dim).numpy()   # actor rsample (SAC.py:244)
        st = self._e.learn(batch, gamma=gamma, tau=tau, actor_lr=self.agent.actor_optimizer.lr,
                           critic_lr=self.agent.critic_optimizer.lr, alpha_lr=self.alphas.alpha_lr,
                           target_entropy=float(self.alphas.target_entropy), idx=idx, noise=noise,
                           want_stats=getattr(self, "track_loss", False))
        if st is not None:
            self.last_losses = tuple(float(st[0, 0, k]) for k in (N.STAT_CRITIC_LOSS, N.STAT_ACTOR_LOSS, N.STAT_ALPHA_LOSS))

    def update_target(self, tau):
        for net in (1, 0):
            q, t = self._e.get_params(net, N.PARAM_ONLINE), self._e.get_params(net, N.PARAM_TARGET)
            self._e.set_params(net, t * np.float32(1.0 - tau) + q * np.float32(tau), N.PARAM_TARGET)

    def save(self, model_dir):
        torch.save(self.agent.actor.state_dict(), os.path.join(model_dir, "SAC.pt"))

    @staticmethod
    def load(dim_info, is_continue, model_dir, trick=None):
        policy = SAC(dim_info, is_continue, 0, 0, 0, device=torch.device("cpu"), trick=trick)
        policy.agent.actor.load_state_dict(torch.load(os.path.join(model_dir, "SAC.pt")))
        return policy
