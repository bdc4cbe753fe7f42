"""`CEM_GD3PG` (guided dual-actor DDPG with a sepCEM population: "Novel Evolutionary Deep Reinforcement Learning Algorithm:
CEM-GD3PG") with the reference's class surface (CEM_GD3PG_file/CEM_GD3PG.py:94-243), backed by the HIP engine, and `sepCEM`, the one
search class its loop uses (CEM_GD3PG_file/ES.py:438-530), on the host.

    policy = CEM_GD3PG(dim_info=[obs_dim, action_dim], is_continue, actor_lr, critic_lr, buffer_size, device)
    policy.agent.actor_1 / actor_2 / critic / *_target / actor_domain          (.get_params() / .set_params(flat) / .get_size() on actors)
    policy.buffer / policy.buffer_domain                                        (len(), .add(...), .sample(indices))
    policy.select_action(obs, actor) / evaluate_action(obs, actor) / add(buffer, obs, action, reward, next_obs, done) / sample(batch_size)
    policy.learn(batch_size, gamma, tau, is_F1_more, delta, actor_domain)
    policy.save(model_dir, actor_domain) / CEM_GD3PG.load(dim_info, model_dir)

`learn()` is one launch chain (kernels_cem_gd3pg.hip): the critic step on the minimum over both target actors, both actor steps through
the updated critic — the poorer actor with the penalty lambda delta sqrt(sum (actor(s) - actor_domain(s))^2 / B) —, the three soft
updates; both rings, the seven nets and Adam's state stay on the GPU.  `rng="host"` consumes NumPy's global stream exactly as
`sample()` does (two `np.random.choice` calls per learn, both bounded by len(buffer_domain)); `rng="device"` draws on the engine's
Philox stream; `rng="auto"` is host below _core.AUTO_DEVICE_MIN_ROWS rows.

Departures (DESIGN.md "CEM_GD3PG"): a batch in which the guided actor equals the domain actor on every row (sum c^2 == 0) takes the
penalty's gradient as 0 where torch's sqrt backward gives NaN; `is_continue=False` raises ValueError (the reference builds a
one-column action buffer that its critic cannot read); `evaluate_action` works (the reference's passes `self` twice and raises
TypeError); `learn()` takes the agent's own `actor_domain` only — the engine holds one per learner.
"""
import os

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, F32, OptimizerView, host_draw, init_layers, resolve_device
from .Buffer import Buffer

HIDDEN = 128        # Actor's / Critic's default widths (CEM_GD3PG.py:31,75)
LAMBDA = 10.0       # Actor.lambda_ (:42)
NET_ACTOR_1, NET_ACTOR_2, NET_CRITIC, NET_DOMAIN = 0, 1, 2, 3


class _Actor(DeviceNet):
    """Actor (CEM_GD3PG.py:30-72): the flat parameter vector in torch's parameters() order, which is the engine's host order."""

    def get_params(self):
        return np.array(self._e.get_params(self._net, self._kind, self._learner), dtype=F32, copy=True)

    def set_params(self, params):
        self._e.set_params(self._net, np.asarray(params, dtype=F32).reshape(-1), self._kind, self._learner)

    def get_size(self):
        return self._e.num_params(self._net)


class Agent:
    """Agent (CEM_GD3PG.py:94-127): actor_1, actor_2, critic, their Adam optimizers, deep copies as targets and `actor_domain`, a
    deep copy of actor_2."""

    def __init__(self, engine, obs_dim, action_dim, actor_lr, critic_lr, hidden):
        la = [("l1", hidden, obs_dim), ("l2", hidden, hidden), ("l3", action_dim, hidden)]
        lc = [("l1", hidden, obs_dim + action_dim), ("l2", hidden, hidden), ("l3", 1, hidden)]
        flats = {}
        for net, layers in ((NET_ACTOR_1, la), (NET_ACTOR_2, la), (NET_CRITIC, lc)):      # torch RNG: actor_1, actor_2, critic
            flats[net] = init_layers(layers)
            engine.set_params(net, flats[net], N.PARAM_ONLINE)
            engine.set_params(net, flats[net], N.PARAM_TARGET)
        engine.set_params(NET_DOMAIN, flats[NET_ACTOR_2], N.PARAM_ONLINE)
        self.actor_1 = _Actor(engine, NET_ACTOR_1, la, act_mode=N.ACT_TANHHEAD)
        self.actor_2 = _Actor(engine, NET_ACTOR_2, la, act_mode=N.ACT_TANHHEAD)
        self.critic = DeviceNet(engine, NET_CRITIC, lc)
        self.actor_1_optimizer = OptimizerView(engine, NET_ACTOR_1, actor_lr)
        self.actor_2_optimizer = OptimizerView(engine, NET_ACTOR_2, actor_lr)
        self.critic_optimizer = OptimizerView(engine, NET_CRITIC, critic_lr)
        self.actor_1_target = _Actor(engine, NET_ACTOR_1, la, kind=N.PARAM_TARGET, act_mode=N.ACT_TANHHEAD)
        self.actor_2_target = _Actor(engine, NET_ACTOR_2, la, kind=N.PARAM_TARGET, act_mode=N.ACT_TANHHEAD)
        self.critic_target = DeviceNet(engine, NET_CRITIC, lc, kind=N.PARAM_TARGET)
        self.actor_domain = _Actor(engine, NET_DOMAIN, la, act_mode=N.ACT_TANHHEAD)

    def update_actor_1(self, loss):
        raise NotImplementedError("zero_grad/backward/clip/step are fused into CEM_GD3PG.learn() on the GPU")

    update_actor_2 = update_critic = update_actor_1


class _Ring(Buffer):
    """One of the learner's two rings (ring 0 `buffer`, ring 1 `buffer_domain`) with Buffer's surface."""

    def __init__(self, engine, ring, capacity, device):
        self._ring = int(ring)
        self.capacity = int(capacity)
        self._attach(engine, 0, 0, device)
        self._rec = np.zeros(engine.width, dtype=F32)

    @property
    def _index(self):
        return self._e.ring_cursor(self._ring)[0]

    @_index.setter
    def _index(self, v):
        self._e.set_ring_cursor(self._ring, int(v), self._e.ring_cursor(self._ring)[1])

    @property
    def _size(self):
        return self._e.ring_cursor(self._ring)[1]

    @_size.setter
    def _size(self, v):
        self._e.set_ring_cursor(self._ring, self._e.ring_cursor(self._ring)[0], int(v))

    def add(self, obs, action, reward, next_obs, done):
        r = self._rec
        r[self._obs[0]:self._obs[0] + self._obs[1]] = np.asarray(obs, dtype=F32).reshape(-1)
        r[self._act[0]:self._act[0] + self._act[1]] = np.asarray(action, dtype=F32).reshape(-1)
        r[self._rew[0]] = reward
        r[self._nobs[0]:self._nobs[0] + self._nobs[1]] = np.asarray(next_obs, dtype=F32).reshape(-1)
        r[self._done[0]] = float(done)
        self._e.ring_add(self._ring, r)

    def _gather(self, indices, fields):
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < -self.capacity or idx.max() >= self.capacity):
            raise IndexError("index out of range for a ring of %d rows" % self.capacity)
        return super()._gather(np.where(idx < 0, idx + self.capacity, idx) + self._ring * self.capacity, fields)

    def _column(self, field, squeeze=False, dtype=None):
        a = self._e.ring_rows(self._ring, 0, self.capacity)[:, field[0]:field[0] + field[1]]
        a = a[:, 0] if squeeze else a
        return a.astype(dtype) if dtype is not None else a


class CEM_GD3PG:
    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick=None, *, hidden=HIDDEN, batch_max=256,
                 seed=0, rng="auto"):
        obs_dim, action_dim = dim_info
        if not is_continue:
            raise ValueError("CEM_GD3PG's actors output continuous actions; with is_continue=False the reference builds a one-column "
                             "action buffer that its critic cannot read (CEM_GD3PG.py:134)")
        if rng not in ("auto", "host", "device"):
            raise ValueError("rng must be 'auto', 'host' or 'device', got %r" % (rng,))
        hip_id, self.device = resolve_device(device)
        cap = max(int(buffer_size), 1)
        self._e = Engine(N.ALGO_CEM_GD3PG, obs_dim, action_dim, cap, hidden=hidden, hidden_act=N.ACT_TANH, batch_max=int(batch_max),
                         device_id=hip_id, seed=seed)
        self.agent = Agent(self._e, obs_dim, action_dim, actor_lr, critic_lr, hidden)
        self.buffer = _Ring(self._e, 0, cap, self.device)
        self.buffer_domain = _Ring(self._e, 1, cap, self.device)
        self.is_continue = is_continue
        self.rng = rng
        self.last_out = None          # learn()'s statistics, in the order of _native.CEM_OUT
        self.last_indices = None      # the rows of the last host-drawn batch: (ring 0's, ring 1's)

    # ------------------------------------------------------------------ acting
    def select_action(self, obs, actor):
        obs = torch.as_tensor(obs, dtype=torch.float32).reshape(1, -1)
        return actor(obs).numpy().squeeze(0)

    def evaluate_action(self, obs, actor):
        """The deterministic policy: select_action (the reference's own passes `self` twice and raises TypeError, :152-154)."""
        return self.select_action(obs, actor)

    # ------------------------------------------------------------------ buffers
    def add(self, buffer, obs, action, reward, next_obs, done):
        buffer.add(obs, action, reward, next_obs, done)

    def _draw(self, batch_size):
        """sample()'s two draws (:161-166): both below len(buffer_domain)."""
        total = len(self.buffer_domain)
        half = min(total, batch_size) // 2
        return np.random.choice(total, half, replace=False), np.random.choice(total, half, replace=False)

    def sample(self, batch_size):
        """(obs, actions, rewards, next_obs, dones) of half a batch from `buffer`, then half from `buffer_domain` (:160-176)."""
        i0, i1 = self._draw(batch_size)
        return tuple(torch.cat([a, b], dim=0) for a, b in zip(self.buffer.sample(i0), self.buffer_domain.sample(i1)))

    # ------------------------------------------------------------------ learn
    def learn(self, batch_size, gamma, tau, is_F1_more, delta, actor_domain):
        if actor_domain is not self.agent.actor_domain:
            raise ValueError("learn() takes the agent's own actor_domain: the engine keeps one domain actor per learner "
                             "(overwrite it with actor_domain.set_params)")
        total = len(self.buffer_domain)
        idx = None
        if host_draw(self.rng, total, min(total, batch_size) // 2):
            self.last_indices = self._draw(batch_size)
            idx = np.stack(self.last_indices)[None]
        self.last_out = self._e.cem_gd3pg_learn(batch_size, gamma=gamma, tau=tau, actor_lr=self.agent.actor_1_optimizer.lr,
                                                critic_lr=self.agent.critic_optimizer.lr, f1_more=bool(is_F1_more), delta=float(delta),
                                                lam=LAMBDA, idx=idx)[0]

    def update_target(self, tau):
        """theta_target = tau * theta + (1 - tau) * theta_target for the critic and both actors (:221-231); learn() already does this on
        the device."""
        for net in (NET_CRITIC, NET_ACTOR_1, NET_ACTOR_2):
            th = self._e.get_params(net, N.PARAM_ONLINE)
            tg = self._e.get_params(net, N.PARAM_TARGET)
            self._e.set_params(net, tg * np.float32(1.0 - tau) + th * np.float32(tau), N.PARAM_TARGET)

    # ------------------------------------------------------------------ checkpoints
    def save(self, model_dir, actor_domain):
        torch.save(actor_domain.state_dict(), os.path.join(model_dir, "CEM_GD3PG.pt"))

    @staticmethod
    def load(dim_info, model_dir, **kw):
        policy = CEM_GD3PG(dim_info, True, 0, 0, 0, device=torch.device("cpu"), **kw)
        policy.agent.actor_domain.load_state_dict(torch.load(os.path.join(model_dir, "CEM_GD3PG.pt")))
        return policy


class sepCEM:
    """The cross-entropy method with a diagonal covariance, as the loop uses it (CEM_GD3PG_file/ES.py:438-530), in NumPy float64 on the
    host and on NumPy's global stream: ~20 k parameters by 10 to 20 candidates per generation.

    ask(n): mu + eps sqrt(cov), eps ~ N(0, 1) [n, num_params]; antithetic and n even: the second half of eps is minus the first; with
    elitism the last candidate is the elite.
    tell(solutions, scores): the `parents` best by score (higher is better), weights w_i ~ log((parents + 1) / i) normalised;
    damp <- 0.95 damp + 0.05 damp_limit; mu <- w . best; cov <- (1 / parents) w . (best - old mu)^2 + damp (the factor 1 / parents on top
    of normalised weights is the reference's); elite <- the best, elite_score <- minus its score."""

    def __init__(self, num_params, mu_init=None, sigma_init=1e-3, pop_size=256, damp=1e-3, damp_limit=1e-5, parents=None, elitism=False,
                 antithetic=False):
        self.num_params = num_params
        self.mu = np.zeros(num_params) if mu_init is None else np.array(mu_init)
        self.sigma = sigma_init
        self.damp = damp
        self.damp_limit = damp_limit
        self.tau = 0.95
        self.cov = self.sigma * np.ones(num_params)
        self.elitism = elitism
        self.elite = np.sqrt(self.sigma) * np.random.rand(num_params)
        self.elite_score = None
        self.pop_size = pop_size
        self.antithetic = antithetic
        if antithetic and pop_size % 2:
            raise AssertionError("Population size must be even")
        self.parents = pop_size // 2 if parents is None or parents <= 0 else parents
        ranks = np.arange(1, self.parents + 1)
        self.weights = np.log((self.parents + 1) / ranks)
        self.weights /= self.weights.sum()

    def ask(self, pop_size):
        if self.antithetic and pop_size % 2 == 0:
            half = np.random.randn(pop_size // 2, self.num_params)
            eps = np.concatenate([half, -half])
        else:
            eps = np.random.randn(pop_size, self.num_params)
        inds = self.mu + eps * np.sqrt(self.cov)
        if self.elitism:
            inds[-1] = self.elite
        return inds

    def tell(self, solutions, scores):
        cost = -np.array(scores)
        order = np.argsort(cost)
        best = np.asarray(solutions)[order[:self.parents]]
        old_mu = self.mu
        self.damp = self.damp * self.tau + (1 - self.tau) * self.damp_limit
        self.mu = self.weights @ best
        z = best - old_mu
        self.cov = 1 / self.parents * self.weights @ (z * z) + self.damp * np.ones(self.num_params)
        self.elite = np.asarray(solutions)[order[0]]
        self.elite_score = cost[order[0]]

    def get_distrib_params(self):
        return np.copy(self.mu), np.copy(self.cov)
