"""`REINFORCE` with the reference's class surface (REINFORCE_file/REINFORCE.py:49-138), backed by the HIP engine.

    policy = REINFORCE(dim_info, is_continue, policy_net_lr, device, trick=None)
    policy.select_action(obs) / evaluate_action(obs) / add(reward, done) / all() / learn(gamma)
    policy.save(model_dir) / REINFORCE.load(dim_info, is_continue, model_dir)
    policy.agent.policy_net / .policy_net_optimizer

The reference keeps the autograd graph of every `select_action` alive until `learn()`.  Here `select_action` stages
(obs, action, log-prob) and `add(reward, done)` commits the staged step with its reward and flag to the engine's ring;
`learn(gamma)` is one launch chain over the stored rows (kernels_reinforce.hip) and empties the ring.  `max_steps` is the
ring's capacity: the most steps that can be stored between two `learn()` calls.

`n_learners > 1` runs a population: `select_action` takes [P, obs_dim] and returns [P] actions, `add` takes [P] rewards and
flags and an optional `active` mask (learners whose episode is over stop committing), `learn` takes every learner's stored
steps — they may differ, and a learner with none sits the call out.

Reference defects handled as intended: `is_continue=True` is a ValueError (the reference ignores the flag and
fails in env.step); a `select_action` / `evaluate_action` that no `add` follows is overwritten by the next one (the
reference appends a log-prob that no reward ever matches); `learn` with one stored step (NaN in the reference) or none is
a ValueError; `add` past `max_steps` is a RuntimeError.
"""
import os

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, OptimizerView, init_layers, resolve_device

HIDDEN = 128        # Policy_MLP's hard-coded width (REINFORCE.py:39)


class SoftmaxPolicy(DeviceNet):
    """`agent.policy_net` (Policy_MLP, REINFORCE.py:32-46): calling it returns the action probabilities."""

    def __call__(self, *inputs):
        return torch.softmax(super().__call__(*inputs), dim=1)


class Agent:
    """Agent (REINFORCE.py:49-60): policy_net, Adam(policy_net.parameters(), lr)."""

    def __init__(self, engine, obs_dim, action_dim, policy_net_lr):
        layers = [("l1", HIDDEN, obs_dim), ("l2", action_dim, HIDDEN)]
        for p in range(engine.P):                                       # torch RNG: l1 then l2, learner by learner
            engine.set_params(0, init_layers(layers), N.PARAM_ONLINE, learner=p)
        self.policy_net = SoftmaxPolicy(engine, 0, layers)
        self.policy_net_optimizer = OptimizerView(engine, 0, policy_net_lr)

    def update_policy(self, loss):
        raise NotImplementedError("zero_grad/backward/step are fused into REINFORCE.learn() on the GPU")


class REINFORCE:
    def __init__(self, dim_info, is_continue, policy_net_lr, device, trick=None, *, max_steps=2048, n_learners=1, seed=0):
        obs_dim, action_dim = dim_info
        if is_continue:
            raise ValueError("REINFORCE samples from a Categorical over discrete actions (REINFORCE.py:82-85); "
                             "is_continue=True has no counterpart in the reference")
        hip_id, self.device = resolve_device(device)
        self.max_steps = max(int(max_steps), 2)
        self._P = int(n_learners)
        self._e = Engine(N.ALGO_REINFORCE, obs_dim, action_dim, self.max_steps, n_learners=self._P, discrete=True,
                         hidden=HIDDEN, batch_max=self.max_steps, device_id=hip_id, seed=seed)
        self.agent = Agent(self._e, obs_dim, action_dim, policy_net_lr)
        self.is_continue = is_continue
        self._obs_dim, self._act_dim = obs_dim, action_dim
        self._staged = None                       # (obs [P, O], action [P], log-prob [P]) of the last select_action
        self._clear()
        self.track_loss = False                   # True: learn() reads the loss back into `last_loss` (it costs a device sync)
        self.last_loss = None

    def _clear(self):
        self.rewards = [[] for _ in range(self._P)]
        self.done = [[] for _ in range(self._P)]
        self.log_probs = [[] for _ in range(self._P)]

    def select_action(self, obs):
        """Categorical(probs).sample() and its log-prob (REINFORCE.py:76-88): torch draws `empty(rows, nA).exponential_(1)` and
        takes argmax(p / q), so the engine gets the same q from the same generator."""
        x = np.asarray(obs, dtype=np.float32).reshape(self._P, 1, self._obs_dim)
        q = torch.empty(self._P, self._act_dim).exponential_(1).numpy()
        a, logp = self._e.act(0, N.ACT_CAT_SAMPLE, x, eps=q.reshape(self._P, 1, -1), want_logp=True)
        self._staged = (x[:, 0].copy(), a[:, 0, 0].copy(), logp[:, 0, 0].copy())
        act = a[:, 0, 0].astype(np.int64)
        return np.int64(act[0]) if self._P == 1 else act

    def evaluate_action(self, obs):
        """The reference's evaluate_action calls select_action (REINFORCE.py:90-92): it samples too."""
        return self.select_action(obs)

    def add(self, reward, done, active=None):
        """Commit the staged step with its reward and `done` flag (REINFORCE.py:95-97)."""
        if self._staged is None:
            raise RuntimeError("add() without a select_action() before it: there is no step to commit")
        obs, act, logp = self._staged
        self._staged = None
        rew = np.broadcast_to(np.asarray(reward, dtype=np.float64).reshape(-1), (self._P,))
        dn = np.broadcast_to(np.asarray(done).reshape(-1), (self._P,))
        on = np.ones(self._P, bool) if active is None else np.asarray(active, dtype=bool).reshape(self._P)
        who = np.nonzero(on)[0]
        for p in who:
            if len(self.rewards[p]) >= self.max_steps:
                raise RuntimeError("%d steps are stored and none has been learned from: raise REINFORCE(..., max_steps=%d) "
                                   "or call learn() more often" % (self.max_steps, self.max_steps))
        lay = self._e.layout
        recs = np.zeros((who.size, self._e.width), np.float32)
        for i, p in enumerate(who):
            recs[i, lay.obs_off[0]:lay.obs_off[0] + self._obs_dim] = obs[p]
            recs[i, lay.act_off[0]] = act[p]
            recs[i, lay.rew_off] = rew[p]
            recs[i, lay.done_off] = float(bool(dn[p]))
            self.rewards[p].append(reward if self._P == 1 else float(rew[p]))
            self.done[p].append(done if self._P == 1 else bool(dn[p]))
            self.log_probs[p].append(torch.tensor([logp[p]], dtype=torch.float32))
        if who.size:
            self._e.add_batch(recs, learners=who.astype(np.int32))

    def all(self):
        """(rewards, dones, log_probs) stored since the last learn() (REINFORCE.py:99-100); lists per learner when n_learners > 1."""
        if self._P == 1:
            return self.rewards[0], self.done[0], self.log_probs[0]
        return self.rewards, self.done, self.log_probs

    def learn(self, gamma):
        """One policy-gradient step on everything stored since the last call (REINFORCE.py:104-127), then the lists are cleared."""
        n = [len(r) for r in self.rewards]
        if max(n) == 0:
            raise ValueError("learn() with no stored step (the reference raises in its backward pass)")
        if 1 in n:
            raise ValueError("learn() with exactly one stored step: the std of one return is NaN and the reference turns "
                             "every parameter into NaN")
        out = self._e.reinforce_learn(gamma=gamma, lr=self.agent.policy_net_optimizer.lr, n_steps=n,
                                      want_loss=self.track_loss)
        if "loss" in out:
            self.last_loss = float(out["loss"][0]) if self._P == 1 else out["loss"]
        self._clear()

    def save(self, model_dir):
        torch.save(self.agent.policy_net.state_dict(), os.path.join(model_dir, "REINFORCE.pt"))

    @staticmethod
    def load(dim_info, is_continue, model_dir, trick=None):
        policy = REINFORCE(dim_info, is_continue, 0, device=torch.device("cpu"), trick=trick)
        policy.agent.policy_net.load_state_dict(torch.load(os.path.join(model_dir, "REINFORCE.pt")))
        return policy
