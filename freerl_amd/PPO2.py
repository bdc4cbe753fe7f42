"""GAIL's policy side with the reference's class surface (GAIL_file/PPO2.py, PPO2_utils.py), backed by the HIP engine: the PPO that
`GAIL.train` drives, and a stand-alone PPO loop of its own.

    ppo = PPO(config)                       # config['s_dim'], ['a_dim'], ['seed'], ['discrete'], ['PPO'] = {policy_mlp_dim, activation, ...}
    a = ppo.pi(s)                           # Normal(tanh(mean), exp(clamp(log_std))).sample() / Categorical(logits=).sample()
    a = ppo.pi(s, return_mean=True)         # tanh(mean) / argmax
    v = ppo.value(s)                        # [rows, 1]
    ppo.PPO_learn(batch, last_value)        # batch['states' | 'actions' | 'rewards' | 'masks_2'] as explore_env builds them
    ppo.train(gymEnvWrapper(env, config), num_episodes)
    ppo.P.state_dict() / ppo.V.state_dict() / ppo.optim.param_groups[0]['lr']

`PPO_learn` is one launch chain (kernels_gail_ppo.hip): V and the old log-prob over the horizon with the pre-update nets, the GAE scan
(`values[t + 1]` is the next row's value also across an episode end, `masks_1 == 1`; only `masks_2` cuts the recursion), the advantage
normalisation, then K_epochs x ceil(horizon / mini_batch_size) clipped-surrogate steps of both nets under the reference's one Adam with
two learning rates.  The nets and Adam's state stay on the GPU.

rng="host" (default) consumes torch's global generator exactly as the reference does: `torch.normal` / the Categorical draw per step in
`pi`, `torch.randperm` per epoch in `PPO_learn`.  rng="device" leaves both to the engine's Philox stream.

`GAE(...)` is a host-side float32 restatement for parity checks; `PPO_learn` does not call it (the scan runs in the launch chain).

Refused with ValueError, in the wording GAIL.py uses for the discriminator: an activation other than 'LeakyReLU' / 'ReLU',
`layernorm=True`, `dropout > 0`; and `discrete` with `a_dim < 2`.
"""
import copy
import json
import os
import time
from collections import namedtuple

import numpy as np
import torch
from torch.distributions import Categorical, Normal

from . import _native as N
from ._core import DeviceNet, Engine, init_layers

F32 = np.float32
_ACTIVATIONS = {"LeakyReLU": N.ACT_LEAKY_RELU, "ReLU": N.ACT_RELU}
CLIP_NORM = 0.5                 # PPO2.py:305-306: clip_grad_norm_(., 0.5) on each net


def _np(x, dtype=F32):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


class Memory:
    """PPO2_utils.Memory: a list of named tuples."""

    def __init__(self, fields=("state", "action", "next_state", "mask")):
        self.Trajectory = namedtuple("Trajectory", fields)
        self.memory = []

    def push(self, *args):
        self.memory.append(self.Trajectory(*args))

    def sample(self, batch_size=None):
        if batch_size is None:
            return self.Trajectory(*zip(*self.memory))
        import random
        return self.Trajectory(*zip(*random.sample(self.memory, batch_size)))

    def append(self, new_memory):
        self.memory += new_memory.memory

    def clear(self):
        self.memory.clear()

    def __len__(self):
        return len(self.memory)


class gymEnvWrapper:
    """PPO2_utils.gymEnvWrapper: observations scaled to [-1, 1] when the space's bounds are finite, continuous actions clipped to
    [-1, 1] and unscaled to the env's range, `done = terminate or truncation`; everything handed back as float32 tensors."""

    def __init__(self, env, config):
        self.env = env
        self.config = config
        self.reproducible = config["env_reproducible"]
        self.device = torch.device("cpu")

    @property
    def reproducible(self):
        return self._reproducible

    @reproducible.setter
    def reproducible(self, value):
        self._reproducible = value
        self.seed = self.config["seed"] if self._reproducible else None

    def _scale(self, state):
        low, high = self.env.observation_space.low, self.env.observation_space.high
        if not (np.any(np.isinf(low)) or np.any(np.isinf(high))):
            state = 2 * (state - low) / (high - low) - 1
        return state

    def reset(self):
        return torch.as_tensor(self._scale(self.env.reset(seed=self.seed)[0]), dtype=torch.float32)

    def step(self, state, action):
        if self.config.get("discrete", False):
            action_np = int(_np(action).squeeze()) if isinstance(action, torch.Tensor) else int(action)
        else:
            sp = self.env.action_space
            action_np = np.clip(_np(action), -1.0, 1.0)
            action_np = action_np * (sp.high - sp.low) / 2 + (sp.high + sp.low) / 2
        next_state, reward, terminate, truncation, info = self.env.step(action_np)
        done = terminate or truncation
        info["terminate"] = torch.as_tensor(terminate, dtype=torch.float32)
        return (torch.as_tensor(self._scale(next_state), dtype=torch.float32), torch.as_tensor(reward, dtype=torch.float32),
                torch.as_tensor(done, dtype=torch.float32), info)


class ScalarRecorder:
    """What the loop needs of SummaryWriter when torch.utils.tensorboard is not importable: add_scalar into a list (and scalars.csv)."""

    def __init__(self, log_dir=None, purge_step=None):
        self.scalars = []
        self._f = open(os.path.join(log_dir, "scalars.csv"), "a") if log_dir else None

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))
        if self._f:
            self._f.write("%s,%d,%r\n" % (tag, int(step), float(value)))
            self._f.flush()

    def close(self):
        if self._f:
            self._f.close()
            self._f = None


def _writer(log_dir, purge_step):
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(log_dir=log_dir, purge_step=purge_step)
    except Exception:
        return ScalarRecorder(log_dir, purge_step)


class _Optim:
    """`ppo.optim`: the reference's ONE Adam with two param groups (P: p_lr, V: v_lr), as far as callers touch it."""

    def __init__(self, engine, p_lr, v_lr):
        self._e = engine
        self.param_groups = [dict(lr=float(lr), betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0) for lr in (p_lr, v_lr)]

    def zero_grad(self):
        pass

    def step(self):
        raise NotImplementedError("the Adam step is fused into PPO_learn on the GPU")

    def state_dict(self):
        return dict(step=self._e.opt_step(0), param_groups=copy.deepcopy(self.param_groups),
                    exp_avg=[self._e.get_params(n, N.PARAM_ADAM_M) for n in (0, 1)], exp_avg_sq=[self._e.get_params(n, N.PARAM_ADAM_V) for n in (0, 1)])

    def load_state_dict(self, sd):
        for n in (0, 1):
            self._e.set_params(n, sd["exp_avg"][n], N.PARAM_ADAM_M)
            self._e.set_params(n, sd["exp_avg_sq"][n], N.PARAM_ADAM_V)
            self._e.set_opt_step(n, int(sd["step"]))
            self.param_groups[n].update(sd["param_groups"][n])


class PolicyModel:
    """PPO2.PolicyModel: `P` (Actor / ActorDiscrete), `V` (Critic), `pi`, `value` on the engine's nets 0 and 1."""

    def __init__(self, config, engine, layers_p, layers_v, rng):
        self.config, self._e, self._rng = config, engine, rng
        self._discrete = bool(config.get("discrete", False))
        self._a = int(config["a_dim"])
        self.P = DeviceNet(engine, 0, layers_p, extra=None if self._discrete else ("log_std", (1, self._a)))
        self.V = DeviceNet(engine, 1, layers_v)

    def _rows(self, s):
        x = _np(s)
        return (x[None], True) if x.ndim == 1 else (x, False)

    def _std(self):
        lo, hi = self._e.log_std_range()
        return np.exp(np.clip(self.P.state_dict()["log_std"].numpy().reshape(-1), lo, hi)).astype(F32)

    def pi(self, s, return_dist=False, return_mean=False):
        x, single = self._rows(s)
        n = len(x)
        if self._discrete:
            if return_mean:
                out = torch.from_numpy(self._e.act(0, N.ACT_ARGMAX, x)[0, :, 0].astype(np.int64))
                return out[0] if single else out
            if return_dist:
                logits = torch.from_numpy(self._e.act(0, N.ACT_RAW, x, out_dim=self._a)[0])
                return Categorical(logits=logits[0] if single else logits)
            # Categorical.sample(): torch.multinomial(probs, 1) = argmax(p / q), q = empty_like(probs).exponential_(1)
            q = torch.empty(n, self._a).exponential_(1).numpy() if self._rng == "host" else None
            out = torch.from_numpy(self._e.act(0, N.ACT_CAT_SAMPLE, x, eps=q)[0, :, 0].astype(np.int64))
            return out[0] if single else out
        if return_mean or return_dist:
            mean = torch.from_numpy(self._e.act(0, N.ACT_TANHHEAD, x, out_dim=self._a)[0])
            mean = mean[0] if single else mean
            if return_mean:
                return mean
            return Normal(mean, torch.from_numpy(self._std()).expand_as(mean))
        # Normal.sample() = torch.normal(mean, std): a standard-normal draw of the mean's shape, times std, plus mean
        eps = torch.normal(torch.zeros(n, self._a), torch.ones(n, self._a)).numpy() if self._rng == "host" else None
        out = torch.from_numpy(self._e.act(0, N.ACT_PPO_SAMPLE, x, eps=eps, out_dim=self._a)[0])
        return out[0] if single else out

    def value(self, s):
        x, single = self._rows(s)
        out = torch.from_numpy(self._e.act(1, N.ACT_RAW, x, out_dim=1)[0])
        return out[0] if single else out

    def to(self, *a, **k):
        return self


class PPO:
    def __init__(self, config, *, rng="host", seed=0):
        C = config["PPO"]
        if C["activation"] not in _ACTIVATIONS:
            raise ValueError("PPO.activation %r: the policy's kernels take 'LeakyReLU' or 'ReLU' (the shipped configs have no other)" % (C["activation"],))
        if C.get("layernorm", False):
            raise ValueError("PPO.layernorm=True is not supported (the shipped config has layernorm False)")
        if C.get("dropout", 0.0) > 0:
            raise ValueError("PPO.dropout > 0 is not supported (the shipped config has dropout 0)")
        if config.get("discrete", False) and int(config["a_dim"]) < 2:
            raise ValueError("discrete with a_dim %d: a Categorical policy needs at least 2 logits" % int(config["a_dim"]))
        if rng not in ("host", "device"):
            raise ValueError("rng must be 'host' or 'device', got %r" % (rng,))
        self.config = config
        self.device = torch.device("cpu")                  # where returned tensors live; the compute device is the HIP GPU
        self._rng = rng
        self._discrete = bool(config.get("discrete", False))
        s, a, H = int(config["s_dim"]), int(config["a_dim"]), int(C["policy_mlp_dim"])
        self._s, self._a = s, a
        layers_p = [("backbone.0", H, s), ("backbone.1", H, H), ("backbone.2", a, H)]
        layers_v = [("backbone.0", H, s), ("backbone.1", H, H), ("backbone.2", 1, H)]
        self._layers = (layers_p, layers_v)
        init_p, init_v = self.consume_init_draws()
        self._e = Engine(N.ALGO_GAIL_PPO, s, a, int(C["horizon"]), discrete=self._discrete, hidden=H, hidden_act=_ACTIVATIONS[C["activation"]],
                         batch_max=int(C["mini_batch_size"]), seed=seed)
        self._e.set_log_std_range(float(C["log_std_min"]), float(C["log_std_max"]))
        self._e.set_params(0, init_p if self._discrete else np.concatenate([init_p, np.zeros(a, F32)]))      # log_std = zeros(1, a_dim)
        self._e.set_params(1, init_v)
        self.P_model = PolicyModel(config, self._e, layers_p, layers_v, rng)
        self.P, self.V = self.P_model.P, self.P_model.V
        self.pi, self.value = self.P_model.pi, self.P_model.value
        self.optim = _Optim(self._e, C["p_lr"], C["v_lr"])
        self.last_learn = None                             # what the last PPO_learn returned (loss trace, raw advantages, returns)

    def global_seed(self, seed):
        torch.manual_seed(seed)
        np.random.seed(seed)

    def consume_init_draws(self):
        """global_seed(config['seed']) and the default-init draws of P, then V — the reference's construction order.  `GAIL(config, ppo=...)`
        calls it again behind the discriminator's draws, where the reference constructs its PPO, so that the generator stands where it does."""
        self.global_seed(self.config["seed"])
        return init_layers(self._layers[0]), init_layers(self._layers[1])

    # ------------------------------------------------------------------ checkpoints (the reference's keys)
    def save_model(self, path=None, iteration=0, name=""):
        name = "_%s" % name if name != "" else ""
        self.model_pth = os.path.join(self.config["log_dir"], "model%s.pth" % name)
        path = path if path is not None else self.model_pth
        ck = {"iteration": iteration, "P_state_dict": self.P.state_dict(), "V_state_dict": self.V.state_dict(),
              "optim_state_dict": self.optim.state_dict(), "cpu_rng_state": torch.get_rng_state(), "numpy_rng_state": np.random.get_state()}
        if torch.cuda.is_available():
            ck["cuda_rng_state"] = torch.cuda.get_rng_state()
        torch.save(ck, path)

    def load_model(self, path):
        ck = torch.load(path, weights_only=False)
        self.config["log_dir"] = os.path.dirname(path)
        self.P.load_state_dict(ck["P_state_dict"])
        self.V.load_state_dict(ck["V_state_dict"])
        self.optim.load_state_dict(ck["optim_state_dict"])
        torch.set_rng_state(ck["cpu_rng_state"])
        if "cuda_rng_state" in ck and torch.cuda.is_available():
            torch.cuda.set_rng_state(ck["cuda_rng_state"])
        np.random.set_state(ck["numpy_rng_state"])
        return ck.get("iteration", 0)

    # ------------------------------------------------------------------ learning
    def GAE(self, rewards, values, masks_1, masks_2, gamma, lam, last_value=None, MC=False):
        """PPO2.GAE (:186-233) restated on the host in float32 for parity checks -> (normalised advantages, returns)."""
        r, v, m1, m2 = (_np(x).reshape(-1) for x in (rewards, values, masks_1, masks_2))
        v = np.append(v, F32(0.0 if last_value is None else float(last_value)))
        g, c = F32(gamma), F32(gamma * lam)
        adv, ret, last, fut = np.zeros_like(r), np.zeros_like(r), F32(0), F32(0)
        for t in reversed(range(len(r))):
            delta = r[t] + g * v[t + 1] * m1[t] - v[t]
            adv[t] = last = delta + c * m2[t] * last
            ret[t] = fut = r[t] + g * fut * m2[t]
        if not MC:
            ret = adv + v[:-1]
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + F32(1e-8))
        return torch.from_numpy(adv.astype(F32)), torch.from_numpy(ret.astype(F32))

    def PPO_learn(self, batch, last_value=None):
        C = self.config["PPO"]
        states, actions = _np(batch["states"]), _np(batch["actions"])
        T = len(states)
        if T > self._e.capacity:
            raise ValueError("a batch of %d rows > config['PPO']['horizon'] = %d, the engine's ring" % (T, self._e.capacity))
        lay = self._e.layout
        rec = np.zeros((T, self._e.width), F32)
        rec[:, lay.obs_off[0]:lay.obs_off[0] + self._s] = states.reshape(T, self._s)
        rec[:, lay.act_off[0]:lay.act_off[0] + lay.act_dim[0]] = actions.reshape(T, lay.act_dim[0])
        rec[:, lay.done_off] = 1.0 - _np(batch["masks_2"]).reshape(T)
        self._e.set_cursor(0, 0, 0)
        self._e.add_batch(rec)
        K = int(C["K_epochs"])
        # torch.randperm once per epoch, in the reference's order (:266)
        perms = np.stack([torch.randperm(T).numpy() for _ in range(K)])[None] if self._rng == "host" else None
        self.last_learn = self._e.gail_ppo_learn(
            T, min(int(C["mini_batch_size"]), self._e.batch_max), K, gamma=C["gamma"], lam=C["lam"], clip=C["clip_epsilon"], ent_weight=C["ent_weight"],
            value_loss_coef=C["value_loss_coef"], p_lr=self.optim.param_groups[0]["lr"], v_lr=self.optim.param_groups[1]["lr"], clip_norm=CLIP_NORM,
            last_value=None if last_value is None else _np(last_value).reshape(-1)[:1], rewards=_np(batch["rewards"]).reshape(1, T), perms=perms,
            want=("adv", "returns", "trace"))

    # ------------------------------------------------------------------ the loop's pieces
    def _init_logging(self, resume=False, start_iteration=0):
        if not resume:
            base = self.config["log_dir"] if os.path.isabs(self.config["log_dir"]) else os.path.join(os.getcwd(), self.config["log_dir"])
            self.config["log_dir"] = os.path.abspath(os.path.join(base, self.config["algo"], time.strftime("%Y%m%d-%H%M%S")))
        os.makedirs(self.config["log_dir"], exist_ok=True)
        self.writer = _writer(self.config["log_dir"], start_iteration)
        print("Logging to:", self.config["log_dir"])
        self.max_reward = -float("inf")
        self.eval_history = []
        self.save_config()

    def save_config(self, path=None):
        with open(path if path is not None else os.path.join(self.config["log_dir"], "config.json"), "w") as f:
            json.dump(self.config, f, indent=4)

    def explore_env(self, env_wrapper):
        while True:
            self.step += 1
            state_tensor = torch.as_tensor(self.state, dtype=torch.float32)
            action = self.pi(state_tensor.unsqueeze(0))
            if self._discrete:
                action_to_env = int(action.item() if action.dim() == 0 else action.squeeze(0).item())
                action_save = torch.tensor([[action_to_env]], dtype=torch.long)
            else:
                action = action.squeeze(0).detach()
                action_to_env = action_save = action
            next_state, reward, done, info = env_wrapper.step(self.state, action_to_env)
            self.memory.push(state_tensor, action_save, reward, 1.0 - done)
            self.state = next_state
            self.episode_reward += reward
            if done:
                self.writer.add_scalar("Episode Reward", self.episode_reward, self.episode_num)
                self.train_return.append(self.episode_reward)
                self.episode_num += 1
                print("Episode %d/%d, Reward: %s" % (self.episode_num, self.max_episodes, float(self.episode_reward)))
                if self.episode_num >= self.max_episodes:
                    return None
                self.state = env_wrapper.reset()
                self.episode_reward = 0.0
            if self.step % self.horizon == 0:
                mem = self.memory.sample()
                return {"states": torch.stack(mem.state), "actions": torch.stack(mem.action), "rewards": torch.stack(mem.reward),
                        "masks_2": torch.stack(mem.mask)}

    def train_init(self, env_wrapper, num_episodes, model_path=None):
        resume = model_path is not None and os.path.exists(model_path)
        start_iter = self.load_model(model_path) if resume else 0
        self._init_logging(resume=resume, start_iteration=start_iter)
        self.horizon = self.config["PPO"]["horizon"]
        self.max_episodes = num_episodes
        self.episode_num = start_iter
        self.step = 0
        self.episode_reward = 0.0
        self.train_return = []
        self.state = env_wrapper.reset()
        self.memory = Memory(fields=("state", "action", "reward", "mask"))

    def eval_and_save(self, env_wrapper):
        C = self.config["PPO"]
        if self.episode_num % C["eval_interval"] == 0 and self.episode_num > 0:
            avg = self.evaluate(env_wrapper, C["eval_episodes"])
            self.writer.add_scalar("Eval/Average Return", avg, self.episode_num)
            self.eval_history.append((self.episode_num, avg))
            if avg > self.max_reward:
                self.max_reward = avg
                self.save_model(name="best", iteration=self.episode_num)
                self.writer.add_scalar("Eval/Best Return", self.max_reward, self.episode_num)
                print("New best model saved with average return: %s" % self.max_reward)

    def train_post(self, env_wrapper):
        self.save_model(name="final", iteration=self.max_episodes)
        # (the reference evaluates model_best.pth here and fails when no evaluation ever saved one; the final model stands in then)
        best = os.path.join(self.config["log_dir"], "model_best.pth")
        return self.evaluate(env_wrapper, 10, for_best_model_eval=True, best_model_path=best if os.path.exists(best) else self.model_pth,
                             for_eval_data=self.config["collect_eval_data"])

    def train(self, env_wrapper, num_episodes, model_path=None):
        self.train_env = env_wrapper
        self.eval_env = copy.deepcopy(env_wrapper)
        self.train_init(self.train_env, num_episodes, model_path)
        while self.episode_num < self.max_episodes:
            batch = self.explore_env(self.train_env)
            if batch is None:
                break
            last_value = self.value(torch.as_tensor(self.state, dtype=torch.float32).unsqueeze(0)).squeeze()
            self.PPO_learn(batch, last_value)
            self.eval_and_save(self.eval_env)
            self.memory.clear()
        return self.train_post(self.eval_env)

    def evaluate(self, env_wrapper, num_episodes, for_best_model_eval=False, best_model_path=None, for_eval_data=False):
        if for_best_model_eval:
            self.load_model(best_model_path if best_model_path is not None else os.path.join(self.config["log_dir"], "model_best.pth"))
            env_wrapper.reproducible = False
        states, actions = [], []
        if for_eval_data:
            env_wrapper.reproducible = False
        total_reward, total_step = [], []
        for _ in range(num_episodes):
            state, done, episode_reward, episode_steps = env_wrapper.reset(), False, 0.0, 0
            while not done:
                action = self.pi(torch.as_tensor(state, dtype=torch.float32).unsqueeze(0), return_mean=True).squeeze(0).detach()
                if for_eval_data:
                    states.append(_np(state))
                    actions.append(_np(action))
                state, reward, done, info = env_wrapper.step(state, action)
                episode_reward += reward
                episode_steps += 1
            total_reward.append(_np(episode_reward))
            total_step.append(episode_steps)
        if for_eval_data:
            np.savez(os.path.join(self.config["log_dir"], "eval_data.npz"), states=np.array(states), actions=np.array(actions).reshape(len(actions), -1),
                     index=np.array(total_step))
        if for_best_model_eval:
            avg = sum(total_reward) / num_episodes
            np.savez(os.path.join(self.config["log_dir"], "eval_rewards.npz"), episode_rewards=total_reward, episode_avg_rewards=avg)
            return avg, total_reward
        return np.mean([r / s for r, s in zip(total_reward, total_step)])
