"""Training loops: the counterpart of the `__main__` blocks of the reference scripts
(`DQN_file/DQN.py:227-349`, `DDPG_file/DDPG_simple.py:238-362`, `TD3_file/TD3.py:315-456`,
`SAC_file/SAC.py:429-586`, `SAC_file/SAC_add_discrete.py:461-580`, `PPO_file/PPO_with_tricks.py:435-584`,
`REINFORCE_file/REINFORCE.py:227-329`, `DDPG_file/DDPG_simple_try_HER.py:295-458`,
`MADDPG_file/MADDPG_simple.py:268-395`), driving freerl_amd's GPU-backed policies.

    python -m freerl_amd.train td3 --env_name Pendulum-v1 --seed 0 --max_episodes 500

Same flags and defaults as the reference script of each algorithm, same results layout
(`results/<env>/<policy>_<n>/{<ALGO>.pt, <policy>_seed_<s>.npy}`), and the same per-step order of
operations — action rule, legacy-NumPy / torch RNG draws, add before learn, learn trigger
`step > start_steps`, per-episode noise schedules, `env.reset(seed=args.seed)` at every episode —
so a seeded run follows the reference's trajectory (tests/test_gpu_loops.py replays golden runs of
the reference's own loops).  One generic loop with per-algorithm hooks replaces the six copies.
"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

from . import envs as _envs
from . import normalization as _norm

# --------------------------------------------------------------------------------- flag tables
_COMMON = [("seed", int, 0), ("max_episodes", int, 500), ("save_freq", int, 500 // 4), ("start_steps", int, 500),
           ("random_steps", int, 0), ("learn_steps_interval", int, 1), ("gamma", float, 0.99), ("tau", float, 0.01)]
_AC = [("actor_lr", float, 1e-3), ("critic_lr", float, 1e-3)]
_REPLAY = [("buffer_size", int, int(1e6)), ("batch_size", int, 256)]
_GAUSS = [("gauss_sigma", float, 0.1), ("gauss_scale", float, 1), ("gauss_init_scale", float, None),
          ("gauss_final_scale", float, 0.0)]

_MAPPO = [("N", int, None), ("horizon", int, 256), ("clip_param", float, 0.2), ("K_epochs", int, 15), ("entropy_coefficient", float, 0.01),
          ("minibatch_size", int, 256), ("lmbda", float, 0.95), ("huber_delta", float, 10.0)]
_MAPPO_TRICK = {"adv_norm": False, "ObsNorm": False, "reward_norm": False, "reward_scaling": False, "orthogonal_init": False,
                "adam_eps": False, "lr_decay": False, "ValueClip": False, "huber_loss": False, "LayerNorm": False, "feature_norm": False}

_MA_PPO = ("mappo", "ippo", "happo")      # the multi-agent PPO scripts: one loop (_run_mappo)
_MADDPG = ("maddpg", "maddpg_att")        # MADDPG_simple.py and MADDPG_simple_with_tricks.py: one loop (_run_maddpg)
_MA_REPLAY = _MADDPG + ("masac",)         # ... and MAAC_file/MASAC.py (_run_masac): continuous parallel envs, dict in / dict out

# what GAIL_file/config.py's two dicts share (their 'PPO' sections but the activation, the learning rates and eval_interval)
_GAIL_PPO = [("seed", int, 42), ("env_reproducible", bool, True), ("discrete", bool, False), ("policy_mlp_dim", int, 128),
             ("log_std_min", float, -10), ("log_std_max", float, 2), ("horizon", int, 2048), ("gamma", float, 0.99), ("lam", float, 0.95),
             ("clip_epsilon", float, 0.2), ("K_epochs", int, 10), ("value_loss_coef", float, 1), ("ent_weight", float, 0.01),
             ("mini_batch_size", int, 64), ("eval_episodes", int, 1)]
FLAGS = {
    "dqn": dict(env_name="BipedalWalker-v3", policy_name="DQN", device="cuda", is_dis_to_con=True,
                flags=_COMMON + _REPLAY + [("Qnet_lr", float, 1e-3), ("epsilon", float, 0.1)],
                trick={"Double": False, "Dueling": False, "PER": False, "Noisy": False, "N_Step": False, "Categorical": False}),
    "ddpg": dict(env_name="Pendulum-v1", policy_name="DDPG_simple", device="cuda", is_dis_to_con=False,
                 flags=_COMMON + _AC + _REPLAY + _GAUSS, trick=None),
    # DDPG_simple_try_HER.py:298-326: DDPG_simple's flags, tau 0.01, both lrs 1e-3, start_steps 500, device cpu
    "her": dict(env_name="Pendulum-v1", policy_name="DDPG_simple_HER", device="cpu", is_dis_to_con=False,
                flags=_COMMON + _AC + _REPLAY + _GAUSS, trick=None),
    "td3": dict(env_name="MountainCarContinuous-v0", policy_name="TD3", device="cpu", is_dis_to_con=False,
                flags=_COMMON + _AC + _REPLAY + _GAUSS + [("policy_noise", float, 0.1), ("noise_clip", float, 0.5),
                                                           ("policy_freq", int, 2), ("policy_noise_scale", float, 1),
                                                           ("policy_noise_init_scale", float, None)],
                overrides=dict(seed=100, batch_size=64, gauss_sigma=1, gauss_init_scale=1), trick=None),
    "sac": dict(env_name="MountainCarContinuous-v0", policy_name="SAC", device="cpu", is_dis_to_con=False,
                flags=_COMMON + _AC + _REPLAY + _GAUSS + [("ou_sigma", float, 1), ("ou_dt", float, 1),
                                                           ("init_scale", float, 1), ("final_scale", float, 0.0)],
                overrides=dict(random_steps=500, batch_size=64, gauss_sigma=1, gauss_init_scale=1),
                trick={"ObsNorm": False, "Batch_ObsNorm": False, "OUNoise": True, "GaussNoise": False}),
    # SAC_add_discrete.py:461-486: CartPole, 500 random steps, batch 256, Batch_ObsNorm
    "sac_discrete": dict(env_name="CartPole-v1", policy_name="SAC_add_discrete", device="cpu", is_dis_to_con=False,
                         flags=_COMMON + _AC + _REPLAY, overrides=dict(random_steps=500),
                         trick={"Batch_ObsNorm": True}),
    # REINFORCE.py:228-248: CartPole, seed 100, one learn() per learn_episodes_interval finished episodes (no tau, no buffer)
    "reinforce": dict(env_name="CartPole-v1", policy_name="REINFORCE", device="cuda", is_dis_to_con=False,
                      flags=[("seed", int, 100), ("max_episodes", int, 1000), ("save_freq", int, 500 // 4), ("start_steps", int, 500),
                             ("random_steps", int, 0), ("learn_steps_interval", int, 1), ("learn_episodes_interval", int, 1),
                             ("gamma", float, 0.99), ("policy_net_lr", float, 1e-3)], trick=None),
    # GAIL_file/config.py: PPO_COBFIG (PPO2.py's __main__: 500 episodes) and GAIL_COBFIG (GAIL.py's __main__: 2000 episodes), restated
    "gail_ppo": dict(env_name="Pendulum-v1", policy_name="PPO2", device="cuda", is_dis_to_con=False,
                     flags=_GAIL_PPO + [("max_episodes", int, 500), ("activation", str, "ReLU"), ("p_lr", float, 1e-3), ("v_lr", float, 1e-3),
                                        ("eval_interval", int, 2), ("collect_eval_data", bool, True)], trick=None),
    "gail": dict(env_name="Pendulum-v1", policy_name="GAIL", device="cuda", is_dis_to_con=False,
                 flags=_GAIL_PPO + [("max_episodes", int, 2000), ("activation", str, "LeakyReLU"), ("p_lr", float, 1e-4), ("v_lr", float, 3e-4),
                                    ("eval_interval", int, 10), ("collect_eval_data", bool, False), ("expert", str, None),
                                    ("d_mlp_dim", int, 128), ("d_activation", str, "LeakyReLU"), ("d_lr", float, 4e-4), ("gp_coef", float, 10.0)],
                 trick=None),
    "ppo": dict(env_name="CartPole-v1", policy_name="PPO", device="cpu", is_dis_to_con=False,
                flags=_COMMON + _AC + [("horizon", int, 2048), ("clip_param", float, 0.2), ("K_epochs", int, 10),
                                       ("entropy_coefficient", float, 0.01), ("minibatch_size", int, 64),
                                       ("lmbda", float, 0.95)],
                overrides=dict(start_steps=0, learn_steps_interval=0),
                trick={"adv_norm": False, "ObsNorm": False, "Batch_ObsNorm": False, "reward_norm": False,
                       "reward_scaling": False, "lr_decay": False, "orthogonal_init": False, "adam_eps": False,
                       "tanh": False}),
    "maddpg": dict(env_name="simple_spread_v3", policy_name="MADDPG_simple", device="cpu", is_dis_to_con=False,
                   flags=_COMMON + _AC + _REPLAY + _GAUSS + [("N", int, 5)],
                   overrides=dict(seed=100, max_episodes=600, save_freq=600 // 4, gamma=0.95, gauss_sigma=1,
                                  gauss_init_scale=1), trick=None),
    # MADDPG_simple_with_tricks.py:283-311: the attention critic of ATT-MADDPG by default; no --save_freq (the loop saves once, at the end)
    "maddpg_att": dict(env_name="simple_spread_v3", policy_name="MADDPG_simple", device="cpu", is_dis_to_con=False,
                       flags=[f for f in _COMMON if f[0] != "save_freq"] + _AC + _REPLAY + _GAUSS + [("N", int, 5)],
                       overrides=dict(seed=0, max_episodes=600, gamma=0.95, gauss_sigma=1, gauss_init_scale=1), trick={"ATT": True}),
    # MAAC_file/MASAC.py:360-387: the script's own defaults (N = None: the env's own agent count)
    "masac": dict(env_name="simple_spread_v3", policy_name="MASAC", device="cpu", is_dis_to_con=False,
                  flags=_COMMON + _AC + _REPLAY + [("N", int, None)],
                  overrides=dict(seed=100, max_episodes=40000, save_freq=600 // 4, start_steps=500, gamma=0.95, tau=0.01, actor_lr=1e-4, critic_lr=1e-4),
                  trick=None),
    # MAPPO_file/MAPPO.py:533-571 and IPPO.py:409-449: the two scripts' own defaults
    "mappo": dict(env_name="simple_spread_v3", policy_name="MAPPO", device="cuda", is_dis_to_con=False,
                  flags=_COMMON + _AC + _MAPPO, overrides=dict(seed=100, max_episodes=200, save_freq=5000 // 4, start_steps=0,
                                                               learn_steps_interval=0, gamma=0.95), trick=dict(_MAPPO_TRICK)),
    "ippo": dict(env_name="simple_adversary_v3", policy_name="IPPO", device="cuda", is_dis_to_con=False,
                 flags=_COMMON + _AC + _MAPPO, overrides=dict(seed=100, max_episodes=5000, save_freq=5000 // 4, start_steps=0,
                                                              learn_steps_interval=0), trick=dict(_MAPPO_TRICK)),
    # MAPPO_file/HAPPO.py:547-583
    "happo": dict(env_name="simple_spread_v3", policy_name="HAPPO", device="cuda", is_dis_to_con=False,
                  flags=_COMMON + _AC + _MAPPO, overrides=dict(seed=100, max_episodes=120000, save_freq=5000 // 4, start_steps=0,
                                                               learn_steps_interval=0, gamma=0.95, actor_lr=1e-4, critic_lr=1e-4),
                  trick=dict(_MAPPO_TRICK)),
    # CEM_GD3PG_file/CEM_GD3PG.py:300-337: the script's own defaults (no --save_freq: the loop saves once, at the end; --elitism and --mult_noise
    # are its store_true flags, --n_grad is parsed and unused there too)
    "cem_gd3pg": dict(env_name="BipedalWalker-v3", policy_name="CEM_GD3PG", device="cpu", is_dis_to_con=False,
                      flags=[f for f in _COMMON if f[0] != "save_freq"] + _AC + _REPLAY + [("gauss_sigma", float, 0.1), ("max_action", float, None),
                             ("pop_size", int, 10), ("n_grad", int, 5), ("sigma_init", float, 1e-3), ("damp", float, 1e-3), ("damp_limit", float, 1e-5)],
                      overrides=dict(start_steps=1000),
                      trick={"Double": False, "Dueling": False, "PER": False, "HER": False, "Noisy": False, "n_step": False}),
}


def build_parser(algo):
    spec = FLAGS[algo]
    p = argparse.ArgumentParser(prog="freerl_amd.train " + algo)
    p.add_argument("--env_name", type=str, default=spec["env_name"])
    over = spec.get("overrides", {})
    for name, typ, default in spec["flags"]:
        p.add_argument("--" + name, type=typ, default=over.get(name, default))
    p.add_argument("--is_dis_to_con", type=bool, default=spec["is_dis_to_con"])
    p.add_argument("--policy_name", type=str, default=spec["policy_name"])
    p.add_argument("--trick", type=dict, default=spec["trick"])
    if algo == "td3":
        p.add_argument("--realize", type=dict, default={"clip_double": True, "policy_noise": True, "twin_delay": True})
    if algo == "ppo":
        p.add_argument("--beta", type=bool, default=False)
    if algo == "cem_gd3pg":
        p.add_argument("--elitism", dest="elitism", action="store_true")
        p.add_argument("--mult_noise", dest="mult_noise", action="store_true")
    if algo in _MA_PPO:                    # (type=bool as in the scripts: any non-empty string is True)
        p.add_argument("--continuous_actions", type=bool, default=(algo == "mappo"))
    p.add_argument("--device", type=str, default=spec["device"])
    # additions of this build (not in the reference)
    p.add_argument("--results_root", type=str, default=os.path.join(os.getcwd(), "results"))
    p.add_argument("--rng", type=str, default="auto", choices=["auto", "host", "device"])
    return p


# -------------------------------------------------------------------------------- bookkeeping
def make_dir(results_root, env_name, policy_name="DQN", trick=None):
    """results/<env>/<prefix><n+1>: prefix = policy name + the names of the enabled tricks
    (DQN.py:173-192)."""
    env_dir = os.path.join(results_root, env_name)
    os.makedirs(env_dir, exist_ok=True)
    prefix = policy_name + "_" + "".join(k + "_" for k, v in (trick or {}).items() if v)
    taken = [int(d.split("_")[-1]) for d in os.listdir(env_dir)
             if re.match("^" + re.escape(prefix) + r"\d+", d) and d.split("_")[-1].isdigit()]
    model_dir = os.path.join(env_dir, prefix + str(max(taken, default=0) + 1))
    os.makedirs(model_dir)
    return model_dir


class ScalarWriter:
    """`SummaryWriter(model_dir).add_scalar(tag, value, step)` (DQN.py:276,330): TensorBoard when the
    package exists, else a CSV with the same three columns."""

    def __init__(self, model_dir):
        self._tb = None
        try:
            from torch.utils.tensorboard import SummaryWriter
            self._tb = SummaryWriter(model_dir)
        except Exception:
            self._f = open(os.path.join(model_dir, "scalars.csv"), "w")
            self._f.write("tag,step,value\n")

    def add_scalar(self, tag, value, step):
        if self._tb is not None:
            self._tb.add_scalar(tag, value, step)
        else:
            self._f.write("%s,%d,%r\n" % (tag, step, float(value)))

    def close(self):
        if self._tb is not None:
            self._tb.close()
        else:
            self._f.close()


class ActionDiscretizer:
    """`dis_to_con` (DQN.py:195-217): 1-D Box -> `n` evenly spaced torques; A-D Box -> n = per^A grid
    points enumerated little-endian in base `per`."""

    def __init__(self, space, n):
        self.low, self.high, self.n = np.asarray(space.low, dtype=np.float64), np.asarray(space.high, dtype=np.float64), n
        self.dims = space.shape[0]
        self.per = n if self.dims == 1 else int(n ** (1 / self.dims))

    def __call__(self, k):
        if self.dims == 1:
            return np.array([self.low[0] + (k / (self.n - 1)) * (self.high[0] - self.low[0])])
        digits = [(k // self.per ** i) % self.per for i in range(self.dims)]
        return np.array([self.low[i] + digits[i] / (self.per - 1) * (self.high[i] - self.low[i]) for i in range(self.dims)])


class OUNoise:
    """Ornstein-Uhlenbeck exploration noise (SAC.py:334-356), NumPy legacy stream."""

    def __init__(self, action_dim, mu=0, theta=0.15, sigma=0.1, dt=1e-2, scale=None):
        self.action_dim, self.mu, self.theta, self.sigma, self.dt, self.scale = action_dim, mu, theta, sigma, dt, scale
        self.reset()

    def reset(self):
        self.state = np.ones(self.action_dim) * self.mu

    def noise(self):
        self.state = self.state + self.theta * (self.mu - self.state) + np.sqrt(self.dt) * self.sigma * np.random.randn(self.action_dim)
        return self.state if self.scale is None else self.state * self.scale


def get_env(env_name, is_dis_to_con=False):
    """(env, dim_info, max_action, is_continue) like the reference's get_env (DQN.py:142-170)."""
    env = _envs.make(env_name)
    obs_space, act_space = env.observation_space, env.action_space
    obs_dim = obs_space.shape[0] if hasattr(obs_space, "low") else 1
    if hasattr(act_space, "low"):
        action_dim = act_space.shape[0]
        dim_info, max_action, is_continue = [obs_dim, action_dim], act_space.high[0], True
        if is_dis_to_con:
            dim_info, is_continue = [obs_dim, 16 if action_dim == 1 else 2 ** action_dim], False
    else:
        dim_info, max_action, is_continue = [obs_dim, act_space.n], None, False
    return env, dim_info, max_action, is_continue


def _remaining(args, episode_num):
    return max(0, args.max_episodes - (episode_num + 1)) / args.max_episodes


# ------------------------------------------------------------------------- per-algorithm hooks
class _Hooks:
    """What differs between the reference loops; the loop itself is `_run_loop`."""

    def __init__(self, args, env, policy, dim_info, max_action):
        self.args, self.env, self.policy, self.dim_info, self.max_action = args, env, policy, dim_info, max_action
        self.action_dim = dim_info[1]

    def begin(self, obs):
        return obs

    def act(self, step, obs):           # -> (stored action, env action, extra stored fields)
        raise NotImplementedError

    def observe(self, next_obs, reward):  # -> (next_obs to store/use, reward to store)
        return next_obs, reward

    def store(self, obs, action, reward, next_obs, terminated, done, extra):
        self.policy.add(obs, action, reward, next_obs, terminated)

    def episode_end(self, episode_num):
        pass

    def after_reset(self, obs):
        return obs

    def learn_due(self, step):
        a = self.args
        return step > a.start_steps and step % a.learn_steps_interval == 0

    def learn(self, episode_num):
        raise NotImplementedError

    def finish(self, model_dir):
        pass


class _DQNHooks(_Hooks):
    def begin(self, obs):
        box = hasattr(self.env.action_space, "low")
        self.disc = ActionDiscretizer(self.env.action_space, self.action_dim) if (self.args.is_dis_to_con and box) else None
        return obs

    def act(self, step, obs):
        a = self.args
        if step < a.random_steps:                                   # DQN.py:297-306
            action = self.env.action_space.sample()
            if self.max_action is not None:
                action = action / self.max_action
                action = np.clip(np.digitize(action[0], np.linspace(-1, 1, self.action_dim + 1)) - 1, 0, self.action_dim - 1)
        elif np.random.rand() < a.epsilon:                          # DQN.py:307-310
            action = np.random.randint(self.action_dim)
        else:
            action = self.policy.select_action(obs)
        return action, (self.disc(action) if self.disc is not None else action), None

    def learn(self, episode_num):
        self.policy.learn(self.args.batch_size, self.args.gamma, self.args.tau)


class _GaussHooks(_Hooks):
    """DDPG_simple / TD3: Gaussian action noise with optional per-episode linear decay."""

    def begin(self, obs):
        a = self.args
        if a.gauss_init_scale is not None:
            a.gauss_scale = a.gauss_init_scale
        if getattr(a, "policy_noise_init_scale", None) is not None:
            a.policy_noise_scale = a.policy_noise_init_scale
        return obs

    def act(self, step, obs):
        a, m = self.args, self.max_action
        if step < a.random_steps:
            env_action = self.env.action_space.sample()
            return env_action / m, env_action, None
        action = self.policy.select_action(obs)
        noise = a.gauss_scale * np.random.normal(scale=a.gauss_sigma * m, size=self.action_dim)
        return action, np.clip(action * m + noise, -m, m), None

    def episode_end(self, episode_num):
        a = self.args
        if a.gauss_init_scale is not None:
            a.gauss_scale = a.gauss_final_scale + (a.gauss_init_scale - a.gauss_final_scale) * _remaining(a, episode_num)
        if getattr(a, "policy_noise_scale", None) is not None and hasattr(a, "policy_freq"):
            a.policy_noise_scale = a.policy_noise_scale * _remaining(a, episode_num)      # TD3.py:428-430

    def learn(self, episode_num):
        a = self.args
        if hasattr(a, "policy_freq"):
            self.policy.learn(a.batch_size, a.gamma, a.tau, a.policy_noise, a.noise_clip, self.max_action, a.policy_freq,
                              a.policy_noise_scale)
        else:
            self.policy.learn(a.batch_size, a.gamma, a.tau)


class _HERHooks(_GaussHooks):
    """DDPG_simple_try_HER.py:357-442: observations are [state | goal]; the stored reward is calcu_reward(goal, obs) of the observation
    before the step; at an episode's end the hindsight rows are written inside the ring (HindsightReplay.end_episode) before the reset,
    and the next goal is drawn after it.  The env action reaches `store` as act()'s extra field."""

    def begin(self, obs):
        from .DDPG_simple_try_HER import HindsightReplay
        a = self.args
        self.state_dim = self.dim_info[0] // 2
        self.her = HindsightReplay(self.policy, self.state_dim, self.state_dim, sample_num=4, sample_range=200, mode="her",
                                   rng="device" if a.rng == "device" else "host")
        self.goal = np.array([1, 0, 0], dtype=np.float32)            # :377
        return np.concatenate((super().begin(obs), self.goal))

    def act(self, step, obs):
        action, env_action, _ = super().act(step, obs)
        return action, env_action, env_action

    def observe(self, next_obs, reward):
        return np.concatenate((next_obs, self.goal)), reward        # :396

    def store(self, obs, action, reward, next_obs, terminated, done, env_action):
        from .DDPG_simple_try_HER import calcu_reward
        self.policy.add(obs, action, calcu_reward(self.goal, obs, env_action), next_obs, terminated)      # :397,402
        self.her.step(obs, env_action, next_obs)                    # :398

    def episode_end(self, episode_num):
        super().episode_end(episode_num)
        self.her.end_episode()                                      # :421-428

    def after_reset(self, obs):
        # the next goal: a point on the unit circle's first quadrant and a spin in [0, 2), two NumPy draws taken after env.reset
        # and in this order (:435-439)
        u, v = np.random.rand(), np.random.rand()
        self.goal = np.array([u, np.sqrt(1 - u ** 2), 2 * v])
        return np.concatenate((obs, self.goal))


class _SACHooks(_Hooks):
    def begin(self, obs):
        a = self.args
        self.obs_norm = _norm.Normalization(shape=self.dim_info[0]) if a.trick["ObsNorm"] else None
        if self.obs_norm is not None:
            obs = self.obs_norm(obs)
        self.ou = OUNoise(self.action_dim, sigma=a.ou_sigma, dt=a.ou_dt, scale=a.init_scale) if a.trick["OUNoise"] else None
        if a.trick["GaussNoise"] and a.gauss_init_scale is not None:
            a.gauss_scale = a.gauss_init_scale
        return obs

    def act(self, step, obs):
        a, m = self.args, self.max_action
        if step < a.random_steps:                                    # SAC.py:522-525
            env_action = self.env.action_space.sample()
            return env_action / m, env_action, None
        action = self.policy.select_action(obs)
        if self.ou is not None:
            env_action = np.clip(action * m + self.ou.noise() * m, -m, m)
        elif a.trick["GaussNoise"]:
            env_action = np.clip(action * m + a.gauss_scale * np.random.normal(scale=a.gauss_sigma * m, size=self.action_dim), -m, m)
        else:
            env_action = np.clip(action * m, -m, m)
        return action, env_action, None

    def observe(self, next_obs, reward):
        return (self.obs_norm(next_obs) if self.obs_norm is not None else next_obs), reward

    def episode_end(self, episode_num):
        a = self.args
        if self.ou is not None:
            self.ou.reset()
            if a.init_scale is not None:
                self.ou.scale = a.final_scale + (a.init_scale - a.final_scale) * _remaining(a, episode_num)
        elif a.trick["GaussNoise"] and a.gauss_init_scale is not None:
            a.gauss_scale = a.gauss_final_scale + (a.gauss_init_scale - a.gauss_final_scale) * _remaining(a, episode_num)

    def after_reset(self, obs):
        return self.obs_norm(obs) if self.obs_norm is not None else obs

    def learn(self, episode_num):
        self.policy.learn(self.args.batch_size, self.args.gamma, self.args.tau)

    def finish(self, model_dir):
        if self.obs_norm is not None:                                # SAC.py:583-584
            np.save(os.path.join(model_dir, "%s_running_mean_std.npy" % self.args.policy_name),
                    np.array([self.obs_norm.running_ms.mean, self.obs_norm.running_ms.std]))


class _SACDiscreteHooks(_Hooks):
    """SAC_add_discrete.py:525-580: the action space's own sample before random_steps, Categorical draws after; the env takes the
    index as it is.  At the end: the Batch_ObsNorm running mean / std next to the checkpoint."""

    def act(self, step, obs):
        if step < self.args.random_steps:                            # :529-532
            action = self.env.action_space.sample()
        else:
            action = self.policy.select_action(obs)
        return action, action, None

    def learn(self, episode_num):
        self.policy.learn(self.args.batch_size, self.args.gamma, self.args.tau)

    def finish(self, model_dir):
        if self.args.trick.get("Batch_ObsNorm"):                     # :579-580
            ms = self.policy.batch_size_obs_norm.running_ms
            np.save(os.path.join(model_dir, "%s_running_mean_std_batch_size.npy" % self.args.policy_name),
                    np.array([ms.mean.numpy(), ms.std.numpy()]))


class _ReinforceHooks(_Hooks):
    """REINFORCE.py:289-323: every action is a Categorical draw; add(reward, terminated); learn(gamma) right after the reset that
    ends every learn_episodes_interval-th episode, between the two save points of the loop."""
    due = False

    def act(self, step, obs):
        action = self.policy.select_action(obs)
        return action, action, None

    def store(self, obs, action, reward, next_obs, terminated, done, extra):
        self.policy.add(reward, terminated)                          # :299

    def episode_end(self, episode_num):
        self.due = (episode_num + 1) % self.args.learn_episodes_interval == 0      # :318

    def learn_due(self, step):
        due, self.due = self.due, False
        return due

    def learn(self, episode_num):
        self.policy.learn(self.args.gamma)


class _PPOHooks(_Hooks):
    def begin(self, obs):
        t = self.args.trick
        self.obs_norm = _norm.Normalization(shape=self.dim_info[0]) if t["ObsNorm"] else None
        self.reward_norm = _norm.Normalization(shape=1) if t["reward_norm"] else None
        self.reward_scaling = _norm.RewardScaling(shape=1, gamma=self.args.gamma) if (t["reward_scaling"] and not t["reward_norm"]) else None
        return self.obs_norm(obs) if self.obs_norm is not None else obs

    def act(self, step, obs):
        action, log_pi = self.policy.select_action(obs)
        m = self.max_action
        env_action = np.clip(action * m, -m, m) if m is not None else action
        return action, env_action, log_pi

    def observe(self, next_obs, reward):
        if self.obs_norm is not None:
            next_obs = self.obs_norm(next_obs)
        if self.reward_norm is not None:
            reward = self.reward_norm(reward)
        elif self.reward_scaling is not None:
            reward = self.reward_scaling(reward)
        return next_obs, reward

    def store(self, obs, action, reward, next_obs, terminated, done, log_pi):
        self.policy.add(obs, action, reward, next_obs, terminated, log_pi, done)       # :542-546

    def after_reset(self, obs):
        if self.reward_scaling is not None:
            self.reward_scaling.reset()
        return self.obs_norm(obs) if self.obs_norm is not None else obs

    def learn_due(self, step):
        return step % self.args.horizon == 0

    def learn(self, episode_num):
        a = self.args
        self.policy.learn(a.minibatch_size, a.gamma, a.lmbda, a.clip_param, a.K_epochs, a.entropy_coefficient)
        if a.trick["lr_decay"]:
            self.policy.lr_decay(episode_num, max_episodes=a.max_episodes)

    def finish(self, model_dir):
        if self.obs_norm is not None:
            np.save(os.path.join(model_dir, "%s_running_mean_std.npy" % self.args.policy_name),
                    np.array([self.obs_norm.running_ms.mean, self.obs_norm.running_ms.std]))


def _run_loop(args, env, policy, hooks, model_dir, writer, log=print):
    """One env step per iteration (the reference's `while episode_num < max_episodes`)."""
    episode_num, step, episode_reward, returns = 0, 0, 0, []
    obs, _ = env.reset(seed=args.seed)
    if args.random_steps > 0:
        env.action_space.seed(seed=args.seed)
    obs = hooks.begin(obs)
    t0 = time.time()
    while episode_num < args.max_episodes:
        step += 1
        action, env_action, extra = hooks.act(step, obs)
        next_obs, reward, terminated, truncated, _ = env.step(env_action)
        next_obs, stored_reward = hooks.observe(next_obs, reward)
        done = terminated or truncated
        hooks.store(obs, action, stored_reward, next_obs, terminated, done, extra)   # done flag = terminated only
        episode_reward += reward
        obs = next_obs
        if done:
            hooks.episode_end(episode_num)
            if (episode_num + 1) % 100 == 0:
                log("episode: {}, reward: {}".format(episode_num + 1, episode_reward))
            if (episode_num + 1) % args.save_freq == 0 and not isinstance(hooks, (_SACHooks, _SACDiscreteHooks, _PPOHooks)):
                policy.save(model_dir)
            writer.add_scalar("reward", episode_reward, episode_num + 1)
            returns.append(episode_reward)
            episode_num += 1
            obs, _ = env.reset(seed=args.seed)          # same seed at every episode start (DQN.py:334)
            obs = hooks.after_reset(obs)
            episode_reward = 0
        if hooks.learn_due(step):
            hooks.learn(episode_num)
        if episode_num % args.save_freq == 0:           # fires on every step of those episodes (DQN.py:342-343)
            policy.save(model_dir)
    log("total_time:", time.time() - t0)
    policy.save(model_dir)
    np.save(os.path.join(model_dir, "%s_seed_%d.npy" % (args.policy_name, args.seed)), np.array(returns))
    hooks.finish(model_dir)
    return dict(returns=np.array(returns), steps=step, seconds=time.time() - t0)


def _run_maddpg(args, env, policy, dim_info, max_action, model_dir, writer, log=print):
    """MADDPG_simple.py:336-395: dict-in/dict-out parallel env, per-agent returns."""
    agents = list(env.agents)
    episode_num, step = 0, 0
    episode_reward = {a: 0 for a in agents}
    returns = {a: [] for a in agents}
    obs, _ = env.reset(seed=args.seed)
    for a in agents:
        env.action_space(a).seed(seed=args.seed)
    if args.gauss_init_scale is not None:
        args.gauss_scale = args.gauss_init_scale
    t0 = time.time()
    while episode_num < args.max_episodes:
        step += 1
        if step < args.random_steps:
            env_action = {a: env.action_space(a).sample() for a in agents}
            action = {a: (env_action[a] * 2 - 1) * max_action for a in agents}
        else:
            action = policy.select_action(obs)
            env_action = {}
            for a in agents:        # one NumPy draw per agent, in env.agents order (:350)
                noisy = action[a] * max_action + args.gauss_scale * np.random.normal(scale=args.gauss_sigma * max_action, size=dim_info[a][1])
                env_action[a] = (np.clip(noisy, -max_action, max_action).astype(np.float32) + 1) / 2
        next_obs, reward, terminated, truncated, _ = env.step(env_action)
        done = {a: terminated[a] or truncated[a] for a in agents}
        policy.add(obs, action, reward, next_obs, {a: terminated[a] for a in agents})
        for a, r in reward.items():
            episode_reward[a] += r
        obs = next_obs
        if any(done.values()):
            if args.gauss_init_scale is not None:
                args.gauss_scale = args.gauss_final_scale + (args.gauss_init_scale - args.gauss_final_scale) * _remaining(args, episode_num)
            if (episode_num + 1) % 100 == 0:
                log("episode: {}, reward: {}".format(episode_num + 1, episode_reward))
            for a, r in episode_reward.items():
                writer.add_scalar("reward_%s" % a, r, episode_num + 1)
                returns[a].append(r)
            episode_num += 1
            obs, _ = env.reset(seed=args.seed)
            episode_reward = {a: 0 for a in agents}
        if step > args.start_steps and step % args.learn_steps_interval == 0:
            policy.learn(args.batch_size, args.gamma, args.tau)
        if getattr(args, "save_freq", None) and episode_num % args.save_freq == 0:      # (MADDPG_simple_with_tricks.py has no such block)
            policy.save(model_dir)
    log("total_time:", time.time() - t0)
    policy.save(model_dir)
    arr = np.array([returns[a] for a in agents])
    suffix = "" if args.N is None else "_N_%d" % len(agents)
    np.save(os.path.join(model_dir, "%s_seed_%d%s.npy" % (args.policy_name, args.seed, suffix)), arr)
    return dict(returns=arr, steps=step, seconds=time.time() - t0)


def _run_masac(args, env, policy, dim_info, max_action, model_dir, writer, log=print):
    """MASAC.py:417-474: the policy samples its own exploration (no action noise), the env is reset without a seed, and the returns are
    kept for every 100th episode only."""
    agents = list(env.agents)
    episode_num, step = 0, 0
    episode_reward = {a: 0 for a in agents}
    returns = {a: [] for a in agents}
    obs, _ = env.reset()
    for a in agents:
        env.action_space(a).seed(seed=args.seed)
    t0 = time.time()
    while episode_num < args.max_episodes:
        step += 1
        if step < args.random_steps:
            env_action = {a: env.action_space(a).sample() for a in agents}
            action = {a: (env_action[a] * 2 - 1) * max_action for a in agents}
        else:
            action = policy.select_action(obs)
            env_action = {a: (action[a] + 1) / 2 * max_action for a in agents}
        next_obs, reward, terminated, truncated, _ = env.step(env_action)
        done = {a: terminated[a] or truncated[a] for a in agents}
        policy.add(obs, action, reward, next_obs, {a: done[a] if not truncated[a] else False for a in agents})
        episode_reward = {a: episode_reward[a] + reward[a] for a in agents}
        obs = next_obs
        if any(done.values()):
            if (episode_num + 1) % 100 == 0:
                log("episode: {}, reward: {}".format(episode_num + 1, episode_reward))
                for a in agents:
                    writer.add_scalar("reward_%s" % a, episode_reward[a], episode_num + 1)
                    returns[a].append(episode_reward[a])
            episode_num += 1
            obs, _ = env.reset()
            episode_reward = {a: 0 for a in agents}
        if step > args.start_steps and step % args.learn_steps_interval == 0:
            policy.learn(args.batch_size, args.gamma, args.tau)
        if episode_num % args.save_freq == 0:
            policy.save(model_dir)
    log("total_time:", time.time() - t0)
    policy.save(model_dir)
    arr = np.array([returns[a] for a in agents])
    suffix = "" if args.N is None else "_N_%d" % len(agents)
    np.save(os.path.join(model_dir, "%s_seed_%d%s.npy" % (args.policy_name, args.seed, suffix)), arr)
    return dict(returns=arr, steps=step, seconds=time.time() - t0)


def _run_cem_gd3pg(args, env, policy, dim_info, max_action, model_dir, writer, log=print):
    """CEM_GD3PG.py:364-486: the population's first evaluations into `buffer`; then per episode — every pop_size episodes a generation
    step (tell, ask, evaluate the new half into `buffer`, mix the best into the poorer actor with weight 0.5) —, the two fitness
    episodes, the running fitness averages and delta, the noisy domain episode into `buffer_domain`, and one learn() per step of it."""
    from .CEM_GD3PG import sepCEM
    action_dim, n = dim_info[1], args.pop_size
    t0 = time.time()

    def eval_actor(actor, buffer=None, noise=False):
        """one episode (:370-396) -> (return, steps); stores into `buffer`, explores with Gaussian noise when `noise`"""
        episode_reward, steps = 0, 0
        obs, _ = env.reset(seed=args.seed)
        done = False
        while not done:
            action = policy.select_action(obs, actor)
            if noise:
                action_ = np.clip(action * max_action + np.random.normal(scale=args.gauss_sigma * max_action, size=action_dim), -max_action, max_action)
            else:
                action_ = action * max_action
            next_obs, reward, terminated, truncated, _ = env.step(action_)
            done = terminated or truncated
            if buffer is not None:
                policy.add(buffer, obs, action, reward, next_obs, done if not truncated else False)
            episode_reward += reward
            steps += 1
            obs = next_obs
        return episode_reward, steps

    ag = policy.agent
    actor_1, actor_2, actor_domain = ag.actor_1, ag.actor_2, ag.actor_domain
    es = sepCEM(actor_1.get_size(), mu_init=actor_1.get_params(), sigma_init=args.sigma_init, damp=args.damp, damp_limit=args.damp_limit,
                pop_size=n, antithetic=not n % 2, parents=n // 2, elitism=args.elitism)
    f1_total = f2_total = 0
    cnt_es, episode_num, step, train_return = 0, 0, 0, []
    env.reset(seed=args.seed)
    es_params = es.ask(n * 2)
    fitness = []
    for i in range(n):                                   # `buffer` starts pop_size episodes ahead of `buffer_domain` (:415-418)
        actor_domain.set_params(es_params[i])
        fitness.append(eval_actor(actor_domain, policy.buffer)[0])
    while episode_num < args.max_episodes:
        if cnt_es == n:
            es.tell(es_params, fitness)
            half = es.ask(n)
            fitness, cnt_es = [], 0
            for params in half:
                actor_domain.set_params(params)
                fitness.append(eval_actor(actor_domain, policy.buffer)[0])
            best = int(np.argsort(fitness)[-1])
            log("select best actor : Actor%d ,fitness :%s" % (best, fitness[best]))
            poorer = actor_2 if f1_total >= f2_total else actor_1
            poorer.set_params((half[best] + poorer.get_params()) / 2)          # pi_poor = (1 - beta) pi_best + beta pi_poor, beta = 0.5 (:436)
            es_params[:n] = half
        f1, f2 = eval_actor(actor_1)[0], eval_actor(actor_2)[0]
        f1_total = 0.8 * f1_total + 0.2 * f1                                   # alpha = 0.2 (:445)
        f2_total = 0.8 * f2_total + 0.2 * f2
        hi, lo, better = (f1_total, f2_total, actor_1) if f1_total >= f2_total else (f2_total, f1_total, actor_2)
        actor_domain.set_params(better.get_params())
        delta = min(1, 1 - lo / hi) if hi > 0 else 1 - hi / lo                 # (:447-460)
        es_params[cnt_es + n] = actor_domain.get_params()
        fitness.append(max(f1, f2))
        cnt_es += 1
        episode_reward, steps = eval_actor(actor_domain, policy.buffer_domain, noise=True)
        args.gauss_sigma = max(0.05, args.gauss_sigma * 0.999)
        if (episode_num + 1) % 100 == 0:
            log("episode: {}, reward: {}".format(episode_num + 1, episode_reward))
        writer.add_scalar("reward_domain", episode_reward, episode_num + 1)
        train_return.append(episode_reward)
        episode_num += 1
        step += steps
        if step > args.start_steps:
            for _ in range(steps):
                policy.learn(args.batch_size, args.gamma, args.tau, f1_total >= f2_total, delta, actor_domain)
    log("total_time:", time.time() - t0)
    policy.save(model_dir, actor_domain)
    np.save(os.path.join(model_dir, "%s_seed_%d.npy" % (args.policy_name, args.seed)), np.array(train_return))
    return dict(returns=[float(r) for r in train_return], steps=step, seconds=time.time() - t0)


def _mappo_policy_name(args, base):
    """MAPPO.py:573-588 / IPPO.py:451-465 / HAPPO.py:586-601: the policy name decides the tricks — `MAPPO` switches all on but reward_norm and lr_decay,
    `MAPPO_simple` all off"""
    t = args.trick
    if t["reward_norm"] and t["reward_scaling"]:
        raise ValueError("reward_norm and reward_scaling are mutually exclusive")
    if args.policy_name == base or (t["lr_decay"] is False and all(v for k, v in t.items() if k not in ("reward_norm", "lr_decay"))):
        args.policy_name = base
        for k in t:
            t[k] = k not in ("reward_norm", "lr_decay")
    if args.policy_name == base + "_simple" or not any(t.values()):
        args.policy_name = base + "_simple"
        for k in t:
            t[k] = False


def _run_mappo(args, env, policy, dim_info, max_action, is_continue, model_dir, writer, log=print):
    """MAPPO.py:617-700 = IPPO.py:495-579 = HAPPO.py:631-713: dict-in/dict-out parallel env, one learn() every `horizon` steps; ObsNorm,
    reward_norm and reward_scaling live here, per agent.  HAPPO.py:681-685 writes and keeps an episode's return only where it prints
    it, every 100th episode"""
    import pickle
    agents = list(env.agents)
    sparse_returns = args.policy_name.startswith("HAPPO")
    episode_num, step = 0, 0
    episode_reward = {a: 0 for a in agents}
    returns = {a: [] for a in agents}
    obs, _ = env.reset(seed=args.seed)
    for a in agents:
        env.action_space(a).seed(seed=args.seed)
    t = args.trick
    if t["ObsNorm"]:
        obs_norm = {a: _norm.Normalization(shape=dim_info[a][0]) for a in agents}
        obs = {a: obs_norm[a](obs[a]) for a in agents}
    if t["reward_norm"]:
        reward_norm = {a: _norm.Normalization(shape=1) for a in agents}
    elif t["reward_scaling"]:
        reward_norm = {a: _norm.RewardScaling(shape=1, gamma=args.gamma) for a in agents}
    t0 = time.time()
    while episode_num < args.max_episodes:
        step += 1
        action, action_log_pi = policy.select_action(obs)
        if is_continue:
            env_action = {a: (np.clip(action[a] * max_action, -max_action, max_action, dtype=np.float32) + 1) / 2 for a in agents}
        else:
            env_action = {a: int(action[a]) for a in agents}
        next_obs, reward, terminated, truncated, _ = env.step(env_action)
        if t["ObsNorm"]:
            next_obs = {a: obs_norm[a](next_obs[a]) for a in agents}
        done = {a: terminated[a] or truncated[a] for a in agents}
        done_bool = {a: terminated[a] for a in agents}
        if t["reward_norm"] or t["reward_scaling"]:
            # (IPPO.py:530 takes element [0] of the (1,) array, MAPPO.py:659 stores the array: the same float either way)
            reward_ = {a: float(np.asarray(reward_norm[a](reward[a])).reshape(-1)[0]) for a in agents}
            policy.add(obs, action, reward_, next_obs, done_bool, action_log_pi, done)
        else:
            policy.add(obs, action, reward, next_obs, done_bool, action_log_pi, done)
        episode_reward = {a: episode_reward[a] + reward[a] for a in agents}
        obs = next_obs
        if any(done.values()):
            if (episode_num + 1) % 100 == 0:
                log("episode: {}, reward: {}".format(episode_num + 1, episode_reward))
            if not sparse_returns or (episode_num + 1) % 100 == 0:
                for a in agents:
                    writer.add_scalar("reward_%s" % a, episode_reward[a], episode_num + 1)
                    returns[a].append(episode_reward[a])
            episode_num += 1
            obs, _ = env.reset(seed=args.seed)
            if t["ObsNorm"]:
                obs = {a: obs_norm[a](obs[a]) for a in agents}
            if t["reward_scaling"]:
                for a in agents:
                    reward_norm[a].reset()
            episode_reward = {a: 0 for a in agents}
        if step % args.horizon == 0:
            policy.learn(args.minibatch_size, args.gamma, args.lmbda, args.clip_param, args.K_epochs, args.entropy_coefficient, args.huber_delta)
            if t["lr_decay"]:
                policy.lr_decay(episode_num, max_episodes=args.max_episodes)
        if episode_num % args.save_freq == 0:
            policy.save(model_dir)
    log("total_time:", time.time() - t0)
    policy.save(model_dir)
    arr = np.array([returns[a] for a in agents])
    suffix = "" if args.N is None else "_N_%d" % len(agents)
    np.save(os.path.join(model_dir, "%s_seed_%d%s.npy" % (args.policy_name, args.seed, suffix)), arr)
    if t["ObsNorm"]:
        with open(os.path.join(model_dir, "obs_norm.pkl"), "wb") as f:
            pickle.dump({a: [obs_norm[a].running_ms.mean, obs_norm[a].running_ms.std] for a in agents}, f)
    return dict(returns=arr, steps=step, seconds=time.time() - t0)


# ------------------------------------------------------------------------------------ drivers
def run(algo, argv=None, env=None, log=print):
    """Parse the reference's flags for `algo`, build env + policy, run the loop, return a dict
    (model_dir, returns, steps, seconds, policy)."""
    args = build_parser(algo).parse_args(argv)
    if algo in ("gail_ppo", "gail"):
        return _run_gail(algo, args, env, log)
    if algo == "td3" and args.policy_name == "TD3":
        args.realize = {"clip_double": True, "policy_noise": True, "twin_delay": True}      # TD3.py:357-358
    if algo == "ppo" and args.trick["reward_norm"] and args.trick["reward_scaling"]:
        raise ValueError("reward_norm and reward_scaling are mutually exclusive")
    log(args)
    log("-" * 50)
    log("Algorithm:", args.policy_name)
    device = torch.device(args.device) if torch.cuda.is_available() else torch.device("cpu")
    if algo in _MA_PPO:
        _mappo_policy_name(args, algo.upper())
    if algo in _MA_REPLAY or algo in _MA_PPO:
        if algo not in _MA_REPLAY and not args.continuous_actions and env is None:
            raise ValueError("the in-repo multi-agent environments have continuous actions: pass --continuous_actions True, or an env of your own")
        env = env if env is not None else _envs.make_parallel(args.env_name, args.N)
        env.reset()
        is_continue = algo in _MA_REPLAY or hasattr(env.action_space(env.agents[0]), "low")
        dim_info = {a: [env.observation_space(a).shape[0], env.action_space(a).shape[0] if is_continue else env.action_space(a).n] for a in env.agents}
        max_action = 1 if is_continue else None
    else:
        if env is None:
            env, dim_info, max_action, is_continue = get_env(args.env_name, args.is_dis_to_con)
        else:
            _, dim_info, max_action, is_continue = _space_info(env, args.is_dis_to_con)
    np.random.seed(args.seed)                       # seeds AFTER env creation, BEFORE the policy (DQN.py:260-266)
    torch.manual_seed(args.seed)
    # (the two multi-agent PPO scripts' make_dir leaves the trick names out of the folder's name: MAPPO.py:512-518)
    model_dir = make_dir(args.results_root, args.env_name, policy_name=args.policy_name, trick=None if algo in _MA_PPO else args.trick)
    log("model_dir:", model_dir)
    writer = ScalarWriter(model_dir)
    # the engine's Philox key follows --seed too: with rng="auto" the index / noise draws move from the seeded NumPy / torch
    # streams to the device generator once the buffer holds _core.AUTO_DEVICE_MIN_ROWS rows, and two --seed values must not
    # share that stream
    kw = dict(rng=args.rng, seed=args.seed)
    if args.rng == "auto":
        from ._core import AUTO_DEVICE_MIN_ROWS
        log("rng=auto: index / noise draws follow the reference's host streams below %d buffer rows, the device "
            "generator (keyed by --seed) from there on; --rng host keeps the reference's streams throughout" % AUTO_DEVICE_MIN_ROWS)
    if algo == "dqn":
        from .DQN import DQN
        policy = DQN(dim_info, is_continue, Qnet_lr=args.Qnet_lr, buffer_size=args.buffer_size, device=device, **kw)
        hooks = _DQNHooks(args, env, policy, dim_info, max_action)
    elif algo == "ddpg":
        from .DDPG import DDPG
        policy = DDPG(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, trick=args.trick, **kw)
        hooks = _GaussHooks(args, env, policy, dim_info, max_action)
    elif algo == "her":
        import random
        from .DDPG_simple_try_HER import DDPG
        if not is_continue:
            raise ValueError("her trains on continuous action spaces (DDPG_simple_try_HER.py); %s is discrete" % args.env_name)
        random.seed(args.seed)                      # :342, the relabel's random.sample stream
        dim_info = [dim_info[0] + dim_info[0], dim_info[1]]         # obs + goal (:357)
        policy = DDPG(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, trick=args.trick, **kw)
        hooks = _HERHooks(args, env, policy, dim_info, max_action)
    elif algo == "td3":
        from .TD3 import TD3
        policy = TD3(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, trick=args.trick,
                     realize=args.realize, **kw)
        hooks = _GaussHooks(args, env, policy, dim_info, max_action)
    elif algo == "sac":
        from .SAC import SAC
        policy = SAC(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, trick=args.trick, **kw)
        hooks = _SACHooks(args, env, policy, dim_info, max_action)
    elif algo == "sac_discrete":
        from .SAC import SAC
        if is_continue:
            raise ValueError("sac_discrete trains on discrete action spaces (SAC_add_discrete.py); %s is continuous" % args.env_name)
        policy = SAC(dim_info, False, args.actor_lr, args.critic_lr, args.buffer_size, device, trick=args.trick, **kw)
        hooks = _SACDiscreteHooks(args, env, policy, dim_info, max_action)
    elif algo == "reinforce":
        from .REINFORCE import REINFORCE
        # the steps between two learn() calls: learn_episodes_interval episodes of at most the env's time limit each
        limit = getattr(env, "max_episode_steps", None) or getattr(getattr(env, "spec", None), "max_episode_steps", None) or 1000
        policy = REINFORCE(dim_info, is_continue, args.policy_net_lr, device, trick=args.trick,
                           max_steps=max(2048, int(limit) * args.learn_episodes_interval), seed=args.seed)
        hooks = _ReinforceHooks(args, env, policy, dim_info, max_action)
    elif algo == "ppo":
        from .PPO import PPO
        policy = PPO(dim_info, is_continue, args.actor_lr, args.critic_lr, args.horizon, device, trick=args.trick,
                     beta=args.beta, **kw)
        hooks = _PPOHooks(args, env, policy, dim_info, max_action)
    elif algo == "maddpg":
        from .MADDPG import MADDPG
        policy = MADDPG(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, args.trick, **kw)
        out = _run_maddpg(args, env, policy, dim_info, max_action, model_dir, writer, log)
        writer.close()
        return dict(out, model_dir=model_dir, policy=policy, args=args)
    elif algo == "maddpg_att":
        from .MADDPG_simple_with_tricks import MADDPG
        policy = MADDPG(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, args.trick, **kw)
        out = _run_maddpg(args, env, policy, dim_info, max_action, model_dir, writer, log)
        writer.close()
        return dict(out, model_dir=model_dir, policy=policy, args=args)
    elif algo == "masac":
        from .MASAC import MASAC
        policy = MASAC(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, args.trick, **kw)
        out = _run_masac(args, env, policy, dim_info, max_action, model_dir, writer, log)
        writer.close()
        return dict(out, model_dir=model_dir, policy=policy, args=args)
    elif algo == "cem_gd3pg":
        from .CEM_GD3PG import CEM_GD3PG
        if not is_continue:
            raise ValueError("cem_gd3pg trains on continuous action spaces (CEM_GD3PG.py:296-298); %s is discrete" % args.env_name)
        policy = CEM_GD3PG(dim_info, is_continue, args.actor_lr, args.critic_lr, args.buffer_size, device, args.trick, batch_max=max(args.batch_size, 2), **kw)
        out = _run_cem_gd3pg(args, env, policy, dim_info, max_action if max_action is not None else args.max_action, model_dir, writer, log)
        writer.close()
        return dict(out, model_dir=model_dir, policy=policy, args=args)
    elif algo in _MA_PPO:
        from .HAPPO import HAPPO
        from .IPPO import IPPO
        from .MAPPO import MAPPO
        cls = dict(mappo=MAPPO, ippo=IPPO, happo=HAPPO)[algo]
        # (these classes draw their permutations from np.random like the scripts unless --rng device is asked for)
        policy = cls(dim_info, is_continue, args.actor_lr, args.critic_lr, args.horizon, device, args.trick,
                     rng="device" if args.rng == "device" else "host", seed=args.seed, minibatch_max=max(args.minibatch_size, 1))
        out = _run_mappo(args, env, policy, dim_info, max_action, is_continue, model_dir, writer, log)
        writer.close()
        return dict(out, model_dir=model_dir, policy=policy, args=args)
    else:
        raise ValueError(algo)
    out = _run_loop(args, env, policy, hooks, model_dir, writer, log)
    writer.close()
    return dict(out, model_dir=model_dir, policy=policy, args=args)


def _run_gail(algo, args, env, log):
    """`python GAIL_file/PPO2.py` (gail_ppo: the policy alone, eval_data.npz written at the end) and `python GAIL_file/GAIL.py` (gail:
    the adversarial loop on --expert, an eval_data.npz such a run wrote) with config.py's values as flags."""
    from .PPO2 import PPO, gymEnvWrapper
    env = env if env is not None else _envs.make(args.env_name)
    s_dim = env.observation_space.shape[0]
    a_dim = env.action_space.n if args.discrete else env.action_space.shape[0]
    config = dict(id=args.env_name, log_dir=os.path.join(args.results_root, args.env_name), algo="PPO" if algo == "gail_ppo" else "GAIL", seed=args.seed,
                  env_reproducible=args.env_reproducible, collect_eval_data=args.collect_eval_data, num_workers=1, use_gpu=True, s_dim=s_dim,
                  a_dim=a_dim, discrete=args.discrete,
                  PPO=dict(policy_mlp_dim=args.policy_mlp_dim, activation=args.activation, dropout=0.0, layernorm=False, log_std_min=args.log_std_min,
                           log_std_max=args.log_std_max, p_lr=args.p_lr, v_lr=args.v_lr, horizon=args.horizon, gamma=args.gamma, lam=args.lam,
                           clip_epsilon=args.clip_epsilon, K_epochs=args.K_epochs, value_loss_coef=args.value_loss_coef, ent_weight=args.ent_weight,
                           mini_batch_size=args.mini_batch_size, eval_interval=args.eval_interval, eval_episodes=args.eval_episodes))
    log(config)
    t0 = time.time()
    wrapper = gymEnvWrapper(env, config)
    if algo == "gail_ppo":
        ppo = PPO(config, rng="device" if args.rng == "device" else "host", seed=args.seed)
        ppo.train(wrapper, num_episodes=args.max_episodes)
        policy = ppo
    else:
        from .GAIL import GAIL, ExpertDataset, create_expert_loader
        if not args.expert:
            raise ValueError("gail needs --expert PATH: an eval_data.npz with `states` and `actions` (what `gail_ppo` writes at the end)")
        config["expert_data_path"] = args.expert
        config["D"] = dict(d_mlp_dim=args.d_mlp_dim, activation=args.d_activation, dropout=0.0, layernorm=False, d_lr=args.d_lr, gp_coef=args.gp_coef)
        gail = GAIL(config, ppo=PPO(config, rng="device" if args.rng == "device" else "host", seed=args.seed), max_rows=args.horizon, seed=args.seed)
        gail.train(wrapper, create_expert_loader(ExpertDataset(args.expert), config), args.max_episodes)
        policy, ppo = gail, gail.ppo
    return dict(model_dir=ppo.config["log_dir"], returns=[float(r) for r in ppo.train_return], steps=ppo.step, seconds=time.time() - t0, policy=policy,
                args=args)


def _space_info(env, is_dis_to_con):
    obs_space, act_space = env.observation_space, env.action_space
    obs_dim = obs_space.shape[0] if hasattr(obs_space, "low") else 1
    if hasattr(act_space, "low"):
        ad = act_space.shape[0]
        if is_dis_to_con:
            return env, [obs_dim, 16 if ad == 1 else 2 ** ad], act_space.high[0], False
        return env, [obs_dim, ad], act_space.high[0], True
    return env, [obs_dim, act_space.n], None, False


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in FLAGS:
        raise SystemExit("usage: python -m freerl_amd.train {%s} [reference flags]" % "|".join(FLAGS))
    run(argv[0], argv[1:])


if __name__ == "__main__":
    main()
