"""`GAIL`'s discriminator (generative adversarial imitation learning) with the reference's class surface
(GAIL_file/GAIL.py:17-120, GAIL_file/GAIL_utils.py:9-56), backed by the HIP engine.

    dataset = ExpertDataset("eval_data.npz")            # or ExpertDataset((states, actions)); min-max scaled to [-1, 1] once
    gail = GAIL(config)                                  # config['s_dim'], ['a_dim'], ['seed'], ['D'] = {d_mlp_dim, activation, ...}
    gail.load_expert(dataset)                            # the expert rows become the engine's ring
    idx = gail.next_expert_indices(batch)                # torch.randint, as InfiniteUniformSampler draws
    d_loss, expert_prob, policy_prob, w_dis = gail.trian_D_indices(idx, policy_states, policy_actions)
    d_loss, expert_prob, policy_prob, w_dis = gail.trian_D(expert_states, expert_actions, policy_states, policy_actions)
    rewards = gail.compute_reward(states, actions)       # float32 tensor
    gail.D_model.state_dict() / gail.D_optimizer.param_groups[0]['betas']

`trian_D` (the reference's spelling) is one launch chain (kernels_gail.hip): forward of the expert and policy rows, the loss of the
mode, the backward — with `gp_coef > 0` including the gradient penalty's second-order part in closed form — and one Adam step; the
net and Adam's state stay on the GPU.  `gp_coef > 0` (the shipped config: 10) trains on logits with 0.5 x BCE-with-logits plus the
reference's literal 5 x the penalty on the expert rows and Adam betas (0.5, 0.9); `gp_coef == 0` on sigmoid + BCE with betas
(0.9, 0.999).

The policy side is `freerl_amd.PPO2.PPO` (GAIL_file/PPO2.py on kernels_gail_ppo.hip).  Pass one to take part in the loop:

    gail = GAIL(config, ppo=PPO(config))                 # the reference's `self.ppo = PPO(config)`, made by the caller
    loader = create_expert_loader(dataset, config)       # infinite: torch.randint batches of config['PPO']['horizon'] rows
    gail.train(gymEnvWrapper(env, config), loader, num_episodes)

`train` is GAIL.py:122-179: explore one horizon, `trian_D` on an expert batch and the policy's rows, `compute_reward`, the rewards
replace the env's in the batch, `last_value = ppo.value(ppo.state)`, `PPO_learn`, `eval_and_save`; `train_post` at the end.  The
rewards make one host round trip of 4 x horizon bytes between the two engines.  Without a `ppo`, `train()` raises
NotImplementedError.  A discrete policy is refused in `train` (ValueError): the reference concatenates the long action index into the
discriminator's float input, and its shipped discrete config has a_dim = 2 against the one stored column.

Refused with ValueError: an activation other than 'LeakyReLU' / 'ReLU', `layernorm=True`, `dropout > 0` — the penalty's
closed form needs a piecewise-linear net, and nothing in the shipped config uses them — and an expert column that is constant (the
reference divides by zero there and trains on NaN).
"""
import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, OptimizerView, init_layers

F32 = np.float32
GP_WEIGHT = 5.0                 # GAIL.py:98: `d_loss += 5 * disc_grad_penalty`, whatever gp_coef says
_ACTIVATIONS = {"LeakyReLU": N.ACT_LEAKY_RELU, "ReLU": N.ACT_RELU}


def _np(x, dtype=F32):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


class ExpertDataset:
    """GAIL_utils.ExpertDataset: `states` and `actions` of an .npz file (or a (states, actions) pair of arrays), each column
    min-max scaled to [-1, 1] once; the four bound arrays keep the reference's names."""

    def __init__(self, file_path_or_arrays):
        if isinstance(file_path_or_arrays, (tuple, list)):
            states, actions = file_path_or_arrays
        else:
            data = np.load(file_path_or_arrays)
            states, actions = data["states"], data["actions"]
        states, actions = np.asarray(states), np.asarray(actions)
        if states.ndim != 2 or actions.ndim != 2 or len(states) != len(actions) or len(states) < 1:
            raise ValueError("expert states / actions must be [n, s_dim] / [n, a_dim] with the same n >= 1")
        self.space_low, self.space_high = states.min(axis=0), states.max(axis=0)
        self.action_low, self.action_high = actions.min(axis=0), actions.max(axis=0)
        self.s_space = [list(self.space_low), list(self.space_high)]
        self.a_space = [list(self.action_low), list(self.action_high)]
        for name, lo, hi in (("states", self.space_low, self.space_high), ("actions", self.action_low, self.action_high)):
            flat = np.nonzero(hi == lo)[0]
            if flat.size:
                raise ValueError("expert %s column %d is constant (%r): min-max scaling would divide by zero" % (name, int(flat[0]), lo[flat[0]]))
        self.states = 2 * (states - self.space_low) / (self.space_high - self.space_low) - 1
        self.actions = 2 * (actions - self.action_low) / (self.action_high - self.action_low) - 1

    def __len__(self):
        return len(self.states)

    def __getitem__(self, idx):
        return torch.as_tensor(self.states[idx], dtype=torch.float32), torch.as_tensor(self.actions[idx], dtype=torch.float32)


class Discriminator(DeviceNet):
    """`Discriminator` (GAIL.py:17-28): state_dict keys backbone.{0,1,2}.{weight,bias}; calling it returns the logits with
    `gp_coef > 0` and sigmoid(logits) without."""

    def __init__(self, engine, layers, gp):
        super().__init__(engine, 0, layers)
        self._gp = gp

    def __call__(self, *inputs):
        out = super().__call__(*inputs)
        return out if self._gp else torch.sigmoid(out)


class GAIL:
    def __init__(self, config, ppo=None, *, max_rows=None, seed=0):
        D = config["D"]
        if D["activation"] not in _ACTIVATIONS:
            raise ValueError("D.activation %r: the discriminator's kernels take 'LeakyReLU' or 'ReLU' (the gradient penalty is "
                             "differentiated in closed form, which needs a piecewise-linear activation)" % (D["activation"],))
        if D.get("layernorm", False):
            raise ValueError("D.layernorm=True is not supported (the shipped config has layernorm False)")
        if D.get("dropout", 0.0) > 0:
            raise ValueError("D.dropout > 0 is not supported (the shipped config has dropout 0)")
        self.global_seed(config["seed"])
        self.config = config
        self.device = torch.device("cpu")                  # where returned tensors live; the compute device is the HIP GPU
        self.s_dim, self.a_dim, H = int(config["s_dim"]), int(config["a_dim"]), int(D["d_mlp_dim"])
        self.gp = float(D.get("gp_coef", 0)) > 0
        self._hidden, self._act, self._seed = H, _ACTIVATIONS[D["activation"]], seed
        self._max_rows = int(max_rows) if max_rows is not None else None
        self._layers = [("backbone.0", H, self.s_dim + self.a_dim), ("backbone.1", H, H), ("backbone.2", 1, H)]
        self._init = init_layers(self._layers)             # torch RNG: the three nn.Linear of mlp(), in order
        self._betas = (0.5, 0.9) if self.gp else (0.9, 0.999)
        self._e = None
        self._make_engine(1, None)
        self.ppo = ppo                                     # a freerl_amd.PPO2.PPO, or None: train() needs one
        if ppo is not None and hasattr(ppo, "consume_init_draws"):
            ppo.consume_init_draws()                       # GAIL.py:49 constructs its PPO here: re-seed, the draws of P and V
        self._expert = None

    def _make_engine(self, capacity, rows):
        """(Re)create the engine around the current net and Adam state: the ring's capacity is the number of expert rows."""
        state = None
        if self._e is not None:
            state = [self._e.get_params(0, k) for k in (N.PARAM_ONLINE, N.PARAM_ADAM_M, N.PARAM_ADAM_V)] + [self._e.opt_step(0)]
            self._e.close()
        batch_max = self._max_rows if self._max_rows is not None else 2048
        self._e = Engine(N.ALGO_GAIL, self.s_dim, self.a_dim, max(int(capacity), 1), hidden=self._hidden, hidden_act=self._act,
                         batch_max=batch_max, seed=self._seed)
        if state is None:
            self._e.set_params(0, self._init, N.PARAM_ONLINE)
        else:
            for kind, flat in zip((N.PARAM_ONLINE, N.PARAM_ADAM_M, N.PARAM_ADAM_V), state[:3]):
                self._e.set_params(0, flat, kind)
            self._e.set_opt_step(0, state[3])
        lr = self.D_optimizer.lr if hasattr(self, "D_optimizer") else self.config["D"]["d_lr"]
        self.D_model = Discriminator(self._e, self._layers, self.gp)
        self.D_optimizer = OptimizerView(self._e, 0, lr)
        self.D_optimizer.param_groups[0]["betas"] = self._betas
        self.D_optimizer.defaults = dict(self.D_optimizer.param_groups[0])
        if rows is not None:
            rec = np.zeros((len(rows), self._e.width), F32)
            rec[:, :self.s_dim + self.a_dim] = rows            # obs and act are the record's first columns; the rest is not read
            self._e.add_batch(rec)
            self._e.flush()

    def global_seed(self, seed):
        torch.manual_seed(seed)
        np.random.seed(seed)

    # ------------------------------------------------------------------ expert rows
    def load_expert(self, dataset):
        """The dataset's (scaled) rows become the engine's ring; the net and Adam's state are kept."""
        rows = np.concatenate([_np(dataset.states), _np(dataset.actions)], axis=1)
        if rows.shape[1] != self.s_dim + self.a_dim:
            raise ValueError("expert rows have %d columns, config says s_dim + a_dim = %d" % (rows.shape[1], self.s_dim + self.a_dim))
        self._expert = dataset
        self._make_engine(len(rows), rows)

    def next_expert_indices(self, batch):
        """InfiniteUniformSampler (GAIL_utils.py:51-56): `batch` rows with replacement from torch's global generator."""
        if self._expert is None:
            raise RuntimeError("load_expert(dataset) first")
        return torch.randint(high=len(self._expert), size=(int(batch),), dtype=torch.int64).numpy()

    # ------------------------------------------------------------------ training
    def _learn(self, idx, policy_rows):
        o = self._e.gail_learn(policy_rows[None], gp=self.gp, lr=self.D_optimizer.lr, beta1=self._betas[0], beta2=self._betas[1],
                               gp_weight=GP_WEIGHT, adam_eps=self.D_optimizer.param_groups[0]["eps"], idx=np.asarray(idx, np.int64)[None])["out"][0]
        self.last_penalty, self.last_grad_norm = float(o[4]), float(o[5])
        return float(o[0]), float(o[1]), float(o[2]), (float(o[3]) if self.gp else 0.0)

    def trian_D_indices(self, idx, policy_states, policy_actions):
        """trian_D on the resident ring: expert rows `idx` of the loaded dataset."""
        if self._expert is None:
            raise RuntimeError("load_expert(dataset) first")
        return self._learn(idx, np.concatenate([_np(policy_states), _np(policy_actions)], axis=1))

    def trian_D(self, expert_states, expert_actions, policy_states, policy_actions):
        """GAIL.trian_D (:75-120) -> (d_loss, expert_prob, policy_prob, w_dis).  The expert rows are uploaded as given (they replace
        the ring's content); trian_D_indices is the fast path on a loaded dataset."""
        rows = np.concatenate([_np(expert_states), _np(expert_actions)], axis=1)
        self._expert = None
        if len(rows) > self._e.capacity or len(rows) > self._e.batch_max:
            self._max_rows = max(self._e.batch_max, len(rows))
            self._make_engine(len(rows), None)
        rec = np.zeros((len(rows), self._e.width), F32)
        rec[:, :rows.shape[1]] = rows
        self._e.set_cursor(0, 0, 0)
        self._e.add_batch(rec)
        return self._learn(np.arange(len(rows)), np.concatenate([_np(policy_states), _np(policy_actions)], axis=1))

    def compute_reward(self, states, actions):
        """GAIL.compute_reward (:62-73) -> float32 tensor [n]."""
        rows = np.concatenate([_np(states), _np(actions)], axis=1)
        return torch.from_numpy(self._e.gail_reward(rows[None], gp=self.gp)[0])

    def train(self, env_wrapper=None, expert_loader=None, num_episodes=None, model_path=None):
        """GAIL.train (:122-179) with `self.ppo` a freerl_amd.PPO2.PPO."""
        if self.ppo is None or not all(hasattr(self.ppo, m) for m in ("PPO_learn", "explore_env", "train_init", "value")):
            # (nothing, or something that is no PPO2-shaped policy: nothing of it is called)
            raise NotImplementedError("GAIL.train drives GAIL_file/PPO2.py, the policy side: pass one at construction, "
                                      "GAIL(config, ppo=PPO(config)) with freerl_amd.PPO2.PPO")
        ppo = self.ppo
        if ppo.config.get("discrete", False):
            raise ValueError("GAIL.train with a discrete policy is refused: the reference concatenates the long action index into the "
                             "discriminator's float input and its shipped discrete config has a_dim = 2 against one stored column")
        if isinstance(expert_loader, ExpertLoader) and self._expert is not expert_loader.dataset:
            self.load_expert(expert_loader.dataset)        # the loader's rows become the ring: trian_D_indices below
        ppo.train_init(env_wrapper, num_episodes, model_path)
        self.episode_num = ppo.episode_num
        self.d_history = []                                # trian_D's 4-tuple of every iteration
        while ppo.episode_num < ppo.max_episodes:
            batch = ppo.explore_env(env_wrapper)
            ppo.memory.clear()
            if batch is None:
                break
            policy_states, policy_actions = batch["states"], batch["actions"]
            expert_states, expert_actions = next(expert_loader)
            if isinstance(expert_loader, ExpertLoader) and self._expert is expert_loader.dataset:
                out = self.trian_D_indices(expert_loader.last_indices, policy_states, policy_actions)
            else:
                out = self.trian_D(expert_states, expert_actions, policy_states, policy_actions)
            d_loss, expert_prob, policy_prob, w_dis = out
            self.d_history.append(out)
            ppo.writer.add_scalar("Discriminator/Loss", d_loss, ppo.episode_num)
            ppo.writer.add_scalar("Discriminator/Expert", expert_prob, ppo.episode_num)
            ppo.writer.add_scalar("Discriminator/Policy", policy_prob, ppo.episode_num)
            if self.gp:
                ppo.writer.add_scalar("Discriminator/Wasserstein_Dis", w_dis, ppo.episode_num)
            batch["rewards"] = self.compute_reward(policy_states, policy_actions)
            last_value = ppo.value(torch.as_tensor(ppo.state, dtype=torch.float32).unsqueeze(0)).squeeze()
            ppo.PPO_learn(batch, last_value)
            ppo.eval_and_save(env_wrapper)
        return ppo.train_post(env_wrapper)


class ExpertLoader:
    """GAIL_utils.create_expert_loader's InfiniteDataLoader over InfiniteUniformSampler: `next(loader)` is a (states, actions) batch of
    `batch_size` rows drawn with replacement by torch.randint (`GAIL.next_expert_indices`' draw); `last_indices` names them.  Creating
    it takes one int64 draw from torch's generator, as a DataLoader iterator does for its base seed; batches are drawn when asked for
    (a DataLoader with num_workers = 0; worker processes would draw ahead)."""

    def __init__(self, dataset, batch_size):
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.last_indices = None
        torch.empty((), dtype=torch.int64).random_()

    def __iter__(self):
        return self

    def __next__(self):
        self.last_indices = torch.randint(high=len(self.dataset), size=(self.batch_size,), dtype=torch.int64).numpy()
        return self.dataset[self.last_indices]


def create_expert_loader(dataset, config):
    """GAIL_utils.create_expert_loader: batches of config['PPO']['horizon'] rows (+ 1 for algo 'MAIL')."""
    return ExpertLoader(dataset, config["PPO"]["horizon"] + 1 if config.get("algo") == "MAIL" else config["PPO"]["horizon"])
