"""`MADDPG` with the class surface of MADDPG_file/MADDPG_simple_with_tricks.py:120-224, backed by the HIP engine.  The script is
MADDPG_simple.py with one trick: `trick['ATT']` (its shipped default) gives every agent the attention critic of ATT-MADDPG
(`ATT_critic`, ATT.py:181-229) — an FRL_ALGO_MADDPG_ATT engine; `trick['ATT']` false builds the plain engine of
`freerl_amd.MADDPG.MADDPG`.  Everything but the critic — the joint ring, the per-agent index draws, `learn`'s launch order, the soft
updates — is the parent class's.

Two defects of the reference are not kept (DESIGN.md "ATT-MADDPG"): `ATT_critic.id_num` is a class-level counter, so a second
`MADDPG` in one process raises IndexError (here a critic's identity is its agent's index); `MADDPG.load` does not pass `trick` and
raises TypeError (here it works; the checkpoint holds actors only).  `ATT_critic_raw` and the `MLPNetworkWithAttention*` classes,
which nothing constructs, are not ported."""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, Engine, F32, OptimizerView, init_layers, resolve_device
from .Buffer import Buffer
from .MADDPG import MADDPG as _PlainMADDPG
from .TD3 import actor_layers

ATT_HEADS = 4            # ATT_critic(dim_info): head_count = 4


def att_critic_layers(obs_dims, act_dims, i, hidden):
    """[(name, out, in)] of ATT_critic in the reference's state_dict (and construction) order: the attention module's
    fc_encoder_input, fc_encoder_heads.0..3, fc_decoder_input, then encoder_input_fc, decoder_input_fc, fc1, fc2."""
    H, OT, AT = hidden, sum(obs_dims), sum(act_dims)
    return ([("attention_modules.fc_encoder_input", H, H)] + [("attention_modules.fc_encoder_heads.%d" % k, H, H) for k in range(ATT_HEADS)] +
            [("attention_modules.fc_decoder_input", H, H), ("encoder_input_fc", H, OT + act_dims[i]), ("decoder_input_fc", H, AT - act_dims[i]),
             ("fc1", H, H), ("fc2", 1, H)])


class AttCriticNet(DeviceNet):
    """`agent.critic` / `agent.critic_target` of an attention critic: the reference's ten nn.Linear as state_dict keys, stored by the
    engine as seven layers with the four heads stacked (weights [4 H, H], then biases [4 H]).  Called as the reference's module is,
    `critic(obs_list, act_list)` with every agent's tensors in agent order -> Q [rows, 1]."""

    def _perm(self):
        """-> index array: reference-order flat position of every engine-order flat element"""
        sizes = [(o * i, o) for _, o, i in self._layers]
        starts, p = [], 0
        for w, b in sizes:
            starts.append((p, p + w))
            p += w + b
        seg = lambda j, bias: np.arange(starts[j][1], starts[j][1] + sizes[j][1]) if bias else np.arange(starts[j][0], starts[j][1])
        heads = range(1, 1 + ATT_HEADS)
        order = [seg(0, False), seg(0, True)] + [seg(j, False) for j in heads] + [seg(j, True) for j in heads]
        for j in range(1 + ATT_HEADS, len(sizes)):
            order += [seg(j, False), seg(j, True)]
        return np.concatenate(order)

    def state_dict(self):
        eng = self._e.get_params(self._net, self._kind, self._learner)
        flat = np.empty_like(eng)
        flat[self._perm()] = eng
        parts = self._split(flat)
        return OrderedDict((k, torch.from_numpy(np.array(parts[k], dtype=F32, copy=True))) for k in self.keys())

    def load_state_dict(self, sd, strict=True):
        want = self.keys()
        if strict and set(sd.keys()) != set(want):
            raise RuntimeError("Error(s) in loading state_dict: expected keys %s, got %s" % (want, list(sd.keys())))
        flat = []
        for n, od, idim in self._layers:
            w = np.asarray(torch.as_tensor(sd[n + ".weight"]).detach().cpu().numpy(), dtype=F32)
            b = np.asarray(torch.as_tensor(sd[n + ".bias"]).detach().cpu().numpy(), dtype=F32)
            if w.shape != (od, idim) or b.shape != (od,):
                raise RuntimeError("size mismatch for %s: %s vs %s" % (n, w.shape, (od, idim)))
            flat += [w.reshape(-1), b.reshape(-1)]
        self._e.set_params(self._net, np.concatenate(flat)[self._perm()], self._kind, self._learner)

    def __call__(self, s, a):
        to_np = lambda ts: [np.asarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=F32) for t in ts]
        x = np.concatenate(to_np(list(s)) + to_np(list(a)), axis=1)
        y = self._e.act(self._net, N.ACT_RAW, x[None] if self._e.P == 1 else x, out_dim=1, use_target=(self._kind == N.PARAM_TARGET))
        return torch.from_numpy(y[0])


class Agent:
    """Agent (MADDPG_simple_with_tricks.py:91-104) with the attention critic; torch RNG order: Actor l1, l2, l3, then the critic's
    modules in state_dict order, all default nn.Linear init."""

    def __init__(self, engine, j, obs_dims, act_dims, actor_lr, critic_lr, hidden):
        al, cl = actor_layers(obs_dims[j], act_dims[j], hidden), att_critic_layers(obs_dims, act_dims, j, hidden)
        fa, fc = init_layers(al), init_layers(cl)
        self.actor = DeviceNet(engine, 2 * j, al, act_mode=N.ACT_TANHHEAD)
        self.critic = AttCriticNet(engine, 2 * j + 1, cl)
        self.actor_target = DeviceNet(engine, 2 * j, al, kind=N.PARAM_TARGET, act_mode=N.ACT_TANHHEAD)
        self.critic_target = AttCriticNet(engine, 2 * j + 1, cl, kind=N.PARAM_TARGET)
        fc_eng = fc[self.critic._perm()]
        for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
            engine.set_params(2 * j, fa, kind)
            engine.set_params(2 * j + 1, fc_eng, kind)
        self.actor_optimizer = OptimizerView(engine, 2 * j, actor_lr)
        self.critic_optimizer = OptimizerView(engine, 2 * j + 1, critic_lr)


class MADDPG(_PlainMADDPG):
    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick, *, rng="auto", hidden=128, batch_max=1024, seed=0):
        self.trick = trick
        if not trick["ATT"]:
            super().__init__(dim_info, is_continue, actor_lr, critic_lr, buffer_size, device, trick, rng=rng, hidden=hidden,
                             batch_max=batch_max, seed=seed)
            return
        if not is_continue:
            raise ValueError("only continuous actions are implemented in the reference (MADDPG_simple_with_tricks.py:139)")
        self.supplement, self._wd = None, 0.0
        self.agent_ids = list(dim_info.keys())
        od = [dim_info[a][0] for a in self.agent_ids]
        ad = [dim_info[a][1] for a in self.agent_ids]
        hip_id, self.device = resolve_device(device)
        self._e = Engine(N.ALGO_MADDPG_ATT, od, ad, max(int(buffer_size), 1), hidden=hidden, batch_max=batch_max, device_id=hip_id, seed=seed)
        self.agents, self.buffers = {}, {}
        for j, aid in enumerate(self.agent_ids):
            self.agents[aid] = Agent(self._e, j, od, ad, actor_lr, critic_lr, hidden)
            self.buffers[aid] = Buffer(buffer_size, od[j], ad[j], self.device, _engine=self._e, _agent=j)
        self.is_continue = is_continue
        self.agent_x = self.agent_ids[0]
        self.regular = False
        self._rng = rng
        self._ad = ad
        self._rec = np.zeros(self._e.width, dtype=F32)
        self.last_losses = None

    @staticmethod
    def load(dim_info, is_continue, model_dir, trick=None, **kw):
        """The reference's load() raises TypeError (it does not pass `trick`); this one works.  The checkpoint holds the actors only,
        so any `trick` loads it; None means the script's default {'ATT': True}."""
        policy = MADDPG(dim_info, is_continue=is_continue, actor_lr=0, critic_lr=0, buffer_size=0, device="cpu",
                        trick=trick if trick is not None else {"ATT": True}, **kw)
        data = torch.load(os.path.join(model_dir, "MADDPG.pth"))
        for agent_id, agent in policy.agents.items():
            agent.actor.load_state_dict(data[agent_id])
        return policy
