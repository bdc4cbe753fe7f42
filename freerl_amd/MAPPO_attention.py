"""`MAPPO` of MAPPO_file/MAPPO_attention.py (:245-430), backed by the HIP engine: MAPPO's actors and joint ring, but every agent's critic
is an `Attention_Critic` (attention.py:135-205) over ONE `Attention` block that all critics share, updated by `frl_mappo_att_learn`
(kernels_mappo_att.hip): the agents are the outer loop of `learn`, so critic i+1 starts from the block as critic i's last step left it.

    MAPPO(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None, improment=None)

`improment` is the reference's spelling; None means {'attention': True}, the script's default.  With improment['attention'] false the
object is the plain joint-critic MAPPO engine with this file's two Adams per agent behind clip_grad_norm_(..., 0.5).  Each agent's
`critic_optimizer` covers the critic's own 6 tensors and the block's 6, so the block has one set of Adam moments and one step count
per agent.  `agents[id].critic(obs.values())` runs on the GPU and `state_dict()` carries the reference's 12 keys.
Refused with ValueError, as the reference raises: fewer than 2 agents (`torch.cat` of no others), unequal observation widths (every
e_j goes through agent i's own encoder_fc_s), hidden other than 128.  At most 8 agents (FRL_MAX_AGENTS).  Reference defect not kept
(DESIGN.md "MAPPO_attention"): `Attention_Critic.id_num` is a class-level counter, so a second `MAPPO(...)` in one process indexes
past `dim_info`; here a critic's index is its agent's.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _native as N
from ._core import DeviceNet, F32, init_layers, linear_init, split_layers
from .IPPO import IPPO
from .MAPPO import MAPPO as _JointMAPPO, MultiAgentPPO, RELU_GAIN

H = 128                                      # Attention(in_dim=128, hidden_dim=128, num_heads=4), attention_dim = hidden_1 = 128
OWN = [("encoder_fc_s", H, None), ("l1", H, 2 * H), ("l3", 1, H)]      # (None: the agent's observation width)
ATT_KEYS = ["attention.query.weight", "attention.key.weight", "attention.value.0.weight", "attention.value.0.bias",
            "attention.fc_out.weight", "attention.fc_out.bias"]


def _own_size(obs_dim):
    return H * obs_dim + H + H * 2 * H + H + H + 1


def pack_attention(sd):
    """the block's 6 tensors -> the engine's three layers: query (zero bias), [key ; value.0] (zero bias over the key), fc_out"""
    g = lambda k: np.asarray(torch.as_tensor(sd[k]).detach().cpu().numpy(), dtype=F32)
    z = np.zeros(H, F32)
    return np.concatenate([g(ATT_KEYS[0]).reshape(-1), z, g(ATT_KEYS[1]).reshape(-1), g(ATT_KEYS[2]).reshape(-1), z, g(ATT_KEYS[3]),
                           g(ATT_KEYS[4]).reshape(-1), g(ATT_KEYS[5])])


def unpack_attention(flat):
    o, out = 0, OrderedDict()
    take = lambda n: flat[o:o + n]
    out[ATT_KEYS[0]] = take(H * H).reshape(H, H); o += H * H + H
    kv = take(2 * H * H).reshape(2 * H, H); o += 2 * H * H
    out[ATT_KEYS[1]], out[ATT_KEYS[2]] = kv[:H], kv[H:]
    out[ATT_KEYS[3]] = flat[o + H:o + 2 * H]; o += 2 * H
    out[ATT_KEYS[4]] = take(H * H).reshape(H, H); o += H * H
    out[ATT_KEYS[5]] = take(H)
    return out


class AttentionCritic:
    """Stands where the reference has `agent.critic`: net 2j+1's own layers, and the shared block in net 1's copy"""

    def __init__(self, engine, j, obs_dim):
        self._e, self._net, self._own = engine, 2 * j + 1, _own_size(obs_dim)
        self._layers = [(n, o, obs_dim if i is None else i) for n, o, i in OWN]

    def keys(self):
        return ATT_KEYS + [n + s for n, _, _ in self._layers for s in (".weight", ".bias")]

    def state_dict(self):
        sd = unpack_attention(self._e.get_params(1)[self._own:])
        sd.update(split_layers(self._layers, self._e.get_params(self._net)[:self._own]))
        return OrderedDict((k, torch.from_numpy(np.array(sd[k], dtype=F32, copy=True))) for k in self.keys())

    def load_state_dict(self, sd, strict=True):
        if strict and set(sd.keys()) != set(self.keys()):
            raise RuntimeError("Error(s) in loading state_dict: expected keys %s, got %s" % (self.keys(), list(sd.keys())))
        own = []
        for n, od, idim in self._layers:
            w, b = (np.asarray(torch.as_tensor(sd[n + s]).detach().cpu().numpy(), dtype=F32) for s in (".weight", ".bias"))
            if w.shape != (od, idim) or b.shape != (od,):
                raise RuntimeError("size mismatch for %s: %s vs %s" % (n, w.shape, (od, idim)))
            own += [w.reshape(-1), b.reshape(-1)]
        att = pack_attention(sd)
        self._e.set_params(self._net, np.concatenate(own + [att]))
        self._e.set_params(1, np.concatenate([self._e.get_params(1)[:self._own], att]))      # the block every critic reads

    def parameters(self):
        return iter(self.state_dict().values())

    def named_parameters(self):
        return iter(self.state_dict().items())

    def __call__(self, s, agents=None):
        """V_i of the joint observation: `s` is the reference's obs.values() (one [rows, obs_dim] per agent); `agents` is not needed"""
        x = np.concatenate([np.asarray(torch.as_tensor(t).detach().cpu().numpy(), dtype=F32) for t in s], axis=1)
        return torch.from_numpy(self._e.act(self._net, N.ACT_RAW, x[None] if self._e.P == 1 else x, out_dim=1)[0])

    def to(self, *a, **k):
        return self


class Agent:
    """Actor, then Attention_Critic (MAPPO_attention.py:208-224): torch's generator is consumed as their constructors do"""

    def __init__(self, engine, j, obs_dim, action_dim, is_continue, trick, attention):
        head = "mean_layer" if is_continue else "l3"
        al = [("l1", H, obs_dim), ("l2", H, H), (head, action_dim, H)]
        ortho = bool(trick["orthogonal_init"])
        fa = init_layers(al, orthogonal=[RELU_GAIN, RELU_GAIN, 0.01] if ortho else None)
        parts = [linear_init(o, obs_dim if i is None else i) for _, o, i in OWN]
        if ortho:                                # net_init on l1 and l3 only (attention.py:174-177): the encoder keeps its default draw
            for k in (1, 2):
                t = torch.empty(parts[k][0].shape)
                torch.nn.init.orthogonal_(t, gain=RELU_GAIN)
                parts[k] = (t.numpy().astype(F32), np.zeros_like(parts[k][1]))
        own = np.concatenate([x.reshape(-1) for wb in parts for x in wb])
        engine.set_params(2 * j, np.concatenate([fa, np.zeros(action_dim, F32)]) if is_continue else fa)
        engine.set_params(2 * j + 1, np.concatenate([own, attention]))
        self.actor = DeviceNet(engine, 2 * j, al, extra=("log_std", (1, action_dim)) if is_continue else None,
                               act_mode=N.ACT_TANHHEAD if is_continue else N.ACT_RAW)
        self.critic = AttentionCritic(engine, j, obs_dim)


class _PlainMAPPO(MultiAgentPPO):
    """improment['attention'] false: the joint-observation critic (MAPPO.py's) with this file's two Adams and gradient clip per agent"""
    _algo = N.ALGO_MAPPO
    _file = "MAPPO.pth"
    _critic_in = _JointMAPPO._critic_in
    _optimizers = IPPO._optimizers
    learn = IPPO.learn
    lr_decay = IPPO.lr_decay


class MAPPO(MultiAgentPPO):
    _algo = N.ALGO_MAPPO_ATT
    _file = "MAPPO.pth"
    _optimizers = IPPO._optimizers               # two Adams per agent (MAPPO_attention.py:219-224)
    lr_decay = IPPO.lr_decay                     # :406-413

    def __new__(cls, dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None, improment=None, **kw):
        if improment is not None and not improment["attention"]:
            return _PlainMAPPO(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick, **kw)
        return super().__new__(cls)

    def __init__(self, dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick=None, improment=None, *, hidden=H, **kw):
        widths = [int(v[0]) for v in dim_info.values()]
        if len(widths) < 2:
            raise ValueError("MAPPO_attention needs at least 2 agents: the attention runs over the other agents' encodings")
        if len(set(widths)) != 1:
            raise ValueError("MAPPO_attention: observation widths %s differ; every agent's observation goes through agent i's own encoder" % widths)
        if hidden != H:
            raise ValueError("MAPPO_attention: hidden %d is refused (the attention block is built 128 wide)" % hidden)
        # Attention() is built once, before the agents (MAPPO_attention.py:250-254): query and key without bias, value.0, fc_out
        q, k = (torch.nn.Linear(H, H, bias=False).weight.detach() for _ in range(2))
        v, o = torch.nn.Linear(H, H), torch.nn.Linear(H, H)
        self._att0 = pack_attention(dict(zip(ATT_KEYS, [q, k, v.weight, v.bias, o.weight, o.bias])))
        super().__init__(dim_info, is_continue, actor_lr, critic_lr, horizon, device, trick, hidden=H, **kw)

    def _agent(self, j, hidden):
        return Agent(self._e, j, self._od[j], self._ad[j], self.is_continue, self.trick, self._att0)

    def learn(self, minibatch_size, gamma, lmbda, clip_param, K_epochs, entropy_coefficient, huber_delta=None):
        perms = None
        if self._rng != "device":                # one np.random.permutation per (agent, epoch), agent-major (:354-358)
            perms = np.stack([np.stack([np.random.permutation(self.horizon) for _ in range(K_epochs)]) for _ in self.agent_ids])[None]
        a0 = self.agents[self.agent_ids[0]]
        track = getattr(self, "track_loss", False)
        out = self._e.mappo_att_learn(self.horizon, minibatch_size, K_epochs, gamma=gamma, lmbda=lmbda, clip=clip_param,
                                      ent_coef=entropy_coefficient, adv_norm=self.trick["adv_norm"], value_clip=self.trick["ValueClip"],
                                      huber_delta=huber_delta if self.trick["huber_loss"] else None, perms=perms, want_trace=track,
                                      want_norms=track, actor_lr=a0.actor_optimizer.lr, critic_lr=a0.critic_optimizer.lr,
                                      adam_eps=a0.actor_optimizer.param_groups[0]["eps"], clip_norm=0.5)
        self.last_trace, self.last_norms = out.get("trace"), out.get("norms")
