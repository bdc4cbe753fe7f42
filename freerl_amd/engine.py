"""Thin object wrapper over the C ABI (include/freerl_hip.h): one `Engine` = one `frl_engine`.

Host-side plumbing only (NumPy arrays in, NumPy arrays out); all compute runs in the HIP
library.  The reference-shaped classes (`freerl_amd.DQN`, `.TD3`, ... `.Buffer`) sit on top.
"""
import ctypes as C

import numpy as np

from . import _native as N

F32 = np.float32


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def make_config(algo, obs_dim, act_dim, capacity, *, n_learners=1, discrete=False, hidden=128,
                hidden_act=N.ACT_RELU, twin_critic=False, batch_max=256, extra_cols=0, device_id=0, seed=0, actor_dist=0, dueling=False, noisy=False, c51=None, reward_dim=0,
                state_dim=0, state_rows=N.STATE_ROWS_POSITION):
    """Engine's arguments as what frl_create / frl_create_ex take: (Config, ConfigExt or None).  Loads no library."""
    obs_dim = list(obs_dim) if isinstance(obs_dim, (list, tuple)) else [int(obs_dim)]
    act_dim = list(act_dim) if isinstance(act_dim, (list, tuple)) else [int(act_dim)]
    assert len(obs_dim) == len(act_dim)
    cfg = N.Config()
    cfg.algo, cfg.n_learners, cfg.n_agents = int(algo), int(n_learners), len(obs_dim)
    for j, (o, a) in enumerate(zip(obs_dim, act_dim)):
        cfg.obs_dim[j], cfg.act_dim[j] = int(o), int(a)
    cfg.discrete, cfg.hidden, cfg.hidden_act = int(bool(discrete)), int(hidden), int(hidden_act)
    cfg.twin_critic, cfg.capacity, cfg.batch_max = int(bool(twin_critic)), int(capacity), int(batch_max)
    cfg.extra_cols, cfg.device_id, cfg.seed = int(extra_cols), int(device_id), int(seed) & (2 ** 64 - 1)
    cfg.actor_dist, cfg.dueling, cfg.noisy = int(actor_dist), int(bool(dueling)), int(bool(noisy))
    cfg.reward_dim = int(reward_dim)          # envelope DQN / DDPG: objectives (0 = 1; ignored by the other algorithms)
    if c51 is not None:                     # (atoms, v_min, v_max)
        cfg.c51_atoms, cfg.c51_vmin, cfg.c51_vmax = int(c51[0]), float(c51[1]), float(c51[2])
    if state_rows and not state_dim:
        raise ValueError("state_rows %r without a state_dim: there is no state block to pair" % (state_rows,))
    # a global-state critic (FRL_ALGO_MAPPO): frl_config cannot grow, the extension block can
    return cfg, (N.ConfigExt(C.sizeof(N.ConfigExt), int(state_dim), int(state_rows)) if state_dim else None)


class Engine:
    def __init__(self, algo, obs_dim, act_dim, capacity, *, n_learners=1, discrete=False, hidden=128,
                 hidden_act=N.ACT_RELU, twin_critic=False, batch_max=256, extra_cols=0, device_id=0, seed=0, actor_dist=0, dueling=False, noisy=False, c51=None, reward_dim=0,
                 state_dim=0, state_rows=N.STATE_ROWS_POSITION):
        cfg, ext = make_config(algo, obs_dim, act_dim, capacity, n_learners=n_learners, discrete=discrete, hidden=hidden, hidden_act=hidden_act,
                               twin_critic=twin_critic, batch_max=batch_max, extra_cols=extra_cols, device_id=device_id, seed=seed, actor_dist=actor_dist,
                               dueling=dueling, noisy=noisy, c51=c51, reward_dim=reward_dim, state_dim=state_dim, state_rows=state_rows)
        self._L = N.lib()
        h = C.c_void_p()
        if ext is not None:
            N.check(self._L.frl_create_ex(C.byref(cfg), C.byref(ext), C.byref(h)))
        else:
            N.check(self._L.frl_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.cfg = cfg
        self.algo = int(algo)
        self.P = cfg.n_learners
        self.n_agents = cfg.n_agents
        self.capacity = cfg.capacity
        self.batch_max = cfg.batch_max
        lay = N.RecordLayout()
        N.check(self._L.frl_record_layout_get(self._h, C.byref(lay)))
        self.layout = lay
        self.width = lay.width
        self.act_max = max(lay.act_dim[j] for j in range(self.n_agents))
        # draw sets per (learner, updating agent) of learn()'s `noise` (include/freerl_hip.h: frl_learn_args.noise)
        self.noise_sets = 2 * self.n_agents + 1 if self.algo == N.ALGO_MASAC else max(2, self.n_agents)
        self.reward_dim = lay.done_off - lay.rew_off if self.n_agents == 1 else 1      # (envelope DQN / DDPG: the reward vector's columns)
        n = C.c_int(0)
        N.check(self._L.frl_net_count(self._h, C.byref(n)))
        self.n_nets = n.value
        self._nparams = {}

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.frl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        N.check(self._L.frl_sync(self._h))

    def lds_bytes(self):
        b, r = C.c_int(0), C.c_int(0)
        N.check(self._L.frl_lds_bytes(self._h, C.byref(b), C.byref(r)))
        return b.value, r.value

    def state_info(self):
        """(state_dim, record column of the state block) of a global-state MAPPO engine (frl_state_info); (0, 0) without one."""
        d, c = C.c_int(0), C.c_int(0)
        N.check(self._L.frl_state_info(self._h, C.byref(d), C.byref(c)))
        return d.value, c.value

    def learn_path(self, batch):
        """(chained, lds_bytes, rows_per_workgroup) of the kernel family learn() launches at this batch size."""
        c, b, r = C.c_int(0), C.c_int(0), C.c_int(0)
        N.check(self._L.frl_learn_path(self._h, int(batch), C.byref(c), C.byref(b), C.byref(r)))
        return bool(c.value), b.value, r.value

    def actor_park(self):
        """Does the actor stage this engine launches read pass A's h2 back from the park buffer (frl_actor_park)?"""
        v = C.c_int(0)
        N.check(self._L.frl_actor_park(self._h, C.byref(v)))
        return bool(v.value)

    # ------------------------------------------------------------------ replay
    def add(self, learner, record):
        rec = np.ascontiguousarray(record, dtype=F32)
        assert rec.size == self.width, (rec.size, self.width)
        N.check(self._L.frl_buffer_add(self._h, int(learner), _fp(rec)))

    def add_batch(self, records, learners=None):
        recs = np.ascontiguousarray(records, dtype=F32).reshape(-1, self.width)
        lp = None
        if learners is not None:
            ln = np.ascontiguousarray(learners, dtype=np.int32)
            assert ln.size == recs.shape[0]
            lp = ln.ctypes.data_as(C.POINTER(C.c_int))
        N.check(self._L.frl_buffer_add_batch(self._h, recs.shape[0], lp, _fp(recs)))

    def flush(self):
        N.check(self._L.frl_buffer_flush(self._h))

    def cursor(self, learner=0):
        i, s = C.c_int(0), C.c_int(0)
        N.check(self._L.frl_buffer_cursor_get(self._h, int(learner), C.byref(i), C.byref(s)))
        return i.value, s.value

    def set_cursor(self, learner, index, size):
        N.check(self._L.frl_buffer_cursor_set(self._h, int(learner), int(index), int(size)))

    def sample_into(self, learner, idx, fields, out_ptrs):
        """fields: [(col0, ncols)], out_ptrs: device addresses of dense [B][ncols] fp32 tensors."""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        nf = len(fields)
        col0 = (C.c_int * nf)(*[f[0] for f in fields])
        ncols = (C.c_int * nf)(*[f[1] for f in fields])
        outs = (C.c_void_p * nf)(*out_ptrs)
        N.check(self._L.frl_buffer_sample(self._h, int(learner), idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                          idx.size, nf, col0, ncols, outs))

    def read_rows(self, learner, row0, n):
        out = np.empty((n, self.width), dtype=F32)
        if n:
            N.check(self._L.frl_buffer_read(self._h, int(learner), int(row0), int(n), _fp(out)))
        return out

    def fill_synthetic(self, rows, seed=0):
        N.check(self._L.frl_buffer_fill_synthetic(self._h, int(rows), int(seed)))

    def her_relabel(self, learners, lengths, *, state_dim, goal_dim, sample_num=4, sample_range=200, mode=N.HER_SPARSE, weights=None,
                    tolerance=0.5, env_actions=None, picks=None):
        """Hindsight relabelling of the finished episodes of `learners` (frl_her_relabel): learner learners[e]'s episode is the
        lengths[e] rows behind its cursor.  `env_actions` [sum L][A] replaces the action columns of the relabelled rows (None: the
        stored action), `picks` int32 [sum rows] injects the offset j - i of every row (None: drawn on the device), `weights`
        [goal_dim] float64 (None: the script's 1, 1, 0.1).  -> the rows written per episode, int32 [n]."""
        ln = np.ascontiguousarray(np.asarray(learners, dtype=np.int32).reshape(-1))
        ls = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32).reshape(-1))
        assert ln.size == ls.size, (ln.size, ls.size)
        a = N.HerArgs()
        a.n_episodes = ln.size
        a.learners, a.lengths = ln.ctypes.data_as(C.POINTER(C.c_int)), ls.ctypes.data_as(C.POINTER(C.c_int))
        a.state_dim, a.goal_dim, a.sample_num, a.sample_range = int(state_dim), int(goal_dim), int(sample_num), int(sample_range)
        a.mode, a.tolerance = int(mode), float(tolerance)
        keep = []
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            assert w.size == int(goal_dim), (w.size, goal_dim)
            a.weights = w.ctypes.data_as(C.POINTER(C.c_double))
            keep.append(w)
        if env_actions is not None:
            ea = np.ascontiguousarray(env_actions, dtype=F32).reshape(-1)
            assert ea.size == int(ls.sum()) * self.layout.act_dim[0], (ea.size, int(ls.sum()), self.layout.act_dim[0])
            a.env_actions = _fp(ea)
            keep.append(ea)
        if picks is not None:
            pk = np.ascontiguousarray(picks, dtype=np.int32).reshape(-1)
            q = min(int(sample_num), int(sample_range))
            want = sum(sum(min(q, int(L) - i) for i in range(max(int(L) - q, 0), int(L))) + max(int(L) - q, 0) * q for L in ls) if q >= 1 else 0
            assert pk.size == want, (pk.size, want)
            a.picks = pk.ctypes.data_as(C.POINTER(C.c_int32))
            keep.append(pk)
        rows = np.zeros(ln.size, dtype=np.int32)
        a.rows_out = rows.ctypes.data_as(C.POINTER(C.c_int))
        N.check(self._L.frl_her_relabel(self._h, C.byref(a)))
        return rows

    # ------------------------------------------------------------------ parameters
    def num_params(self, net):
        if net not in self._nparams:
            n = C.c_int(0)
            N.check(self._L.frl_net_num_params(self._h, int(net), C.byref(n)))
            self._nparams[net] = n.value
        return self._nparams[net]

    def get_params(self, net, kind=N.PARAM_ONLINE, learner=0):
        out = np.empty(self.num_params(net), dtype=F32)
        N.check(self._L.frl_params_get(self._h, int(learner), int(net), int(kind), _fp(out)))
        return out

    def set_params(self, net, flat, kind=N.PARAM_ONLINE, learner=0):
        flat = np.ascontiguousarray(flat, dtype=F32).reshape(-1)
        assert flat.size == self.num_params(net), (flat.size, self.num_params(net))
        N.check(self._L.frl_params_set(self._h, int(learner), int(net), int(kind), _fp(flat)))

    def pad_max(self, net, kind=N.PARAM_ONLINE, learner=0):
        """max |x| over the padding slots of a net's block (must stay 0: frl_params_pad_max)."""
        v = C.c_float(0)
        N.check(self._L.frl_params_pad_max(self._h, int(learner), int(net), int(kind), C.byref(v)))
        return v.value

    def opt_step(self, net, learner=0):
        t = C.c_int(0)
        N.check(self._L.frl_opt_step_get(self._h, int(learner), int(net), C.byref(t)))
        return t.value

    def set_opt_step(self, net, t, learner=0):
        N.check(self._L.frl_opt_step_set(self._h, int(learner), int(net), int(t)))

    def alpha_state(self, learner=0):
        v = np.zeros(4, dtype=F32)
        t = C.c_int(0)
        N.check(self._L.frl_alpha_get(self._h, int(learner), _fp(v), C.byref(t)))
        return v, t.value

    def set_alpha_state(self, vals4, step=0, learner=0):
        v = np.ascontiguousarray(vals4, dtype=F32)
        N.check(self._L.frl_alpha_set(self._h, int(learner), _fp(v), int(step)))

    def alpha_state_agent(self, agent, learner=0):
        """({log_alpha, exp_avg, exp_avg_sq, alpha}, Adam step) of ONE agent's alpha (frl_alpha_get_agent: MASAC engines)."""
        v = np.zeros(4, dtype=F32)
        t = C.c_int(0)
        N.check(self._L.frl_alpha_get_agent(self._h, int(learner), int(agent), _fp(v), C.byref(t)))
        return v, t.value

    def set_alpha_state_agent(self, agent, vals4, step=0, learner=0):
        v = np.ascontiguousarray(vals4, dtype=F32)
        N.check(self._L.frl_alpha_set_agent(self._h, int(learner), int(agent), _fp(v), int(step)))

    # ------------------------------------------------------------------ forward
    def act(self, net, mode, obs, *, eps=None, head=0, use_target=False, out_dim=None, want_logp=False, normalize=True):
        """obs [P, n_rows, in_dim] (or [n_rows, in_dim] when P == 1) -> out [P, n_rows, out_dim]."""
        obs = np.ascontiguousarray(obs, dtype=F32)
        if obs.ndim == 2:
            obs = obs[None]
        P, n_rows, in_dim = obs.shape
        assert P == self.P
        od = 1 if mode in (N.ACT_ARGMAX, N.ACT_CAT_SAMPLE) else int(out_dim)
        out = np.empty((P, n_rows, od), dtype=F32)
        logp = np.empty((P, n_rows, od), dtype=F32) if want_logp else None
        ep = None
        if eps is not None:
            eps = np.ascontiguousarray(eps, dtype=F32).reshape(P, n_rows, -1)
            ep = _fp(eps)
        flags = int(mode) | (0 if normalize else N.ACT_NO_OBSNORM)
        N.check(self._L.frl_act(self._h, int(net), flags, int(head), int(use_target), n_rows, in_dim,      # 2: noisy effective set 0
                                _fp(obs), ep, _fp(out), _fp(logp) if want_logp else None))
        return (out, logp) if want_logp else out

    # ------------------------------------------------------------------ learn
    def act_explore(self, mode, obs, *, kind, epsilon=0.0, sigma=0.0, scale=1.0, max_action=1.0, ou_theta=0.15, ou_sigma=0.2,
                    ou_dt=1e-2, ended=None, out_dim=None):
        """select_action + the reference loop's exploration rule in one launch (frl_act_explore): obs [P, rows, obs_dim] ->
        (stored action, env-unit action), each [P, rows, out_dim] ([P, rows] for ACT_ARGMAX).  Draws come from the engine's
        Philox stream; `ended` [P, rows] resets those rows' OU state first."""
        obs = np.ascontiguousarray(obs, dtype=F32)
        assert obs.ndim == 3 and obs.shape[0] == self.P
        rows = obs.shape[1]
        x = N.ExploreArgs()
        x.kind, x.epsilon, x.sigma, x.scale, x.max_action = int(kind), epsilon, sigma, scale, max_action
        x.ou_theta, x.ou_sigma, x.ou_dt = ou_theta, ou_sigma, ou_dt
        disc = mode == N.ACT_ARGMAX
        shape = (self.P, rows) if disc else (self.P, rows, int(out_dim if out_dim is not None else self.act_max))
        store, env = np.empty(shape, F32), np.empty(shape, F32)
        ep = None
        if ended is not None:
            en = np.ascontiguousarray(ended, dtype=np.uint8).reshape(self.P, rows)
            ep = en.ctypes.data_as(C.POINTER(C.c_uint8))
        N.check(self._L.frl_act_explore(self._h, int(mode), rows, _fp(obs), C.byref(x), ep, _fp(store), _fp(env)))
        return store, env

    def learn(self, batch, *, gamma, tau, actor_lr=0.0, critic_lr=0.0, alpha_lr=1e-4, adam_eps=1e-8,
              critic_weight_decay=0.0, clip_norm=0.5, do_actor=True, use_policy_noise=False, policy_noise=0.0,
              noise_clip=0.0, max_action=1.0, policy_noise_scale=1.0, target_entropy=0.0, double_dqn=False, per=False,
              noisy_eps=None, idx=None, noise=None,
              want_stats=False, huber_delta=None):
        a = N.LearnArgs()
        a.batch, a.do_actor, a.use_policy_noise = int(batch), int(bool(do_actor)), int(bool(use_policy_noise))
        a.double_dqn, a.per = int(bool(double_dqn)), int(per)
        a.gamma, a.tau = gamma, tau
        a.actor_lr, a.critic_lr, a.alpha_lr, a.adam_eps = actor_lr, critic_lr, alpha_lr, adam_eps
        a.critic_weight_decay, a.clip_norm = critic_weight_decay, clip_norm
        a.policy_noise, a.noise_clip, a.max_action, a.policy_noise_scale = policy_noise, noise_clip, max_action, policy_noise_scale
        a.target_entropy = target_entropy
        if huber_delta is not None:             # TD loss = huber_loss(e, delta).mean() instead of F.mse_loss
            a.loss_kind, a.huber_delta = 1, float(huber_delta)
        keep = []
        if noisy_eps is not None:
            ne = np.ascontiguousarray(noisy_eps, dtype=F32).reshape(self.P, -1)
            keep.append(ne)
            a.noisy_eps = _fp(ne)
        if idx is not None:
            ix = np.ascontiguousarray(idx, dtype=np.int64).reshape(self.P, self.n_agents, int(batch))
            keep.append(ix)
            a.idx = ix.ctypes.data_as(C.POINTER(C.c_int64))
        if noise is not None:
            nz = np.ascontiguousarray(noise, dtype=F32).reshape(self.P, self.n_agents, self.noise_sets, int(batch), self.act_max)
            keep.append(nz)
            a.noise = _fp(nz)
        stats = None
        if want_stats:
            stats = np.zeros((self.P, self.n_agents, N.FRL_STAT_COUNT), dtype=F32)
            a.stats_out = _fp(stats)
        N.check(self._L.frl_learn(self._h, C.byref(a)))
        return stats

    def stats(self):
        out = np.zeros((self.P, self.n_agents, N.FRL_STAT_COUNT), dtype=F32)
        N.check(self._L.frl_stats_get(self._h, _fp(out)))
        return out

    def last_indices(self, batch):
        """int64 [P][n_agents][batch]: the ring rows the last learn() trained on."""
        out = np.zeros((self.P, self.n_agents, int(batch)), dtype=np.int64)
        N.check(self._L.frl_last_indices(self._h, int(batch), out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def learn_work(self, batch, do_actor=True):
        fl, by = C.c_double(0), C.c_double(0)
        N.check(self._L.frl_learn_work(self._h, int(batch), int(bool(do_actor)), C.byref(fl), C.byref(by)))
        return fl.value, by.value

    def learn_work_executed(self, batch, do_actor=True):
        """Flops the launch executes (no first-layer dX of trained nets, action columns only for dQ/da): frl_learn_work_executed."""
        fl = C.c_double(0)
        N.check(self._L.frl_learn_work_executed(self._h, int(batch), int(bool(do_actor)), C.byref(fl)))
        return fl.value

    # ------------------------------------------------------------------ noisy head
    def noisy_eps_size(self):
        n = C.c_int(0)
        N.check(self._L.frl_noisy_eps_size(self._h, C.byref(n)))
        return n.value

    def noisy_resample(self, eps=None):
        if eps is None:
            N.check(self._L.frl_noisy_resample(self._h, None))
        else:
            ne = np.ascontiguousarray(eps, dtype=F32).reshape(self.P, -1)
            N.check(self._L.frl_noisy_resample(self._h, _fp(ne)))

    # ------------------------------------------------------------------ prioritised replay
    def per_enable(self, alpha=0.5, beta=0.4, beta_increment=0.001, epsilon=0.01):
        N.check(self._L.frl_per_enable(self._h, alpha, beta, beta_increment, epsilon))

    def per_sample(self, batch, uniforms=None, want_outputs=True):
        """-> (idx int64 [P][batch], is_weight f32 [P][batch]); the rows become the current sample for learn(per=True).
        want_outputs=False: nothing is read back and the call is asynchronous (returns None)."""
        up = None
        if uniforms is not None:
            u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(self.P, int(batch))
            up = u.ctypes.data_as(C.POINTER(C.c_double))
        if not want_outputs:
            N.check(self._L.frl_per_sample(self._h, int(batch), up, None, None))
            return None
        idx = np.zeros((self.P, int(batch)), np.int64)
        w = np.zeros((self.P, int(batch)), F32)
        N.check(self._L.frl_per_sample(self._h, int(batch), up, idx.ctypes.data_as(C.POINTER(C.c_int64)), _fp(w)))
        return idx, w

    def per_update(self, batch, idx=None, td_error=None):
        ip = tp = None
        if idx is not None:
            ix = np.ascontiguousarray(idx, dtype=np.int64).reshape(self.P, int(batch))
            ip = ix.ctypes.data_as(C.POINTER(C.c_int64))
        if td_error is not None:
            td = np.ascontiguousarray(td_error, dtype=F32).reshape(self.P, int(batch))
            tp = _fp(td)
        N.check(self._L.frl_per_update(self._h, int(batch), ip, tp))

    def per_state(self, learner=0):
        s, m, b = C.c_double(0), C.c_double(0), C.c_double(0)
        N.check(self._L.frl_per_state(self._h, int(learner), C.byref(s), C.byref(m), C.byref(b)))
        return dict(sum=s.value, max=m.value, beta=b.value)

    def ppo_learn(self, horizon, minibatch, k_epochs, *, gamma, lmbda, clip, ent_coef, actor_lr, critic_lr,
                  adam_eps=1e-8, clip_norm=0.5, adv_norm=False, perms=None, want_trace=False, want_adv=False,
                  optimizer=0, last_value=None):
        """last_value (one float per learner): PPO_advance/PPO_2.py's learn — advantages and returns from the values the
        ring stored at rollout time (extra column before adv_done), no value pass."""
        a = N.PpoArgs()
        a.horizon, a.minibatch, a.k_epochs, a.adv_norm = int(horizon), int(minibatch), int(k_epochs), int(bool(adv_norm))
        a.gamma, a.lmbda, a.clip, a.ent_coef = gamma, lmbda, clip, ent_coef
        a.actor_lr, a.critic_lr, a.adam_eps, a.clip_norm = actor_lr, critic_lr, adam_eps, clip_norm
        a.optimizer = int(optimizer)
        keep = []
        if perms is not None:
            pm = np.ascontiguousarray(perms, dtype=np.int64).reshape(self.P, int(k_epochs), int(horizon))
            keep.append(pm)
            a.perms = pm.ctypes.data_as(C.POINTER(C.c_int64))
        if last_value is not None:
            lv = np.ascontiguousarray(np.broadcast_to(np.asarray(last_value, dtype=F32).reshape(-1), (self.P,)))
            keep.append(lv)
            a.gae_mode, a.last_value, a.gae_gamma, a.gae_lmbda = 1, _fp(lv), float(gamma), float(lmbda)
        n_mb = (int(horizon) + int(minibatch) - 1) // int(minibatch)
        out = {}
        if want_trace:
            out["trace"] = np.zeros((self.P, int(k_epochs) * n_mb, 2), dtype=F32)
            a.loss_trace_out = _fp(out["trace"])
        if want_adv:
            out["adv"] = np.zeros((self.P, int(horizon)), dtype=F32)
            out["v_target"] = np.zeros((self.P, int(horizon)), dtype=F32)
            a.adv_out, a.vtarget_out = _fp(out["adv"]), _fp(out["v_target"])
        N.check(self._L.frl_ppo_learn(self._h, C.byref(a)))
        return out

    def gail_ppo_learn(self, horizon, minibatch, k_epochs, *, gamma, lam, clip, ent_weight, value_loss_coef, p_lr, v_lr, clip_norm=0.5,
                       last_value=None, rewards=None, perms=None, want=()):
        """GAIL_file/PPO2.py's PPO_learn on a GAIL_PPO engine (frl_gail_ppo_learn).  last_value [P], rewards [P, horizon] (in place of the
        ring's reward column), perms [P, k_epochs, horizon] (torch.randperm draws; None: drawn on the device).  want: any of "adv" (before
        normalisation), "returns", "logp_old", "trace" -> the dict's arrays."""
        T, K = int(horizon), int(k_epochs)
        a = N.GailPpoArgs()
        a.horizon, a.minibatch, a.k_epochs = T, int(minibatch), K
        a.gamma, a.lam, a.clip, a.ent_weight, a.value_loss_coef = gamma, lam, clip, ent_weight, value_loss_coef
        a.p_lr, a.v_lr, a.clip_norm = p_lr, v_lr, clip_norm
        keep = []
        if last_value is not None:
            lv = np.ascontiguousarray(np.broadcast_to(np.asarray(last_value, dtype=F32).reshape(-1), (self.P,)))
            keep.append(lv)
            a.last_value = _fp(lv)
        if rewards is not None:
            rw = np.ascontiguousarray(rewards, dtype=F32).reshape(self.P, T)
            keep.append(rw)
            a.rewards = _fp(rw)
        if perms is not None:
            pm = np.ascontiguousarray(perms, dtype=np.int64).reshape(self.P, K, T)
            keep.append(pm)
            a.perms = pm.ctypes.data_as(C.POINTER(C.c_int64))
        n_mb = (T + int(minibatch) - 1) // max(int(minibatch), 1)
        out = {}
        for name, field, shape in (("adv", "adv_out", (self.P, T)), ("returns", "returns_out", (self.P, T)),
                                   ("logp_old", "logp_old_out", (self.P, T)), ("trace", "loss_trace_out", (self.P, max(K, 0) * n_mb, 2))):
            if name in want:
                out[name] = np.zeros(shape, dtype=F32)
                setattr(a, field, _fp(out[name]))
        N.check(self._L.frl_gail_ppo_learn(self._h, C.byref(a)))
        return out

    def set_log_std_range(self, lo, hi):
        """The actor's log_std clamp range of a GAIL_PPO engine (frl_log_std_range_set)."""
        N.check(self._L.frl_log_std_range_set(self._h, float(lo), float(hi)))

    def log_std_range(self):
        lo, hi = C.c_float(0), C.c_float(0)
        N.check(self._L.frl_log_std_range_get(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def reinforce_learn(self, *, gamma, lr, n_steps=None, adam_eps=1e-8, want_loss=False, want_returns=False):
        """REINFORCE.learn(gamma) for every learner (frl_reinforce_learn): learner p trains on ring rows 0..n_steps[p]-1
        (None: its cursor size; 0: it sits the call out).  -> dict with `loss` [P] and / or `returns` [P][capacity]
        (normalised returns; rows past a learner's length, and learners that sat out, are NaN); empty and asynchronous when
        neither is asked for."""
        a = N.ReinforceArgs()
        a.gamma, a.lr, a.adam_eps = float(gamma), float(lr), float(adam_eps)
        if n_steps is not None:
            ns = np.ascontiguousarray(np.broadcast_to(np.asarray(n_steps, dtype=np.int32).reshape(-1), (self.P,)))
            a.n_steps = ns.ctypes.data_as(C.POINTER(C.c_int))
        out = {}
        if want_loss:
            out["loss"] = np.full(self.P, np.nan, dtype=F32)
            a.loss_out = _fp(out["loss"])
        if want_returns:
            out["returns"] = np.full((self.P, self.capacity), np.nan, dtype=F32)
            a.returns_out = _fp(out["returns"])
        N.check(self._L.frl_reinforce_learn(self._h, C.byref(a)))
        return out

    def _envelope_call(self, fn, a, batch, weight_num, idx, weights, want_weights, out):
        """What envelope_learn and envelope_ddpg_learn share: batch / weight_num / idx / weights into `a`, the `weights` output, the call."""
        a.batch, a.weight_num = int(batch), int(weight_num)
        keep = []
        if idx is not None:
            ix = np.ascontiguousarray(idx, dtype=np.int64).reshape(self.P, int(batch))
            keep.append(ix)
            a.idx = ix.ctypes.data_as(C.POINTER(C.c_int64))
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=F32).reshape(self.P, int(weight_num), self.reward_dim)
            keep.append(w)
            a.weights = _fp(w)
        if want_weights:
            out["weights"] = np.full((self.P, max(int(weight_num), 0), self.reward_dim), np.nan, dtype=F32)
            a.weights_out = _fp(out["weights"])
        N.check(fn(self._h, C.byref(a)))
        return out

    def envelope_learn(self, batch, weight_num, *, gamma, tau, lr, beta, idx=None, weights=None, want_loss=False, want_weights=False):
        """ENVELOPE.learn for every learner (frl_envelope_learn) on batch x weight_num rows: row j is ring row idx[j % batch] under
        preference weights[j // batch].  idx [P][batch] / weights [P][weight_num][reward_dim], or None: drawn on the device.
        -> dict with `loss` [P] and / or `weights` [P][weight_num][reward_dim] (the preferences used); empty and asynchronous
        when neither is asked for."""
        a = N.EnvelopeArgs()
        a.gamma, a.tau, a.lr, a.beta = float(gamma), float(tau), float(lr), float(beta)
        out = {}
        if want_loss:
            out["loss"] = np.full(self.P, np.nan, dtype=F32)
            a.loss_out = _fp(out["loss"])
        return self._envelope_call(self._L.frl_envelope_learn, a, batch, weight_num, idx, weights, want_weights, out)

    def envelope_ddpg_learn(self, batch, weight_num, *, gamma, tau, actor_lr, critic_lr, beta, idx=None, weights=None, want_loss=False,
                            want_weights=False):
        """ENVELOPE_DDPG.learn for every learner (frl_envelope_ddpg_learn) on batch x weight_num rows: row j is ring row idx[j % batch]
        under preference weights[j // batch]; the critic step, then the actor step through the updated critic, both clipped at 0.5,
        then both soft updates.  idx [P][batch] / weights [P][weight_num][reward_dim], or None: drawn on the device.
        -> dict with `critic_loss` [P] and `actor_loss` [P] and / or `weights` [P][weight_num][reward_dim] (the preferences used);
        empty and asynchronous when neither is asked for."""
        a = N.EnvelopeDdpgArgs()
        a.gamma, a.tau, a.actor_lr, a.critic_lr, a.beta = float(gamma), float(tau), float(actor_lr), float(critic_lr), float(beta)
        out = {}
        if want_loss:
            out["critic_loss"] = np.full(self.P, np.nan, dtype=F32)
            out["actor_loss"] = np.full(self.P, np.nan, dtype=F32)
            a.critic_loss_out, a.actor_loss_out = _fp(out["critic_loss"]), _fp(out["actor_loss"])
        return self._envelope_call(self._L.frl_envelope_ddpg_learn, a, batch, weight_num, idx, weights, want_weights, out)

    # ------------------------------------------------------------------ CEM_GD3PG: two rings per learner, one learn entry point
    def ring_add(self, ring, record, learner=0):
        rec = np.ascontiguousarray(record, dtype=F32)
        assert rec.size == self.width, (rec.size, self.width)
        N.check(self._L.frl_ring_add(self._h, int(learner), int(ring), _fp(rec)))

    def ring_add_batch(self, ring, records, learners=None):
        recs = np.ascontiguousarray(records, dtype=F32).reshape(-1, self.width)
        lp = None
        if learners is not None:
            ln = np.ascontiguousarray(learners, dtype=np.int32)
            assert ln.size == recs.shape[0]
            lp = ln.ctypes.data_as(C.POINTER(C.c_int))
        N.check(self._L.frl_ring_add_batch(self._h, int(ring), recs.shape[0], lp, _fp(recs)))

    def ring_cursor(self, ring, learner=0):
        i, s = C.c_int(0), C.c_int(0)
        N.check(self._L.frl_ring_cursor_get(self._h, int(learner), int(ring), C.byref(i), C.byref(s)))
        return i.value, s.value

    def set_ring_cursor(self, ring, index, size, learner=0):
        N.check(self._L.frl_ring_cursor_set(self._h, int(learner), int(ring), int(index), int(size)))

    def ring_rows(self, ring, row0, n, learner=0):
        """Rows [row0, row0 + n) of ring `ring` (a learner's rings lie side by side: frl_buffer_read's rows [ring capacity, ..))."""
        return self.read_rows(learner, int(ring) * self.capacity + int(row0), n)

    def cem_gd3pg_learn(self, batch, *, gamma, tau, actor_lr, critic_lr, f1_more, delta, lam=10.0, idx=None, want_out=True):
        """CEM_GD3PG.learn for every learner (frl_cem_gd3pg_learn) on 2 x half rows, half = min(len(ring 1), batch) // 2: f1_more and delta
        one per learner (scalars broadcast), idx [P][2][half] ring-relative rows (ring 0's first) or None: drawn on the device.
        -> float32 [P][8] in the order of _native.CEM_OUT, or None (asynchronous) when want_out is false."""
        a = N.CemGd3pgArgs()
        a.batch, a.gamma, a.tau, a.actor_lr, a.critic_lr = int(batch), float(gamma), float(tau), float(actor_lr), float(critic_lr)
        setattr(a, "lambda", float(lam))
        f1 = np.ascontiguousarray(np.broadcast_to(np.asarray(f1_more).astype(np.int32).reshape(-1), (self.P,)))
        dl = np.ascontiguousarray(np.broadcast_to(np.asarray(delta, dtype=F32).reshape(-1), (self.P,)))
        a.f1_more, a.delta = f1.ctypes.data_as(C.POINTER(C.c_int)), _fp(dl)
        keep = [f1, dl]
        if idx is not None:
            ix = np.ascontiguousarray(idx, dtype=np.int64).reshape(self.P, 2, -1)
            half = min(min(self.ring_cursor(1, p)[1] for p in range(self.P)), int(batch)) // 2      # what the library will read
            if ix.shape[2] != half:
                raise ValueError("idx holds %d rows per ring, the call uses %d" % (ix.shape[2], half))
            keep.append(ix)
            a.idx = ix.ctypes.data_as(C.POINTER(C.c_int64))
        out = None
        if want_out:
            out = np.full((self.P, 8), np.nan, dtype=F32)
            a.out = _fp(out)
        N.check(self._L.frl_cem_gd3pg_learn(self._h, C.byref(a)))
        return out

    def gail_learn(self, policy_rows, *, gp, lr, beta1, beta2, n_expert=None, gp_weight=5.0, adam_eps=1e-8, idx=None, want_out=True,
                   want_idx=False):
        """GAIL.trian_D for every learner (frl_gail_learn): policy_rows [P][n_policy][obs_dim + act_dim] against expert ring rows
        idx [P][n_expert] (None: n_expert rows drawn with replacement on the device).  gp False: sigmoid + BCE; True: logits,
        0.5 x BCE-with-logits + gp_weight x the gradient penalty on the expert rows.
        -> dict with `out` [P][6] = d_loss, expert_prob, policy_prob, w_dis, penalty mean, gradient norm and / or `idx`
        [P][n_expert] (the rows used); empty and asynchronous when neither is asked for."""
        rows = np.ascontiguousarray(policy_rows, dtype=F32)
        cols = self.layout.obs_dim[0] + self.layout.act_dim[0]
        rows = rows.reshape(self.P, rows.size // (self.P * cols), cols)
        a = N.GailArgs()
        keep = [rows]
        if idx is not None:
            ix = np.ascontiguousarray(idx, dtype=np.int64).reshape(self.P, -1)
            keep.append(ix)
            a.idx = ix.ctypes.data_as(C.POINTER(C.c_int64))
            n_expert = ix.shape[1] if n_expert is None else n_expert
        a.n_expert, a.n_policy, a.gp, a.gp_weight = int(n_expert), rows.shape[1], int(gp), float(gp_weight)
        a.lr, a.beta1, a.beta2, a.adam_eps = float(lr), float(beta1), float(beta2), float(adam_eps)
        a.policy_rows = _fp(rows)
        out = {}
        if want_out:
            out["out"] = np.full((self.P, 6), np.nan, dtype=F32)
            a.out = _fp(out["out"])
        if want_idx:
            out["idx"] = np.full((self.P, max(int(n_expert), 0)), -1, dtype=np.int64)
            a.idx_out = out["idx"].ctypes.data_as(C.POINTER(C.c_int64))
        N.check(self._L.frl_gail_learn(self._h, C.byref(a)))
        return out

    def gail_reward(self, rows, *, gp):
        """GAIL.compute_reward (frl_gail_reward): rows [P][n][obs_dim + act_dim] -> float32 [P][n]."""
        x = np.ascontiguousarray(rows, dtype=F32).reshape(self.P, -1, self.layout.obs_dim[0] + self.layout.act_dim[0])
        out = np.empty((self.P, x.shape[1]), dtype=F32)
        N.check(self._L.frl_gail_reward(self._h, int(gp), x.shape[1], _fp(x), _fp(out)))
        return out

    def net_norm_set(self, feature_norm, layer_norm):
        """trick['feature_norm'] / trick['LayerNorm'] of a MAPPO / IPPO engine (frl_net_norm_set); both off at create."""
        N.check(self._L.frl_net_norm_set(self._h, int(bool(feature_norm)), int(bool(layer_norm))))

    def action_mask_set(self, on=True):
        """invalid-action masking of a discrete FRL_ALGO_MAPPO engine whose extra columns end with one mask block per agent
        (frl_action_mask_set): mappo_learn then reads the masks, and act_masked serves select_action."""
        N.check(self._L.frl_action_mask_set(self._h, int(bool(on))))

    def act_masked(self, net, obs, mask, *, eps=None, want_logp=False):
        """CategoricalMasked(logits = actor(obs), masks = mask).sample() (frl_act_masked): obs [P, n_rows, in_dim], mask [P, n_rows, A]
        (nonzero = available), eps [P, n_rows, A] Exp(1) draws (None: drawn on the device) -> action index [P, n_rows] (and its
        log-prob [P, n_rows] with want_logp).  2-D inputs when P == 1."""
        obs = np.ascontiguousarray(obs, dtype=F32)
        if obs.ndim == 2:
            obs = obs[None]
        P, n_rows, in_dim = obs.shape
        assert P == self.P
        mask = np.ascontiguousarray(mask, dtype=F32).reshape(P, n_rows, -1)
        assert 0 <= int(net) < self.n_nets and mask.shape[2] == self.cfg.act_dim[int(net) // 2], mask.shape
        ep = None
        if eps is not None:
            eps = np.ascontiguousarray(eps, dtype=F32).reshape(mask.shape)
            ep = _fp(eps)
        out = np.empty((P, n_rows), dtype=F32)
        logp = np.empty((P, n_rows), dtype=F32) if want_logp else None
        N.check(self._L.frl_act_masked(self._h, int(net), n_rows, in_dim, _fp(obs), _fp(mask), ep, _fp(out), _fp(logp) if want_logp else None))
        return (out, logp) if want_logp else out

    def _mappo_args(self, a, keep, out, horizon, minibatch, k_epochs, *, gamma, lmbda, clip, ent_coef, actor_lr, critic_lr, adam_eps=1e-8,
                    clip_norm=0.5, adv_norm=False, value_clip=False, huber_delta=None, perms=None, want_trace=False, want_adv=False):
        """fills frl_mappo_args' fields of `a` (a MappoArgs, or a HappoArgs, which begins with them)"""
        a.horizon, a.minibatch, a.k_epochs = int(horizon), int(minibatch), int(k_epochs)
        a.gamma, a.lmbda, a.clip, a.ent_coef = gamma, lmbda, clip, ent_coef
        a.actor_lr, a.critic_lr, a.adam_eps, a.clip_norm = actor_lr, critic_lr, adam_eps, clip_norm
        a.adv_norm, a.value_clip = int(bool(adv_norm)), int(bool(value_clip))
        if huber_delta is not None:
            a.loss_kind, a.huber_delta = N.LOSS_HUBER, float(huber_delta)
        if perms is not None:
            pm = np.ascontiguousarray(perms, dtype=np.int64).reshape(self.P, self.n_agents, int(k_epochs), int(horizon))
            keep.append(pm)
            a.perms = pm.ctypes.data_as(C.POINTER(C.c_int64))
        n_mb = (int(horizon) + int(minibatch) - 1) // max(int(minibatch), 1)      # (minibatch < 1: the library refuses the call)
        if want_trace:
            out["trace"] = np.zeros((self.P, self.n_agents, int(k_epochs) * n_mb, 2), dtype=F32)
            a.loss_trace_out = _fp(out["trace"])
        if want_adv:
            out["adv"] = np.zeros((self.P, int(horizon), self.n_agents), dtype=F32)
            out["v_target"] = np.zeros((self.P, int(horizon), self.n_agents), dtype=F32)
            a.adv_out, a.vtarget_out = _fp(out["adv"]), _fp(out["v_target"])

    def mappo_learn(self, horizon, minibatch, k_epochs, **kw):
        """MAPPO.learn / IPPO.learn for every learner (frl_mappo_learn): gamma, lmbda, clip, ent_coef, actor_lr, critic_lr, adam_eps=1e-8,
        clip_norm=0.5, adv_norm, value_clip, huber_delta (None: F.mse_loss), perms [P][n_agents][k_epochs][horizon] (None: drawn on the
        device).  -> dict with `trace` [P][n_agents][k_epochs * n_mb][2] (want_trace) and / or `adv` (before normalisation) and
        `v_target`, both [P][horizon][n_agents] (want_adv)."""
        a, keep, out = N.MappoArgs(), [], {}
        self._mappo_args(a, keep, out, horizon, minibatch, k_epochs, **kw)
        N.check(self._L.frl_mappo_learn(self._h, C.byref(a)))
        return out

    def happo_learn(self, horizon, minibatch, k_epochs, *, agent_order=None, want_factor=False, **kw):
        """HAPPO.learn for every learner (frl_happo_learn): mappo_learn's arguments (perms and `trace` indexed by agent id), and
        agent_order [P][n_agents], the agent visited at each position (None: drawn on the host from the engine's seed).  want_factor
        adds `factor` [P][n_agents][horizon] by visiting position: what the k-th visited agent's steps were weighted with."""
        a, keep, out = N.HappoArgs(), [], {}
        self._mappo_args(a, keep, out, horizon, minibatch, k_epochs, **kw)
        if agent_order is not None:
            od = np.ascontiguousarray(agent_order, dtype=np.int32).reshape(self.P, self.n_agents)
            keep.append(od)
            a.agent_order = od.ctypes.data_as(C.POINTER(C.c_int32))
        if want_factor:
            out["factor"] = np.zeros((self.P, self.n_agents, int(horizon)), dtype=F32)
            a.factor_out = _fp(out["factor"])
        N.check(self._L.frl_happo_learn(self._h, C.byref(a)))
        return out

    # ------------------------------------------------------------------ timing
    def ppo_work(self, horizon, k_epochs):
        fl, by = C.c_double(0), C.c_double(0)
        N.check(self._L.frl_ppo_work(self._h, int(horizon), int(k_epochs), C.byref(fl), C.byref(by)))
        return fl.value, by.value

    def timer_start(self):
        N.check(self._L.frl_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float(0)
        N.check(self._L.frl_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def profile(self, on):
        N.check(self._L.frl_profile_enable(self._h, int(bool(on))))

    def profile_read(self):
        """-> {slot name: (total ms, launches)} of frl_learn's kernels since profile(True)."""
        ms = (C.c_double * 8)()
        cnt = (C.c_longlong * 8)()
        N.check(self._L.frl_profile_read(self._h, ms, cnt))
        names = ["draw", "grad_critic", "adam_critic", "grad_actor", "adam_actor", "soft_update", "ppo", "_"]
        return {names[k]: (ms[k], cnt[k]) for k in range(8) if cnt[k]}

    def obsnorm_enable(self, on=True):
        N.check(self._L.frl_obsnorm_enable(self._h, int(bool(on))))

    def obsnorm_stats(self, learner=0, agent=0):
        """-> dict(n, mean[O], S[O], std[O]) of the Batch_ObsNorm running statistics (of one agent of a MADDPG engine)."""
        w = 1 + 3 * max(self.layout.obs_dim[j] for j in range(self.n_agents))
        buf = np.zeros(self.n_agents * w, dtype=F32)
        N.check(self._L.frl_obsnorm_get(self._h, int(learner), _fp(buf)))
        O, b = self.layout.obs_dim[agent], buf[agent * w:(agent + 1) * w]
        return dict(n=int(b[0]), mean=b[1:1 + O].copy(), S=b[1 + O:1 + 2 * O].copy(), std=b[1 + 2 * O:1 + 3 * O].copy())
