"""The cases of tests/test_gpu_onpolicy_draws.py and of its fixture's maker (tests/golden/make_onpolicy_draws_golden.py): one
`perms=None` learn call of each on-policy entry point — HAPPO with `agent_order=None` too — on an engine created with a fixed seed.

Shapes: hidden 32, observations of width 3, actions of width 2, two learners, K = 1, two agents for MAPPO and HAPPO; horizon 40 in
minibatches of 16 (ppo_perm_kernel's draw, a ragged last minibatch of 8 rows) and horizon 8193 in one minibatch (past 8192 rows the
host shuffle draws).  Nets and rows are synthetic, from NumPy's PCG64 under a fixed seed; the engine's seed reaches nothing but the
draws.  What a case yields is every net's parameters and Adam first moments, learner by learner: with one minibatch and K = 1 the
parameters take one Adam step of about +-lr whatever the row order, the first moment keeps the gradient sum's own bits."""
import numpy as np

F32 = np.float32
ENTRIES = ("ppo", "gail_ppo", "mappo", "happo")
SHAPES = ((40, 16), (8193, 8193))                      # (horizon, minibatch)
CASES = [(entry, T, mb) for entry in ENTRIES for T, mb in SHAPES]
SEED, OTHER_SEED = 20240607, 77
O, A, HIDDEN, P, K = 3, 2, 32, 2, 1
HYPER = dict(gamma=0.99, clip=0.2, clip_norm=0.5)


def name(entry, T, mb):
    return "%s_T%d_mb%d" % (entry, T, mb)


def _engine(N, entry, T, mb, seed):
    from freerl_amd.engine import Engine
    kw = dict(n_learners=P, hidden=HIDDEN, batch_max=mb, seed=seed)
    if entry == "ppo":
        return Engine(N.ALGO_PPO, O, A, T, extra_cols=A + 1, **kw)
    if entry == "gail_ppo":
        return Engine(N.ALGO_GAIL_PPO, O, A, T, **kw)
    return Engine(N.ALGO_MAPPO if entry == "mappo" else N.ALGO_HAPPO, [O, O], [A, A], T, extra_cols=2 * A + 2, **kw)


def _fill(e, entry, T):
    """the same nets and rows whatever the engine's seed"""
    g = np.random.default_rng(5)
    for p in range(P):
        for net in range(e.n_nets):
            e.set_params(net, (g.standard_normal(e.num_params(net)) * 0.1).astype(F32), learner=p)
    lay, n = e.layout, e.n_agents
    rec = (g.standard_normal((P * T, e.width)) * 0.5).astype(F32)
    rec[:, lay.done_off:lay.done_off + n] = g.random((P * T, n)) < 0.02
    if entry != "gail_ppo":                            # the log-prob blocks, then one adv_done column per agent
        rec[:, lay.extra_off + n * A:lay.extra_off + n * A + n] = g.random((P * T, n)) < 0.02
    e.add_batch(rec, learners=np.repeat(np.arange(P), T).astype(np.int32))


def run(N, entry, T, mb, seed=SEED):
    """-> float32 [everything]: (parameters, Adam m) of net 0, 1, .. of learner 0, then learner 1's"""
    e = _engine(N, entry, T, mb, seed)
    try:
        _fill(e, entry, T)
        if entry == "ppo":
            e.ppo_learn(T, mb, K, lmbda=0.95, ent_coef=0.01, actor_lr=3e-4, critic_lr=3e-4, adv_norm=True, perms=None, **HYPER)
        elif entry == "gail_ppo":
            e.gail_ppo_learn(T, mb, K, lam=0.95, ent_weight=0.01, value_loss_coef=0.5, p_lr=3e-4, v_lr=3e-4, perms=None, **HYPER)
        elif entry == "mappo":
            e.mappo_learn(T, mb, K, lmbda=0.95, ent_coef=0.01, actor_lr=3e-4, critic_lr=3e-4, adv_norm=True, perms=None, **HYPER)
        else:
            e.happo_learn(T, mb, K, lmbda=0.95, ent_coef=0.01, actor_lr=3e-4, critic_lr=3e-4, adv_norm=True, perms=None, agent_order=None,
                          **HYPER)
        out = np.concatenate([e.get_params(net, kind, p) for p in range(P) for net in range(e.n_nets) for kind in (N.PARAM_ONLINE, N.PARAM_ADAM_M)])
    finally:
        e.close()
    assert np.all(np.isfinite(out)), name(entry, T, mb)
    return out
