"""Time of GAIL's policy update (kernels_gail_ppo.hip, `frl_gail_ppo_learn`) at the reference script's shape:

  s_dim 3, a_dim 1, hidden 128, horizon 2048, minibatch 64, K_epochs 10 (320 steps per net), permutations drawn on the device

Per population P (default 1 and 64): one PPO_learn with LeakyReLU and with ReLU hidden layers; beside it `frl_ppo_learn` at the same
dims with ReLU, forced onto the streaming ppo_update_kernel (FRL_PPO_STREAMING=1: the same per-step work — the yardstick) and unforced
(the on-chip kernels_ppo2.hip: the size of a follow-up); the same update in eager torch on the same device (P = 1 only: P learners one
after the other is P times that); and one full GAIL.train iteration through the classes — trian_D + compute_reward + PPO_learn.
Warm-up, then timed blocks of calls with one synchronisation per block (every call here ends synchronised).  One JSON line per point.
    python tools/gail_ppo_bench.py [--no-torch] [P ...]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

O, A, H, T, MB, K = 3, 1, 128, 2048, 64, 10
WARM, BLOCK, BLOCKS = 2, 5, 4             # 4 blocks of 5 = 20 timed calls per point (a call is 320 dependent steps)
HYP = dict(gamma=0.99, clip=0.2)


def _timed(fn, sync=lambda: None, warm=WARM, block=BLOCK, blocks=BLOCKS):
    def run(n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return (time.perf_counter() - t0) / n
    if warm:
        run(warm)
    ts = [1e3 * run(block) for _ in range(blocks)]
    return dict(call_ms=round(float(np.mean(ts)), 3), block_min_ms=round(min(ts), 3), block_max_ms=round(max(ts), 3), calls=block * blocks)


def _rows(e, P, extra):
    g = np.random.default_rng(4)
    lay, n = e.layout, P * T
    rec = np.zeros((n, e.width), np.float32)
    rec[:, lay.obs_off[0]:lay.obs_off[0] + O] = g.uniform(-1, 1, (n, O))
    rec[:, lay.act_off[0]:lay.act_off[0] + A] = g.uniform(-1, 1, (n, A))
    rec[:, lay.rew_off] = g.standard_normal(n)
    rec[:, lay.done_off] = g.random(n) < 0.005
    rec[:, lay.next_obs_off[0]:lay.next_obs_off[0] + O] = g.uniform(-1, 1, (n, O))
    if extra:                              # frl_ppo_learn's stored log-prob and adv_done columns
        rec[:, lay.extra_off] = -1.2
        rec[:, lay.extra_off + 1] = rec[:, lay.done_off]
    e.add_batch(rec, learners=np.repeat(np.arange(P), T))
    e.flush()
    for p in range(P):
        for net in (0, 1):
            e.set_params(net, (np.random.default_rng(10 * p + net).standard_normal(e.num_params(net)) * 0.05).astype(np.float32), learner=p)


def gail_ppo_point(P, act):
    e = Engine(N.ALGO_GAIL_PPO, O, A, T, n_learners=P, hidden=H, hidden_act=act, batch_max=MB)
    _rows(e, P, False)
    kw = dict(lam=0.95, ent_weight=0.01, value_loss_coef=1.0, p_lr=1e-4, v_lr=3e-4, **HYP)
    r = _timed(lambda: e.gail_ppo_learn(T, MB, K, **kw))
    tr = e.gail_ppo_learn(T, MB, K, want=("trace",), **kw)["trace"]
    r.update(finite=bool(np.isfinite(tr).all()), lds_rc=e.lds_bytes())
    e.close()
    return r


def ppo_point(P, streaming):
    os.environ.pop("FRL_PPO_STREAMING", None)
    if streaming:
        os.environ["FRL_PPO_STREAMING"] = "1"
    e = Engine(N.ALGO_PPO, O, A, T, n_learners=P, hidden=H, hidden_act=N.ACT_RELU, batch_max=MB, extra_cols=2)
    _rows(e, P, True)
    kw = dict(lmbda=0.95, ent_coef=0.01, actor_lr=1e-4, critic_lr=3e-4, adv_norm=True, **HYP)
    r = _timed(lambda: e.ppo_learn(T, MB, K, **kw))
    tr = e.ppo_learn(T, MB, K, want_trace=True, **kw)["trace"]
    r.update(finite=bool(np.isfinite(tr).all()), lds_rc=e.lds_bytes())
    e.close()
    os.environ.pop("FRL_PPO_STREAMING", None)
    return r


def torch_point(act):
    """PPO_learn (GAIL_file/PPO2.py:235-307) restated in eager torch on the device, one learner, rows already there."""
    import torch
    import torch.nn.functional as F
    from torch.distributions import Normal
    dev = torch.device("cuda")
    torch.manual_seed(0)
    mk = (lambda: torch.nn.LeakyReLU()) if act == N.ACT_LEAKY_RELU else (lambda: torch.nn.ReLU())
    net = lambda out: torch.nn.Sequential(torch.nn.Linear(O, H), mk(), torch.nn.Linear(H, H), mk(), torch.nn.Linear(H, out)).to(dev)  # noqa: E731
    P_, V_ = net(A), net(1)
    log_std = torch.nn.Parameter(torch.zeros(1, A, device=dev))
    opt = torch.optim.Adam([{"params": list(P_.parameters()) + [log_std], "lr": 1e-4}, {"params": V_.parameters(), "lr": 3e-4}])
    s, a = torch.rand(T, O, device=dev) * 2 - 1, torch.rand(T, A, device=dev) * 2 - 1
    rew, m2 = torch.randn(T, device=dev), (torch.rand(T, device=dev) > 0.005).float()

    def dist(x):
        mean = torch.tanh(P_(x))
        return Normal(mean, torch.exp(torch.clamp(log_std.expand_as(mean), -10, 2)))

    def learn():
        with torch.no_grad():
            v = V_(s).squeeze(-1)
            lp_old = dist(s).log_prob(a).sum(-1, keepdim=True)
            vals = torch.cat([v, torch.zeros(1, device=dev)]).cpu()          # the reference's Python loop over the horizon, on host copies
            r_, m_ = rew.cpu(), m2.cpu()
            adv, last = torch.zeros(T), 0.0
            for t in reversed(range(T)):
                last = r_[t] + 0.99 * vals[t + 1] - vals[t] + 0.99 * 0.95 * m_[t] * last
                adv[t] = last
            ret = (adv + vals[:-1]).to(dev).reshape(-1, 1)
            adv = ((adv - adv.mean()) / (adv.std() + 1e-8)).to(dev).reshape(-1, 1)
        for _ in range(K):
            idx = torch.randperm(T, device=dev)
            for i in range(0, T, MB):
                j = idx[i:i + MB]
                d = dist(s[j])
                ratio = torch.exp(d.log_prob(a[j]).sum(-1, keepdim=True) - lp_old[j])
                pl = -torch.min(ratio * adv[j], torch.clamp(ratio, 0.8, 1.2) * adv[j]).mean() - 0.01 * d.entropy().sum(-1).mean()
                loss = pl + F.mse_loss(V_(s[j]), ret[j])
                opt.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(list(P_.parameters()) + [log_std], 0.5)
                torch.nn.utils.clip_grad_norm_(V_.parameters(), 0.5)
                opt.step()
        return loss
    r = _timed(learn, torch.cuda.synchronize, warm=1, block=2, blocks=2)
    r["finite"] = bool(torch.isfinite(learn()).item())
    return r


def train_iteration_point():
    """trian_D + compute_reward + PPO_learn through freerl_amd.GAIL.GAIL / freerl_amd.PPO2.PPO at GAIL_COBFIG's values."""
    import torch
    from freerl_amd.GAIL import GAIL, ExpertDataset
    from freerl_amd.PPO2 import PPO
    cfg = dict(seed=42, s_dim=O, a_dim=A, algo="GAIL", log_dir="logs", env_reproducible=True, collect_eval_data=False,
               PPO=dict(policy_mlp_dim=H, activation="LeakyReLU", dropout=0.0, layernorm=False, log_std_min=-10, log_std_max=2, p_lr=1e-4, v_lr=3e-4,
                        horizon=T, gamma=0.99, lam=0.95, clip_epsilon=0.2, K_epochs=K, value_loss_coef=1, ent_weight=0.01, mini_batch_size=MB,
                        eval_interval=10, eval_episodes=1),
               D=dict(d_mlp_dim=H, activation="LeakyReLU", dropout=0.0, layernorm=False, d_lr=4e-4, gp_coef=10.0))
    gail = GAIL(cfg, ppo=PPO(cfg, rng="device"), max_rows=T)
    g = np.random.default_rng(5)
    ds = ExpertDataset((g.standard_normal((8192, O)), g.uniform(-2, 2, (8192, A))))
    gail.load_expert(ds)
    batch = dict(states=torch.rand(T, O) * 2 - 1, actions=torch.rand(T, A) * 2 - 1, rewards=torch.zeros(T), masks_2=(torch.rand(T) > 0.005).float())
    parts = dict(trian_D=0.0, compute_reward=0.0, PPO_learn=0.0)

    def it():
        t0 = time.perf_counter()
        gail.trian_D_indices(gail.next_expert_indices(T), batch["states"], batch["actions"])
        t1 = time.perf_counter()
        b = dict(batch, rewards=gail.compute_reward(batch["states"], batch["actions"]))
        t2 = time.perf_counter()
        gail.ppo.PPO_learn(b, torch.tensor(0.1))
        t3 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[k] += v
    it()
    for k in parts:
        parts[k] = 0.0
    r = _timed(it, warm=0)
    r.update({k + "_ms": round(1e3 * v / r["calls"], 3) for k, v in parts.items()})
    r["finite"] = bool(np.isfinite(gail.ppo.last_learn["trace"]).all())
    return r


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    base = dict(obs=O, act=A, hidden=H, horizon=T, minibatch=MB, k_epochs=K, steps_per_net=K * (T // MB))
    for P in ps:
        for what, fn in (("gail_ppo_learn_leaky", lambda: gail_ppo_point(P, N.ACT_LEAKY_RELU)), ("gail_ppo_learn_relu", lambda: gail_ppo_point(P, N.ACT_RELU)),
                         ("ppo_learn_relu_streaming", lambda: ppo_point(P, True)), ("ppo_learn_relu_onchip", lambda: ppo_point(P, False))):
            print(json.dumps(dict(base, algo="gail_ppo", side="hip", what=what, P=P, **fn())), flush=True)
    print(json.dumps(dict(base, algo="gail_ppo", side="hip", what="gail_train_iteration", P=1, **train_iteration_point())), flush=True)
    if with_torch:
        for what, act in (("gail_ppo_learn_leaky", N.ACT_LEAKY_RELU), ("gail_ppo_learn_relu", N.ACT_RELU)):
            print(json.dumps(dict(base, algo="gail_ppo", side="torch_eager", what=what, P=1, **torch_point(act))), flush=True)


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
