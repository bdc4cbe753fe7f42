"""learn() time of CEM_GD3PG (kernels_cem_gd3pg.hip, frl_cem_gd3pg_learn) at the reference script's shape:

  obs 24, 4 actions (BipedalWalker-v3), hidden 128, batch 256 = 128 rows of each ring per call

per population P (default 1 and 64), next to two yardsticks on the same build and device:
  ddpg    Engine(ALGO_DDPG).learn() at the same dims and batch, pinned to the row-chunk kernels (FRL_CRITIC_V2=0, FRL_SOLO=0,
          FRL_SOLOW=0 at create): one critic and one actor update where CEM_GD3PG has one critic and two actor updates behind six
          gradient-free forwards — by multiply-adds roughly three DDPG updates;
  eager   the same CEM_GD3PG update written in eager PyTorch on the same GPU, one learner (a population is that many times the call).
Rows are drawn on the device; warm-up, then timed blocks of calls with one synchronisation per block (tools/envelope_bench.py's
timing); the figure is the median block.  One JSON line per point, appended to profiles/cem_gd3pg/cem_gd3pg_bench.jsonl with --write.
    python tools/cem_gd3pg_bench.py [--write] [P ...]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

O, A, H, B, ROWS = 24, 4, 128, 256, 4096
WARM, BLOCK, BLOCKS = 5, 20, 7
KW = dict(gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3)


def _fill_params(e, P):
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            flat = (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32)
            for k in (N.PARAM_ONLINE, N.PARAM_TARGET):
                e.set_params(net, flat, k, learner=p)


def _cem_engine(P):
    e = Engine(N.ALGO_CEM_GD3PG, O, A, ROWS, n_learners=P, hidden=H, hidden_act=N.ACT_TANH, batch_max=B, seed=1)
    _fill_params(e, P)
    g = np.random.default_rng(2)
    rows = g.standard_normal((ROWS, e.width)).astype(np.float32)
    rows[:, e.layout.done_off] = g.random(ROWS) < 0.05
    for ring in (0, 1):
        for p in range(P):
            e.ring_add_batch(ring, rows, learners=np.full(ROWS, p, np.int32))
    e.flush()
    return e, lambda **kw: e.cem_gd3pg_learn(B, f1_more=True, delta=0.5, want_out=bool(kw), **KW)


def _ddpg_engine(P):
    old = {k: os.environ.get(k) for k in ("FRL_CRITIC_V2", "FRL_SOLO", "FRL_SOLOW")}
    os.environ.update(FRL_CRITIC_V2="0", FRL_SOLO="0", FRL_SOLOW="0")          # the row-chunk kernels, whatever the population
    try:
        e = Engine(N.ALGO_DDPG, O, A, ROWS, n_learners=P, hidden=H, batch_max=B, seed=1)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert not e.learn_path(B)[0], "the DDPG yardstick must run on the row-chunk kernels"
    _fill_params(e, P)
    e.fill_synthetic(ROWS, seed=3)
    return e, lambda **kw: e.learn(B, want_stats=bool(kw), **KW)


def _eager():
    """CEM_GD3PG.py:180-231 in eager PyTorch on the GPU, rows gathered from device-resident tables"""
    import torch
    dev = torch.device("cuda")
    F = torch.nn.functional

    def mlp(i, o):
        return torch.nn.Sequential(torch.nn.Linear(i, H), torch.nn.Identity(), torch.nn.Linear(H, H), torch.nn.Identity(), torch.nn.Linear(H, o)).to(dev)

    def pi(net, s):
        return torch.tanh(net[4](torch.tanh(net[2](torch.tanh(net[0](s))))))

    def q(net, s, a):
        return net[4](F.leaky_relu(net[2](F.leaky_relu(net[0](torch.cat([s, a], 1))))))
    actors, critic = [mlp(O, A), mlp(O, A)], mlp(O + A, 1)
    import copy
    actors_t, critic_t, domain = [copy.deepcopy(a) for a in actors], copy.deepcopy(critic), mlp(O, A)
    opts = [torch.optim.Adam(a.parameters(), lr=1e-3) for a in actors] + [torch.optim.Adam(critic.parameters(), lr=1e-3)]
    tab = [dict(obs=torch.randn(ROWS, O, device=dev), act=torch.rand(ROWS, A, device=dev) * 2 - 1, rew=torch.randn(ROWS, 1, device=dev),
                nobs=torch.randn(ROWS, O, device=dev), done=(torch.rand(ROWS, 1, device=dev) < 0.05).float()) for _ in range(2)]

    def learn():
        idx = [torch.randperm(ROWS, device=dev)[:B // 2] for _ in range(2)]
        cat = lambda k: torch.cat([tab[0][k][idx[0]], tab[1][k][idx[1]]])
        obs, act, rew, nobs, done = cat("obs"), cat("act"), cat("rew"), cat("nobs"), cat("done")
        tq = torch.min(q(critic_t, nobs, pi(actors_t[0], nobs)), q(critic_t, nobs, pi(actors_t[1], nobs)))
        loss = F.mse_loss(q(critic, obs, act), (rew + 0.99 * tq * (1 - done)).detach())
        opts[2].zero_grad(); loss.backward(); torch.nn.utils.clip_grad_norm_(critic.parameters(), 0.5); opts[2].step()
        q1, q2 = q(critic, obs, pi(actors[0], obs)).mean(), q(critic, obs, pi(actors[1], obs)).mean()
        opts[0].zero_grad(); (-q1).backward(); torch.nn.utils.clip_grad_norm_(actors[0].parameters(), 0.5); opts[0].step()
        c = pi(actors[1], obs) - pi(domain, obs)
        l2 = -q2 + 10 * 0.5 * torch.sqrt(torch.sum(c * c) / len(c))
        opts[1].zero_grad(); l2.backward(); torch.nn.utils.clip_grad_norm_(actors[1].parameters(), 0.5); opts[1].step()
        with torch.no_grad():
            for tg, src in ((critic_t, critic), (actors_t[0], actors[0]), (actors_t[1], actors[1])):
                for a, b in zip(tg.parameters(), src.parameters()):
                    a.mul_(0.99).add_(b, alpha=0.01)

    class _E:
        sync = staticmethod(torch.cuda.synchronize)
        close = staticmethod(lambda: None)
    return _E, lambda **kw: learn()


def _time(e, learn):
    def block(n):
        e.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            learn()
        e.sync()
        return (time.perf_counter() - t0) / n
    block(WARM)
    us = sorted(1e6 * block(BLOCK) for _ in range(BLOCKS))
    return us[len(us) // 2], us[0], us[-1]


def main(ps, write):
    lines = []
    e, learn = _eager()          # (first: torch initialises the device before the library's engines exist, as under pytest)
    eager_med, eager_lo, eager_hi = _time(e, learn)
    for P in ps:
        point = dict(P=P, obs=O, act=A, hidden=H, batch=B, calls=BLOCK * BLOCKS)
        for name, make in (("cem_gd3pg", _cem_engine), ("ddpg_rowchunk", _ddpg_engine)):
            e, learn = make(P)
            med, lo, hi = _time(e, learn)
            out = learn(check=True)
            point[name + "_us"], point[name + "_us_min_max"] = round(med, 1), [round(lo, 1), round(hi, 1)]
            point[name + "_finite"] = bool(np.all(np.isfinite(out)))
            point[name + "_lds_rc"] = e.lds_bytes()
            e.close()
        point["cem_over_ddpg"] = round(point["cem_gd3pg_us"] / point["ddpg_rowchunk_us"], 2)
        lines.append(point)
        print(json.dumps(point), flush=True)
    point = dict(eager_torch_us_one_learner=round(eager_med, 1), eager_us_min_max=[round(eager_lo, 1), round(eager_hi, 1)])
    for ln in lines:
        point["eager_over_cem_P%d" % ln["P"]] = round(ln["P"] * eager_med / ln["cem_gd3pg_us"], 1)
    lines.append(point)
    print(json.dumps(point), flush=True)
    if write:
        os.makedirs(os.path.join(ROOT, "profiles", "cem_gd3pg"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "cem_gd3pg", "cem_gd3pg_bench.jsonl"), "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--write"]
    main([int(x) for x in argv] or [1, 64], "--write" in sys.argv[1:])
