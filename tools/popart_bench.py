"""learn() time of PopArt DDPG (kernels_popart.hip, frl_popart_ddpg_learn) at the reference script's nets on its smallest shape:

  obs 3, 1 action (Pendulum-v1), hidden 128, batches of 64 (the script's) and 256

per population P (default 1 and 64), next to two yardsticks on the same build and device:
  ddpg    Engine(ALGO_DDPG).learn() at the same dims and batch, pinned to the row-chunk kernels (FRL_CRITIC_V2=0, FRL_SOLO=0,
          FRL_SOLOW=0 at create): the same critic and actor update without the target launch and the upper layer;
  eager   the same PopArt update written in eager PyTorch on the same GPU, one learner (a population is that many times the call).
Rows are drawn on the device; warm-up, then timed blocks of calls with one synchronisation per block (tools/cem_gd3pg_bench.py's
timing); the figure is the median block.  One JSON line per point, appended to profiles/popart/popart_bench.jsonl with --write.
    python tools/popart_bench.py [--write] [P ...]
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

O, A, H, ROWS = 3, 1, 128, 4096
BATCHES = (64, 256)
WARM, BLOCK, BLOCKS = 5, 20, 7
KW = dict(gamma=0.99, tau=0.01, actor_lr=1e-3, critic_lr=1e-3)


def _fill(e, P):
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            flat = (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32)
            for k in (N.PARAM_ONLINE, N.PARAM_TARGET):
                e.set_params(net, flat, k, learner=p)
    e.fill_synthetic(ROWS, seed=3)


def _popart_engine(P, B):
    e = Engine(N.ALGO_DDPG_POPART, O, A, ROWS, n_learners=P, hidden=H, batch_max=B, seed=1)
    _fill(e, P)
    return e, lambda **kw: e.popart_ddpg_learn(B, want_out=bool(kw), **KW)


def _ddpg_engine(P, B):
    old = {k: os.environ.get(k) for k in ("FRL_CRITIC_V2", "FRL_SOLO", "FRL_SOLOW")}
    os.environ.update(FRL_CRITIC_V2="0", FRL_SOLO="0", FRL_SOLOW="0")          # the row-chunk kernels, whatever the population
    try:
        e = Engine(N.ALGO_DDPG, O, A, ROWS, n_learners=P, hidden=H, batch_max=B, seed=1)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert not e.learn_path(B)[0], "the DDPG yardstick must run on the row-chunk kernels"
    _fill(e, P)
    return e, lambda **kw: e.learn(B, want_stats=bool(kw), **KW)


def _eager(B):
    """DDPG_simple_with_tricks.py:253-292 in eager PyTorch on the GPU, rows gathered from device-resident tables"""
    import copy
    import torch
    dev = torch.device("cuda")

    def mlp(i, o):
        return torch.nn.Sequential(torch.nn.Linear(i, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(), torch.nn.Linear(H, o)).to(dev)
    actor, critic, upper = mlp(O, A), mlp(O + A, 1), torch.nn.Linear(1, 1).to(dev)
    actor_t, critic_t = copy.deepcopy(actor), copy.deepcopy(critic)
    oa, ol, ou = (torch.optim.Adam(m.parameters(), lr=1e-3) for m in (actor, critic, upper))
    st = dict(sigma=torch.ones((), device=dev), mu=torch.zeros((), device=dev), nu=torch.ones((), device=dev))
    tab = dict(obs=torch.randn(ROWS, O, device=dev), act=torch.rand(ROWS, A, device=dev) * 2 - 1, rew=torch.randn(ROWS, 1, device=dev),
               nobs=torch.randn(ROWS, O, device=dev), done=(torch.rand(ROWS, 1, device=dev) < 0.05).float())
    clip, beta = torch.nn.utils.clip_grad_norm_, 0.99999

    def learn():
        idx = torch.randperm(ROWS, device=dev)[:B]
        obs, act, rew, nobs, done = (tab[k][idx] for k in ("obs", "act", "rew", "nobs", "done"))
        with torch.no_grad():
            y = rew + 0.99 * (1 - done) * (st["sigma"] * upper(critic_t(torch.cat([nobs, torch.tanh(actor_t(nobs))], 1))) + st["mu"])
            mu_new = (1 - beta) * st["mu"] + beta * y.mean()
            st["nu"] = (1 - beta) * st["nu"] + beta * (y * y).mean()
            sigma_new = torch.sqrt(st["nu"] - mu_new ** 2)
            upper.weight.mul_(st["sigma"] / sigma_new)
            upper.bias.mul_(st["sigma"] / sigma_new).add_((st["mu"] - mu_new) / sigma_new)
            st["sigma"], st["mu"] = sigma_new, mu_new
        loss = torch.nn.functional.mse_loss(upper(critic(torch.cat([obs, act], 1))), (y - st["mu"]) / st["sigma"])
        ol.zero_grad(); ou.zero_grad(); loss.backward()
        clip(critic.parameters(), 0.5); ol.step(); clip(upper.parameters(), 0.5); ou.step()
        aloss = -(st["sigma"] * upper(critic(torch.cat([obs, torch.tanh(actor(obs))], 1))) + st["mu"]).mean()
        oa.zero_grad(); aloss.backward(); clip(actor.parameters(), 0.5); oa.step()
        with torch.no_grad():
            for tg, src in ((critic_t, critic), (actor_t, actor)):
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
    for B in BATCHES:
        e, learn = _eager(B)          # (first: torch initialises the device before the library's engines exist, as under pytest)
        eager = _time(e, learn)
        for P in ps:
            point = dict(P=P, obs=O, act=A, hidden=H, batch=B, calls=BLOCK * BLOCKS, eager_torch_us_one_learner=round(eager[0], 1),
                         eager_us_min_max=[round(eager[1], 1), round(eager[2], 1)])
            for name, make in (("popart", _popart_engine), ("ddpg_rowchunk", _ddpg_engine)):
                e, learn = make(P, B)
                med, lo, hi = _time(e, learn)
                out = learn(check=True)
                point[name + "_us"], point[name + "_us_min_max"] = round(med, 1), [round(lo, 1), round(hi, 1)]
                point[name + "_finite"] = bool(np.all(np.isfinite(out)))
                point[name + "_lds_rc"] = e.lds_bytes()
                e.close()
            point["popart_over_ddpg"] = round(point["popart_us"] / point["ddpg_rowchunk_us"], 2)
            point["eager_over_popart"] = round(P * eager[0] / point["popart_us"], 1)
            lines.append(point)
            print(json.dumps(point), flush=True)
    if write:
        os.makedirs(os.path.join(ROOT, "profiles", "popart"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "popart", "popart_bench.jsonl"), "a") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines))


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--write"]
    main([int(x) for x in argv] or [1, 64], "--write" in sys.argv[1:])
