"""learn() time of MASAC (kernels_masac.hip) at MASAC.py's own shape:

  simple_spread_v3 with N = 3: 3 agents x (obs 18, act 5), hidden 128, batch 256

measured in the same run against (a) a MATD3 engine of that shape (FRL_ALGO_MADDPG, twin critic, target policy smoothing, every call a
policy step) forced onto the row-chunk family (FRL_CRITIC_V2=0, FRL_SOLOW=0 at create) and (b) the same update — per agent in order:
critic step on sampled target actions, actor step through all online actors and the minimum of the twins, alpha step; then the soft
updates — in eager torch on the same device, written here.  Per population P: rows and draws on the device, warm-up, then timed blocks
of calls (one synchronisation per block), the timing tools/att_bench.py uses; the engines' per-kernel times come from frl_profile.
Prints one JSON line per (side, P), and per P the ratio MASAC / MATD3 next to the ratio of multiply-adds per row; writes the lines to
profiles/masac/masac_bench.jsonl.
    python tools/masac_bench.py [P ...] [--no-torch]      (default P = 1 64)
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

NA, O, A, H, B, ROWS = 3, 18, 5, 128, 256, 4096
T = NA * (O + A)
WARM, BLOCK, BLOCKS = 3, 5, 4            # 4 blocks of 5 = 20 timed calls per point
KW = dict(gamma=0.95, tau=0.01, actor_lr=1e-4, critic_lr=1e-4)


def macs(masac):
    """multiply-adds per batch row of one agent's update, before padding: forward = 1, weight gradient = 1, input gradient = 1 per layer"""
    actor = O * H + H * H + H * (2 * A if masac else A)
    head = T * H + H * H + H
    critic_stage = NA * actor + 2 * head + 2 * 3 * head                 # target actors, twin target critic, both heads forward + dW + dX
    if masac:       # every online actor, both heads forward and dX, the own actor's backward
        return critic_stage + NA * actor + 2 * head + 2 * head + 2 * actor
    return critic_stage + actor + head + head + 2 * actor               # the own actor, Q1 forward and dX, the actor's backward


def _engine(P, masac):
    knobs = {} if masac else dict(FRL_CRITIC_V2="0", FRL_SOLOW="0")      # MATD3 on the row-chunk family, whatever the population
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        e = Engine(N.ALGO_MASAC if masac else N.ALGO_MADDPG, [O] * NA, [A] * NA, ROWS, n_learners=P, hidden=H, batch_max=B, seed=1, twin_critic=True)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            flat = (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32)
            for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
                e.set_params(net, flat, kind, learner=p)
        if masac:
            for j in range(NA):
                e.set_alpha_state_agent(j, [np.log(0.01), 0.0, 0.0, 0.01], 0, learner=p)
    e.fill_synthetic(ROWS, seed=3)
    return e


def _block(fn, sync, n):
    sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    sync()
    return time.perf_counter() - t0


def _time(fn, sync, warm=WARM, block=BLOCK, blocks=BLOCKS):
    _block(fn, sync, warm)
    return 1e6 * sum(_block(fn, sync, block) for _ in range(blocks)) / (blocks * block)


def bench_engine(P, masac):
    e = _engine(P, masac)
    assert e.learn_path(B)[0] is False
    kw = dict(KW) if masac else dict(KW, use_policy_noise=True, policy_noise=0.2, noise_clip=0.5, do_actor=True)
    us = _time(lambda: e.learn(B, **kw), e.sync)
    e.profile(True)
    for _ in range(BLOCK):
        e.learn(B, **kw)
    e.sync()
    prof = {k: round(1e3 * ms / cnt, 1) for k, (ms, cnt) in e.profile_read().items()}      # us per launch
    e.profile(False)
    st = e.learn(B, **kw, want_stats=True)
    out = dict(side="masac" if masac else "matd3_rowchunk", P=P, agents=NA, obs=O, act=A, hidden=H, batch=B, learn_us=round(us, 1),
               updates_per_s=round(P / us * 1e6, 1), kernels_us=prof, finite=bool(np.all(np.isfinite(st[:, :, :2]))), lds_rc=e.lds_bytes())
    e.close()
    return out


def bench_torch(P):
    """the same update in eager torch on the same device, P learners one after another"""
    import copy
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda")
    lin = torch.nn.Linear

    class Actor(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.l1, self.l2, self.mean, self.ls = lin(O, H), lin(H, H), lin(H, A), lin(H, A)

        def forward(self, x):
            h = F.relu(self.l2(F.relu(self.l1(x))))
            mean, std = self.mean(h), torch.clamp(self.ls(h), -20, 2).exp()
            u = mean + std * torch.randn_like(mean)
            lp = torch.distributions.Normal(mean, std).log_prob(u).sum(1, keepdim=True) - (2 * (np.log(2) - u - F.softplus(-2 * u))).sum(1, keepdim=True)
            return torch.tanh(u), lp

    class Critic(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Sequential(lin(T, H), torch.nn.ReLU(), lin(H, H), torch.nn.ReLU(), lin(H, 1))
            self.b = torch.nn.Sequential(lin(T, H), torch.nn.ReLU(), lin(H, H), torch.nn.ReLU(), lin(H, 1))

        def forward(self, s, a):
            x = torch.cat(list(s) + list(a), dim=1)
            return self.a(x), self.b(x)
    learners = []
    for _ in range(P):
        ac, cr = [Actor().to(dev) for _ in range(NA)], [Critic().to(dev) for _ in range(NA)]
        la = [torch.tensor(np.log(0.01), dtype=torch.float32, device=dev, requires_grad=True) for _ in range(NA)]
        learners.append(dict(ac=ac, cr=cr, act=[copy.deepcopy(m) for m in ac], crt=[copy.deepcopy(m) for m in cr], la=la,
                             aopt=[torch.optim.Adam(m.parameters(), lr=1e-4) for m in ac], copt=[torch.optim.Adam(m.parameters(), lr=1e-4) for m in cr],
                             lopt=[torch.optim.Adam([x], lr=1e-4) for x in la]))
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    ring = dict(obs=rnd(NA, ROWS, O), nobs=rnd(NA, ROWS, O), act=torch.tanh(rnd(NA, ROWS, A)), rew=rnd(NA, ROWS, 1), done=(rnd(NA, ROWS, 1) > 1.5).float())

    def learn():
        for L in learners:
            for i in range(NA):
                idx = torch.randperm(ROWS, device=dev)[:B]
                obs, nobs, act = ring["obs"][:, idx], ring["nobs"][:, idx], ring["act"][:, idx]
                alpha = L["la"][i].exp().detach()
                with torch.no_grad():
                    nxt = [L["act"][j](nobs[j]) for j in range(NA)]
                    qa, qb = L["crt"][i](nobs, [x[0] for x in nxt])
                    tgt = ring["rew"][i, idx] + KW["gamma"] * (1 - ring["done"][i, idx]) * (torch.min(qa, qb) - alpha * nxt[i][1])
                q1, q2 = L["cr"][i](obs, act)
                loss = F.mse_loss(q1, tgt) + F.mse_loss(q2, tgt)
                L["copt"][i].zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(L["cr"][i].parameters(), 0.5)
                L["copt"][i].step()
                new = [L["ac"][j](obs[j])[0] for j in range(NA)]
                q1, q2 = L["cr"][i](obs, new)
                lp2 = L["ac"][i](obs[i])[1]
                aloss = (-torch.min(q1, q2) + alpha * lp2).mean()
                L["aopt"][i].zero_grad()
                aloss.backward()
                torch.nn.utils.clip_grad_norm_(L["ac"][i].parameters(), 0.5)
                L["aopt"][i].step()
                L["lopt"][i].zero_grad()
                (L["la"][i].exp() * (-lp2.detach() + A)).mean().backward()
                L["lopt"][i].step()
            with torch.no_grad():
                for tg, src in zip(L["act"] + L["crt"], L["ac"] + L["cr"]):
                    for tp, sp in zip(tg.parameters(), src.parameters()):
                        tp.mul_(1 - KW["tau"]).add_(sp, alpha=KW["tau"])
    # (a population is P sequential eager updates: fewer timed calls there, 2 blocks of 1)
    us = _time(learn, torch.cuda.synchronize) if P == 1 else _time(learn, torch.cuda.synchronize, 1, 1, 2)
    return dict(side="torch_eager", P=P, agents=NA, obs=O, act=A, hidden=H, batch=B, learn_us=round(us, 1), updates_per_s=round(P / us * 1e6, 1))


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    for P in ps:
        masac, matd3 = bench_engine(P, True), bench_engine(P, False)
        emit(masac)
        emit(matd3)
        if with_torch:
            emit(bench_torch(P))
        emit(dict(side="ratio", P=P, time_masac_over_matd3=round(masac["learn_us"] / matd3["learn_us"], 2),
                  macs_per_row_masac_over_matd3=round(macs(True) / macs(False), 2)))
    out = os.path.join(ROOT, "profiles", "masac")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "masac_bench.jsonl"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
