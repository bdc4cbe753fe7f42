"""learn() time of ATT-MADDPG (kernels_att.hip) at MADDPG_simple_with_tricks.py's own shape:

  simple_spread_v3 with N = 5: 5 agents x (obs 30, act 5), hidden 128, 4 heads, batch 256

measured in the same run against (a) a plain FRL_ALGO_MADDPG engine of that shape forced onto the row-chunk family (FRL_CRITIC_V2=0,
FRL_SOLOW=0 at create) and (b) the same update — per agent: critic step, actor step through the stepped critic, then the soft updates —
in eager torch on the same device.  Per population P: rows drawn on the device, warm-up, then timed blocks of calls (one
synchronisation per block), the timing tools/envelope_bench.py uses; the engines' per-kernel times come from frl_profile.  Prints one
JSON line per (side, P), and per P the ratio ATT / plain next to the critics' multiply-add ratio per row.
    python tools/att_bench.py [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

NA, O, A, H, K, B, ROWS = 5, 30, 5, 128, 4, 256, 4096
WARM, BLOCK, BLOCKS = 3, 5, 4            # 4 blocks of 5 = 20 timed calls per point
KW = dict(gamma=0.95, tau=0.01, actor_lr=1e-3, critic_lr=1e-3)
# multiply-adds per row of one critic forward, before padding: encoder 155 + decoder 20 input columns, 3 + 4 + 1 hidden layers, the head
MACS_ATT = (NA * O + A + (NA - 1) * A) * H + (3 + K) * H * H + H
MACS_PLAIN = (NA * O + NA * A) * H + H * H + H


def _engine(P, att):
    knobs = {} if att else dict(FRL_CRITIC_V2="0", FRL_SOLOW="0")      # the plain engine on the row-chunk family, whatever the population
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        e = Engine(N.ALGO_MADDPG_ATT if att else N.ALGO_MADDPG, [O] * NA, [A] * NA, ROWS, n_learners=P, hidden=H, batch_max=B, seed=1)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            flat = (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32)
            for kind in (N.PARAM_ONLINE, N.PARAM_TARGET):
                e.set_params(net, flat, kind, learner=p)
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


def bench_engine(P, att):
    e = _engine(P, att)
    assert e.learn_path(B)[0] is False
    us = _time(lambda: e.learn(B, **KW), e.sync)
    e.profile(True)
    for _ in range(BLOCK):
        e.learn(B, **KW)
    e.sync()
    prof = {k: round(1e3 * ms / cnt, 1) for k, (ms, cnt) in e.profile_read().items()}      # us per launch
    e.profile(False)
    st = e.learn(B, **KW, want_stats=True)
    out = dict(side="att" if att else "plain_rowchunk", P=P, agents=NA, obs=O, act=A, hidden=H, batch=B, learn_us=round(us, 1),
               updates_per_s=round(P / us * 1e6, 1), kernels_us=prof, finite=bool(np.all(np.isfinite(st[:, :, :2]))), lds_rc=e.lds_bytes())
    e.close()
    return out


def bench_torch(P):
    """the same update in eager torch on the same device, P learners one after another"""
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda")
    lin = torch.nn.Linear

    class Critic(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ei, self.heads, self.di = lin(H, H), torch.nn.ModuleList([lin(H, H) for _ in range(K)]), lin(H, H)
            self.E, self.D, self.fc1, self.fc2 = lin(NA * O + A, H), lin((NA - 1) * A, H), lin(H, H), lin(H, 1)

        def forward(self, xe, xd):
            g, u = F.relu(self.ei(self.E(xe))), F.relu(self.di(self.D(xd)))
            h = torch.stack([F.relu(hd(g)) for hd in self.heads], dim=0)
            w = F.softmax(torch.sum(h * u, dim=2).permute(1, 0), dim=1).unsqueeze(2)
            c = torch.matmul(h.permute(1, 2, 0), w).squeeze(2)
            return self.fc2(F.relu(self.fc1(c)))

    def actor():
        return torch.nn.Sequential(lin(O, H), torch.nn.ReLU(), lin(H, H), torch.nn.ReLU(), lin(H, A), torch.nn.Tanh()).to(dev)
    import copy
    learners = []
    for _ in range(P):
        ac = [actor() for _ in range(NA)]
        cr = [Critic().to(dev) for _ in range(NA)]
        learners.append(dict(ac=ac, cr=cr, act=[copy.deepcopy(m) for m in ac], crt=[copy.deepcopy(m) for m in cr],
                             aopt=[torch.optim.Adam(m.parameters(), lr=1e-3) for m in ac], copt=[torch.optim.Adam(m.parameters(), lr=1e-3) for m in cr]))
    g = torch.Generator(device=dev).manual_seed(3)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    ring = dict(obs=rnd(NA, ROWS, O), nobs=rnd(NA, ROWS, O), act=torch.tanh(rnd(NA, ROWS, A)), rew=rnd(NA, ROWS, 1), done=(rnd(NA, ROWS, 1) > 1.5).float())

    def xin(i, obs, act):
        return torch.cat(list(obs) + [act[i]], dim=1), torch.cat([act[j] for j in range(NA) if j != i], dim=1)

    def learn():
        for L in learners:
            for i in range(NA):
                idx = torch.randperm(ROWS, device=dev)[:B]
                obs, nobs, act = ring["obs"][:, idx], ring["nobs"][:, idx], ring["act"][:, idx]
                with torch.no_grad():
                    nact = [L["act"][j](nobs[j]) for j in range(NA)]
                    T = ring["rew"][i, idx] + KW["gamma"] * L["crt"][i](*xin(i, nobs, nact)) * (1 - ring["done"][i, idx])
                loss = F.mse_loss(L["cr"][i](*xin(i, obs, list(act))), T)
                L["copt"][i].zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(L["cr"][i].parameters(), 0.5)
                L["copt"][i].step()
                a2 = list(act)
                a2[i] = L["ac"][i](obs[i])
                aloss = -L["cr"][i](*xin(i, obs, a2)).mean()
                L["aopt"][i].zero_grad()
                aloss.backward()
                torch.nn.utils.clip_grad_norm_(L["ac"][i].parameters(), 0.5)
                L["aopt"][i].step()
            with torch.no_grad():
                for tgt, src in zip(L["act"] + L["crt"], L["ac"] + L["cr"]):
                    for tp, sp in zip(tgt.parameters(), src.parameters()):
                        tp.mul_(1 - KW["tau"]).add_(sp, alpha=KW["tau"])
    # (a population is P sequential eager updates: fewer timed calls there, 2 blocks of 1)
    us = _time(learn, torch.cuda.synchronize) if P == 1 else _time(learn, torch.cuda.synchronize, 1, 1, 2)
    return dict(side="torch_eager", P=P, agents=NA, obs=O, act=A, hidden=H, batch=B, learn_us=round(us, 1), updates_per_s=round(P / us * 1e6, 1))


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    for P in ps:
        att, plain = bench_engine(P, True), bench_engine(P, False)
        print(json.dumps(att), flush=True)
        print(json.dumps(plain), flush=True)
        if with_torch:
            print(json.dumps(bench_torch(P)), flush=True)
        print(json.dumps(dict(side="ratio", P=P, time_att_over_plain=round(att["learn_us"] / plain["learn_us"], 2),
                              critic_macs_att_over_plain=round(MACS_ATT / MACS_PLAIN, 2))), flush=True)


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
