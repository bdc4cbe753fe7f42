"""Time of GAIL's discriminator update (kernels_gail.hip) at the reference script's shape:

  2048 expert + 2048 policy rows per call (config.py: horizon 2048), 3 + 1 input columns, hidden 128

Per population P: `frl_gail_learn` without and with the gradient penalty (expert rows drawn on the device, the policy rows uploaded
by every call, as a training loop would) and `frl_gail_reward` on 2048 rows; warm-up, then timed blocks of calls with one
synchronisation per block, the timing tools/envelope_bench.py uses.  Beside them the same update written with torch on the same
device, eager — the restatement of `GAIL.trian_D` (GAIL_file/GAIL.py:75-120), P learners one after the other, rows already on the
device — timed the same way.  Prints one JSON line per (P, what).
    python tools/gail_bench.py [--no-torch] [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

O, A, H, E, NP, TABLE = 3, 1, 128, 2048, 2048, 8192
WARM, BLOCK, BLOCKS = 5, 50, 4            # 4 blocks of 50 = 200 timed calls per point
LR = 4e-4


def _engine(P):
    e = Engine(N.ALGO_GAIL, O, A, TABLE, n_learners=P, hidden=H, hidden_act=N.ACT_LEAKY_RELU, batch_max=max(E, NP))
    g = np.random.default_rng(1)
    for p in range(P):
        e.set_params(0, (g.standard_normal(e.num_params(0)) * 0.05).astype(np.float32), learner=p)
    e.fill_synthetic(TABLE, seed=3)
    return e


def _timed(sync, fn):
    def block(n):
        sync()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        sync()
        return time.perf_counter() - t0
    block(WARM)
    return 1e6 * sum(block(BLOCK) for _ in range(BLOCKS)) / (BLOCKS * BLOCK)


def hip_points(P):
    e = _engine(P)
    rows = (0.8 * np.random.default_rng(2).standard_normal((P, NP, O + A))).astype(np.float32)
    out = {}
    for gp, betas in ((0, (0.9, 0.999)), (1, (0.5, 0.9))):
        kw = dict(gp=gp, lr=LR, beta1=betas[0], beta2=betas[1], n_expert=E)
        us = _timed(e.sync, lambda: e.gail_learn(rows, want_out=False, **kw))
        res = e.gail_learn(rows, **kw)["out"]
        out["learn_gp" if gp else "learn_bce"] = (us, bool(np.all(np.isfinite(res))))
    us = _timed(e.sync, lambda: e.gail_reward(rows, gp=1))
    out["reward_gp"] = (us, bool(np.all(np.isfinite(e.gail_reward(rows, gp=1)))))
    lds = e.lds_bytes()
    e.close()
    return out, lds


def torch_points(P):
    import torch
    import torch.nn.functional as F
    dev = torch.device("cuda")
    torch.manual_seed(0)
    nets = [torch.nn.Sequential(torch.nn.Linear(O + A, H), torch.nn.LeakyReLU(), torch.nn.Linear(H, H), torch.nn.LeakyReLU(),
                                torch.nn.Linear(H, 1)).to(dev) for _ in range(P)]
    xe = torch.rand(P, E, O + A, device=dev) * 2 - 1
    xp = torch.randn(P, NP, O + A, device=dev) * 0.8
    out = {}

    def step(net, opt, p, gp):
        le, lp = net(xe[p]), net(xp[p])
        if gp:
            loss = 0.5 * (F.binary_cross_entropy_with_logits(le, torch.ones_like(le)) + F.binary_cross_entropy_with_logits(lp, torch.zeros_like(lp)))
            xd = xe[p].clone().requires_grad_(True)
            od = net(xd)
            g = torch.autograd.grad(od, xd, grad_outputs=torch.ones_like(od), create_graph=True, retain_graph=True, only_inputs=True)[0]
            loss = loss + 5 * torch.mean(torch.sum(torch.square(g), dim=-1))
        else:
            pe, pp = torch.sigmoid(le), torch.sigmoid(lp)
            loss = F.binary_cross_entropy(pe, torch.ones_like(pe)) + F.binary_cross_entropy(pp, torch.zeros_like(pp))
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for gp, betas in ((0, (0.9, 0.999)), (1, (0.5, 0.9))):
        opts = [torch.optim.Adam(n.parameters(), lr=LR, betas=betas) for n in nets]

        def call():
            for p in range(P):
                step(nets[p], opts[p], p, gp)
        us = _timed(torch.cuda.synchronize, call)
        out["learn_gp" if gp else "learn_bce"] = (us, bool(torch.isfinite(step(nets[0], opts[0], 0, gp)).item()))

    def reward():
        with torch.no_grad():
            for p in range(P):
                prob = 1 / (1 + torch.exp(-nets[p](xp[p])))
                r = -torch.log(torch.maximum(1 - prob, torch.tensor(0.0001, device=dev))) * 2
        return r
    us = _timed(torch.cuda.synchronize, reward)
    out["reward_gp"] = (us, bool(torch.isfinite(reward()).all().item()))
    return out


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    for P in ps:
        hip, lds = hip_points(P)
        sides = [("hip", hip)] + ([("torch_eager", torch_points(P))] if with_torch else [])
        for side, pts in sides:
            for what, (us, finite) in pts.items():
                print(json.dumps(dict(algo="gail", side=side, what=what, P=P, obs=O, act=A, hidden=H, n_expert=E, n_policy=NP,
                                      calls=BLOCKS * BLOCK, call_us=round(us, 1), updates_per_s=round(P / us * 1e6, 1), finite=finite,
                                      lds_rc=lds if side == "hip" else None)), flush=True)


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
