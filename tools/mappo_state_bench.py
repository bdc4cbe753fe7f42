"""Time of one `learn()` of MAPPO with a global-state critic (kernels_mappo_state.hip) against the action-masked one without a state
(kernels_mappo_mask.hip) on the same discrete shape, from the same build, in one command:

  3 agents x (80 obs, 9 actions), hidden 128, horizon 256 in one minibatch of 256, K_epochs 15, every trick on; state_dim 120

tools/mappo_mask_bench.py's STAND-IN shape plus a stand-in state width: SMACv2's own dimensions come from the environment and cannot
be read without it.  A critic's first layer is 360 columns wide instead of 240.  Per population P, two engines hold the same rows and
parameters (the state engine's critics have 120 more input columns); both run `frl_mappo_learn` with device-drawn permutations and the
class's settings (two Adams, eps 1e-5, clip_norm 0.5).  The two sides run ALTERNATELY, block by block; a block is a few calls between
two synchronisations (host clock), after a warm-up call of each side.  Then the same update of ONE learner in eager PyTorch on the same
device (the reference's arithmetic: value pass, GAE on the host, K epochs of one actor and one critic step per agent), for scale.
Prints one JSON line per (P, side), one with the ratio, and one for eager torch.
    python tools/mappo_state_bench.py [--no-torch] [P ...]      (default P = 1 64)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from freerl_amd import _native as N  # noqa: E402
from freerl_amd.engine import Engine  # noqa: E402

NA, O, A, H, T, K, SD = 3, 80, 9, 128, 256, 15, 120
HYPER = dict(gamma=0.95, lmbda=0.95, clip=0.2, ent_coef=0.01, actor_lr=1e-3, critic_lr=1e-3, adam_eps=1e-5, clip_norm=0.5, adv_norm=True,
             value_clip=True, huber_delta=10.0)
BLOCKS = 5


def _rows(P, seed):
    g = np.random.default_rng(seed)
    obs = g.standard_normal((P, T, NA, O)).astype(np.float32)
    act = g.integers(0, A, (P, T, NA, 1))
    mask = g.random((P, T, NA, A)) < 0.5
    np.put_along_axis(mask, act, True, axis=3)
    return dict(obs=obs, nobs=(obs + 0.3 * g.standard_normal(obs.shape)).astype(np.float32), act=act.astype(np.float32),
                logp=np.log(g.uniform(0.15, 0.6, (P, T, NA, 1))).astype(np.float32), rew=g.standard_normal((P, T, NA)).astype(np.float32),
                done=np.zeros((P, T, NA), np.float32), adv_done=(np.arange(T) % 25 == 24).astype(np.float32)[None, :, None].repeat(P, 0).repeat(NA, 2),
                mask=mask.astype(np.float32), state=g.standard_normal((P, T, SD)).astype(np.float32))


def _engine(P, rows, state):
    sd = SD if state else 0
    e = Engine(N.ALGO_MAPPO, [O] * NA, [A] * NA, T, n_learners=P, discrete=True, hidden=H, batch_max=T, extra_cols=2 * NA + NA * A + sd, state_dim=sd)
    e.net_norm_set(True, True)
    e.action_mask_set(True)
    g = np.random.default_rng(1)
    for p in range(P):
        for net in range(e.n_nets):
            e.set_params(net, (g.standard_normal(e.num_params(net)) * 0.05).astype(np.float32), learner=p)
    f = lambda x: x.reshape(P * T, -1)
    cols = [f(rows["obs"]), f(rows["act"]), f(rows["rew"]), f(rows["done"]), f(rows["nobs"]), f(rows["logp"]), f(rows["adv_done"]), f(rows["mask"])]
    if state:
        cols.append(f(rows["state"]))
    e.add_batch(np.concatenate(cols, axis=1), learners=np.repeat(np.arange(P), T).astype(np.int32))
    e.flush()
    return e


def _block(e, n):
    e.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        e.mappo_learn(T, T, K, **HYPER)      # (the rows stay: learn() resets the counters only, and reads the whole capacity)
    e.sync()
    return time.perf_counter() - t0


def _torch_ms(rows, calls=3, device="cuda"):
    """the same update of learner 0 in eager PyTorch on the same device, the reference's way: -> ms per learn()"""
    import torch
    import torch.nn.functional as F
    dev = torch.device(device)
    t = lambda x: torch.as_tensor(x[0], device=dev)
    obs, nobs, act, logp, rew, done, mask, state = (t(rows[k]) for k in ("obs", "nobs", "act", "logp", "rew", "done", "mask", "state"))
    adv_done = rows["adv_done"][0]

    def mlp(i, o):
        return torch.nn.ModuleList([torch.nn.Linear(i, H), torch.nn.Linear(H, H), torch.nn.Linear(H, o)]).to(dev)

    def fwd(net, x):
        x = F.layer_norm(x, x.shape[1:])
        x = F.layer_norm(F.relu(net[0](x)), (H,))
        x = F.layer_norm(F.relu(net[1](x)), (H,))
        return net[2](x)
    actors, critics = [mlp(O, A) for _ in range(NA)], [mlp(NA * O + SD, 1) for _ in range(NA)]
    aopt = [torch.optim.Adam(a.parameters(), lr=1e-3, eps=1e-5) for a in actors]
    copt = [torch.optim.Adam(c.parameters(), lr=1e-3, eps=1e-5) for c in critics]
    flat, nflat = obs.reshape(T, -1), nobs.reshape(T, -1)

    def learn():
        with torch.no_grad():
            adv = np.zeros((T, NA), np.float32)
            vs_all = []
            for i in range(NA):
                vs = fwd(critics[i], torch.cat([flat, state], 1))
                vs_ = fwd(critics[i], torch.cat([nflat, state], 1))
                td = (rew[:, i:i + 1] + HYPER["gamma"] * (1 - done[:, i:i + 1]) * vs_ - vs).reshape(-1).cpu().numpy()
                a = 0.0
                for s in range(T - 1, -1, -1):
                    a = td[s] + HYPER["gamma"] * HYPER["lmbda"] * a * (1 - adv_done[s, i])
                    adv[s, i] = a
                vs_all.append(vs)
            advt = torch.as_tensor(adv, device=dev)
            v_target = advt + torch.cat(vs_all, 1)
            advt = (advt - advt.mean()) / (advt.std() + 1e-8)
        for i in range(NA):
            for _ in range(K):
                idx = torch.as_tensor(np.random.permutation(T), device=dev)
                logits = torch.where(mask[idx, i] > 0, fwd(actors[i], obs[idx, i]), torch.tensor(-1e8, device=dev))
                dist = torch.distributions.Categorical(logits=logits)
                ratio = torch.exp(dist.log_prob(act[idx, i, 0]).reshape(-1, 1) - logp[idx, i])
                surr = torch.min(ratio * advt[idx], torch.clamp(ratio, 0.8, 1.2) * advt[idx])
                p_log_p = torch.where(mask[idx, i] > 0, dist.logits * dist.probs, torch.tensor(0.0, device=dev))
                loss = -surr.mean() - HYPER["ent_coef"] * (-p_log_p.sum(-1)).mean()
                aopt[i].zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(actors[i].parameters(), 0.5)
                aopt[i].step()
                v = fwd(critics[i], torch.cat([flat[idx], state], 1)).repeat(1, NA)
                closs = F.huber_loss(v, v_target[idx], delta=HYPER["huber_delta"])
                copt[i].zero_grad()
                closs.backward()
                torch.nn.utils.clip_grad_norm_(critics[i].parameters(), 0.5)
                copt[i].step()
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    learn()
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        learn()
    sync()
    return 1e3 * (time.perf_counter() - t0) / calls


def main(ps, with_torch=True):
    if with_torch:                 # torch opens the device first: it finds none once the engine's library has loaded its HIP runtime
        import torch
        torch.cuda.init()
    for P in ps:
        rows = _rows(P, 2)
        sides = [("masked", _engine(P, rows, False)), ("state", _engine(P, rows, True))]
        n = 20 if P == 1 else 5
        total = {s: 0.0 for s, _ in sides}
        for _, e in sides:
            _block(e, 1)                                   # warm-up
        for _ in range(BLOCKS):                            # the two sides alternately
            for side, e in sides:
                total[side] += _block(e, n)
        ms = {}
        for side, e in sides:
            ms[side] = 1e3 * total[side] / (BLOCKS * n)
            finite = all(np.isfinite(e.get_params(net)).all() for net in range(e.n_nets))
            print(json.dumps(dict(algo="mappo", side=side, P=P, agents=NA, obs=O, act=A, state_dim=SD if side == "state" else 0, hidden=H, horizon=T,
                                  minibatch=T, k_epochs=K, critic_in=NA * O + (SD if side == "state" else 0),
                                  calls=BLOCKS * n, call_ms=round(ms[side], 3), finite=finite, lds_rc=e.lds_bytes())), flush=True)
            e.close()
        print(json.dumps(dict(P=P, state_over_masked=round(ms["state"] / ms["masked"], 4))), flush=True)
    if with_torch:
        print(json.dumps(dict(side="state_torch_eager", P=1, state_dim=SD, call_ms=round(_torch_ms(_rows(1, 2)), 1))), flush=True)


if __name__ == "__main__":
    argv = [x for x in sys.argv[1:] if x != "--no-torch"]
    main([int(x) for x in argv] or [1, 64], with_torch="--no-torch" not in sys.argv[1:])
