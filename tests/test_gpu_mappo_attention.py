"""GPU: MAPPO_attention (freerl_amd.MAPPO_attention, kernels_mappo_att.hip) against tests/mappo_attention_oracle.py, float64 on the CPU:
per-step losses, pre-clip gradient norms, every parameter and Adam's first moments after 1 and 3 learn() calls.

Tolerances are the project's, unwidened (tests/mappo_oracle.py: assert_net, assert_m; losses rtol 1e-4 / atol 1e-6; norms rtol 1e-3;
parameters 5e-4 / 5e-6) for `pair`, `octet` and `trio`'s first call.  `trio`'s later calls (critic lr 3e-3, a sharp softmax) amplify
rounding: the oracle's own float32 run is then 2.44e-4 off its float64 run in a loss, 1.32 % in a critic norm, 2.9e-3 in a critic or
block parameter and 1.15e-5 in an actor parameter, and those bounds are 4 x that (TRIO_LATER; DESIGN.md "MAPPO_attention")."""
import numpy as np
import pytest
import torch

from tests import mappo_attention_oracle as A
from tests import mappo_oracle as M

pytestmark = pytest.mark.gpu
CALLS = 3
PLAIN = dict(loss_atol=1e-6, norm_rtol=1e-3, actor_atol=5e-6, critic_atol=5e-6)
TRIO_LATER = dict(loss_atol=9.8e-4, norm_rtol=5.3e-2, actor_atol=4.6e-5, critic_atol=1.16e-2)      # 4 x the oracle's float32-to-float64 gap


def _engine(c, inps):
    """an engine with a learner per entry of `inps` (one learner: the Python class's own engine), its nets set from them"""
    from freerl_amd import _native as N
    from freerl_amd.engine import Engine
    from freerl_amd.MAPPO_attention import MAPPO, pack_attention
    od, ad, n = [d[0] for d in c["dims"]], [d[1] for d in c["dims"]], len(c["dims"])
    if len(inps) == 1:
        e = MAPPO({"agent_%d" % i: list(d) for i, d in enumerate(c["dims"])}, c["cont"], c["actor_lr"], c["critic_lr"], c["horizon"], "cpu",
                  trick=dict(c["trick"], orthogonal_init=False), improment={"attention": True}, minibatch_max=c["minibatch"])._e
    else:
        e = Engine(N.ALGO_MAPPO_ATT, od, ad, c["horizon"], n_learners=len(inps), hidden=128, batch_max=c["minibatch"],
                   extra_cols=(sum(ad) if c["cont"] else n) + n, discrete=not c["cont"])
        e.net_norm_set(c["trick"]["feature_norm"], c["trick"]["LayerNorm"])
    for p, inp in enumerate(inps):
        att = pack_attention(inp["attention"])
        for i in range(len(c["dims"])):
            e.set_params(2 * i, M.flat(c, "actor", inp["actors"][i]), learner=p)
            e.set_params(2 * i + 1, np.concatenate([np.concatenate([v.reshape(-1) for v in inp["critics"][i].values()]), att]), learner=p)
    return e, N


def _fill(e, c, inps):
    lay, stored = e.layout, sum(d[1] for d in c["dims"]) if c["cont"] else len(c["dims"])
    for p, inp in enumerate(inps):
        rec = np.zeros((c["horizon"], e.width), np.float32)
        lp = lay.extra_off
        for j, r in enumerate(inp["rows"]):
            rec[:, lay.obs_off[j]:lay.obs_off[j] + lay.obs_dim[j]] = r["obs"]
            rec[:, lay.act_off[j]:lay.act_off[j] + lay.act_dim[j]] = r["act"]
            rec[:, lay.rew_off + j], rec[:, lay.done_off + j] = r["rew"][:, 0], r["done"][:, 0]
            rec[:, lay.next_obs_off[j]:lay.next_obs_off[j] + lay.obs_dim[j]] = r["next_obs"]
            rec[:, lp:lp + lay.act_dim[j]] = r["logp"]
            lp += lay.act_dim[j]
            rec[:, lay.extra_off + stored + j] = r["adv_done"][:, 0]
        e.set_cursor(p, 0, 0)
        for t in range(c["horizon"]):
            e.add(p, rec[t])


def _learn(e, c, perms):
    return e.mappo_att_learn(c["horizon"], c["minibatch"], c["k_epochs"], gamma=c["gamma"], lmbda=c["lmbda"], clip=c["clip"], ent_coef=c["ent_coef"],
                                  adv_norm=c["trick"]["adv_norm"], value_clip=c["trick"]["ValueClip"], huber_delta=c["huber_delta"] if c["trick"]["huber_loss"] else None,
                                  perms=np.stack(perms), want_trace=True, want_norms=True, actor_lr=c["actor_lr"], critic_lr=c["critic_lr"],
                                  adam_eps=1e-5 if c["trick"]["adam_eps"] else 1e-8, clip_norm=0.5)


def _state(e, N, n, p):
    return [(e.get_params(k, learner=p), e.get_params(k, N.PARAM_ADAM_M, learner=p)) for k in range(2 * n)]


@pytest.mark.parametrize("name,P", [("pair", 1), ("trio", 1), ("octet", 1), ("trio", 2)])
def test_learn_matches_float64_oracle(name, P):
    from freerl_amd.MAPPO_attention import pack_attention, unpack_attention
    c = A.case(name)
    n, steps = len(c["dims"]), c["k_epochs"] * -(-c["horizon"] // c["minibatch"])
    inps = [A.inputs(c, c["seed"] + 100 * p) for p in range(P)]
    oracles = [A.Oracle(c, inp) for inp in inps]
    pol, N = _engine(c, inps)
    solo = [_engine(c, [inp]) for inp in inps] if P > 1 else []
    for call in range(CALLS):
        perms = [M.perms(c, c["seed"] + 100 * p + call) for p in range(P)]
        _fill(pol, c, inps)
        out = _learn(pol, c, perms)
        for p, o in enumerate(oracles):
            losses, norms = o.learn(perms[p])
            tol = TRIO_LATER if name == "trio" and call > 0 else PLAIN
            if name == "trio" and call == 0 and p == 0:         # the case's conditions, on the oracle
                g = norms[:, :, 1]
                assert (g < 0.5).any() and (g > 0.5).any(), g
                w = torch.cat(o.weights[:n])
                assert float(((w.max(1).values - w.min(1).values) >= 0.05).float().mean()) >= 0.10
                ind = A.Oracle(c, inps[0])
                ind.learn(perms[0], independent=True)          # every agent from the pre-call block: must be visibly different
                a, b = o.flat(o.critics[n - 1]), ind.flat(ind.critics[n - 1])
                assert (np.abs(a - b) > 10 * (5e-6 + 5e-4 * np.abs(a))).mean() > 0.25
            np.testing.assert_allclose(out["trace"][p], losses, rtol=1e-4, atol=tol["loss_atol"])
            np.testing.assert_allclose(out["norms"][p], norms[:, :, 1], rtol=tol["norm_rtol"])
            if call not in (0, CALLS - 1):
                continue
            st, own = _state(pol, N, n, p), o.flat(o.critics[0]).size
            block = pack_attention({k: v.detach() for k, v in o.att.items()})
            M.assert_net(st[1][0][own:], block, c["critic_lr"], steps * n * (call + 1), "attention block", atol=tol["critic_atol"])
            for i in range(n):
                M.assert_net(st[2 * i][0], o.flat(o.actors[i]), c["actor_lr"], steps * (call + 1), "actor %d" % i, atol=tol["actor_atol"])
                M.assert_net(st[2 * i + 1][0][:own], o.flat(o.critics[i]), c["critic_lr"], steps * (call + 1), "critic %d" % i, atol=tol["critic_atol"])
                M.assert_m(st[2 * i][1], o.adam_m(o.aopt[i]), "actor %d" % i)
                m = o.adam_m(o.copt[i])
                M.assert_m(st[2 * i + 1][1][:own], m[:own], "critic %d" % i)
                got = unpack_attention(st[2 * i + 1][1][own:])
                M.assert_m(np.concatenate([got[k].reshape(-1) for k in A.ATT]), m[own:], "critic %d's moments of the block" % i)
                assert pol.opt_step(2 * i + 1, learner=p) == steps * (call + 1)          # Adam counts every step
                if name == "pair" and call == 0:                # one other: p is exactly 1, so query and key get exactly zero gradient
                    for k in A.ATT[:2]:
                        assert not got[k].any(), k
        for p, (sp, _) in enumerate(solo):                      # two learners in one engine = two one-learner engines, bit for bit
            _fill(sp, c, [inps[p]])
            so = _learn(sp, c, [perms[p]])
            assert np.array_equal(so["trace"][0], out["trace"][p]) and np.array_equal(so["norms"][0], out["norms"][p])
            for (a, am), (b, bm) in zip(_state(sp, N, n, 0), _state(pol, N, n, p)):
                assert np.array_equal(a, b) and np.array_equal(am, bm)
