"""CPU: the NumPy restatement of CEM_GD3PG.learn (tests/cem_gd3pg_oracle.py) in float64 against torch autograd in double, at 1e-10:
losses, KL, the three pre-clip gradient norms, every parameter of the six trained / tracked nets and Adam's moments after three calls;
and what the oracle's switches and its draw do."""
import numpy as np
import pytest
import torch

from tests import cem_gd3pg_oracle as co

TOL = 1e-10


class _Net(torch.nn.Module):
    def __init__(self, p, hidden_act):
        super().__init__()
        for n in co.NAMES:
            w = p[n + ".weight"]
            lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
            lin.weight.data = torch.tensor(np.asarray(w, np.float64))
            lin.bias.data = torch.tensor(np.asarray(p[n + ".bias"], np.float64))
            setattr(self, n, lin)
        self.act = hidden_act

    def forward(self, x):
        return self.l3(self.act(self.l2(self.act(self.l1(x)))))


def _torch_learn(inp, c, calls):
    """CEM_GD3PG.py:180-231 on torch modules in double, the rows injected"""
    leaky = torch.nn.functional.leaky_relu
    actor = [_Net(inp["actor_1"], torch.tanh), _Net(inp["actor_2"], torch.tanh)]
    actor_t = [_Net(inp["actor_1_target"], torch.tanh), _Net(inp["actor_2_target"], torch.tanh)]
    critic, critic_t = _Net(inp["critic"], leaky), _Net(inp["critic_target"], leaky)
    domain = _Net(inp["actor_domain"], torch.tanh)
    pi = lambda net, s: torch.tanh(net(s))
    q = lambda net, s, a: net(torch.cat([s, a], 1))
    opts = [torch.optim.Adam(a.parameters(), lr=c["actor_lr"]) for a in actor] + [torch.optim.Adam(critic.parameters(), lr=c["critic_lr"])]
    o = co.CemGd3pg(inp, c, np.float64)          # (only for its rings)
    res = []
    for k in range(calls):
        idx = inp["idx"][k]
        cat = lambda key: torch.tensor(np.concatenate([o.ring[0][key][idx[0]], o.ring[1][key][idx[1]]]))
        obs, act, nobs, rew, done = cat("obs"), cat("act"), cat("next_obs"), cat("rew")[:, None], cat("done")[:, None]
        tq = torch.min(q(critic_t, nobs, pi(actor_t[0], nobs)), q(critic_t, nobs, pi(actor_t[1], nobs)))
        target = rew + c["gamma"] * tq * (1 - done)
        closs = torch.nn.functional.mse_loss(q(critic, obs, act), target.detach())
        opts[2].zero_grad()
        closs.backward()
        cnorm = torch.nn.utils.clip_grad_norm_(critic.parameters(), 0.5)
        opts[2].step()
        q1, q2 = q(critic, obs, pi(actor[0], obs)).mean(), q(critic, obs, pi(actor[1], obs)).mean()
        g = 1 if c["f1_more"] else 0
        cd = pi(actor[g], obs) - pi(domain, obs)
        kl = torch.sqrt(torch.sum(cd * cd) / len(cd))
        losses = [-q1, -q2]
        losses[g] = losses[g] + co.LAMBDA * c["delta"] * kl
        norms = []
        for j in (0, 1):
            opts[j].zero_grad()
            losses[j].backward()
            norms.append(torch.nn.utils.clip_grad_norm_(actor[j].parameters(), 0.5))
            opts[j].step()
        with torch.no_grad():
            for tg, src in ((critic_t, critic), (actor_t[0], actor[0]), (actor_t[1], actor[1])):
                for a, b in zip(tg.parameters(), src.parameters()):
                    a.copy_(a * (1.0 - c["tau"]) + b * c["tau"])
        res.append([closs.item(), float(cnorm), losses[0].item(), float(norms[0]), losses[1].item(), float(norms[1]), kl.item(), float(len(obs))])
    nets = dict(actor_1=actor[0], actor_2=actor[1], critic=critic, actor_1_target=actor_t[0], actor_2_target=actor_t[1], critic_target=critic_t)
    return np.array(res), nets, opts


@pytest.mark.parametrize("name", list(co.CASES))
def test_float64_oracle_matches_autograd(name):
    c = co.case(name)
    inp = co.inputs(c)
    o, got = co.run(c, inp, dtype=np.float64)
    want, nets, opts = _torch_learn(inp, c, c["n_learn"])
    np.testing.assert_allclose(got, want, rtol=TOL, atol=TOL)
    mine = dict(actor_1=o.actor[0], actor_2=o.actor[1], critic=o.critic, actor_1_target=o.actor_t[0], actor_2_target=o.actor_t[1], critic_target=o.critic_t)
    for key, net in nets.items():
        for k, v in net.state_dict().items():
            np.testing.assert_allclose(mine[key][k], v.numpy(), rtol=TOL, atol=TOL, err_msg="%s/%s" % (key, k))
    for opt, mo, net in ((opts[0], o.aopt[0], nets["actor_1"]), (opts[1], o.aopt[1], nets["actor_2"]), (opts[2], o.copt, nets["critic"])):
        for k, p in net.named_parameters():
            np.testing.assert_allclose(mo.m[k], opt.state[p]["exp_avg"].numpy(), rtol=TOL, atol=TOL, err_msg="m " + k)
            np.testing.assert_allclose(mo.v[k], opt.state[p]["exp_avg_sq"].numpy(), rtol=TOL, atol=1e-14, err_msg="v " + k)
        assert mo.t == c["n_learn"]
    assert got[0, 7] == 2 * (min(c["n1"], c["batch"]) // 2)


def test_float32_oracle_is_close_to_float64():
    c = co.case("odd")
    inp = co.inputs(c)
    _, a = co.run(c, inp, dtype=np.float32)
    _, b = co.run(c, inp, dtype=np.float64)
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)


def test_zero_c2_takes_no_penalty_gradient():
    """actor_domain == the guided actor: KL is 0, every number is finite, and the step equals the same step at delta = 0."""
    c = co.case("pend")
    inp = co.inputs(c)
    inp["actor_domain"] = {k: v.copy() for k, v in inp["actor_2"].items()}       # f1_more: actor_2 is the guided one
    o1, r1 = co.run(c, inp, n_learn=1)
    o0, r0 = co.run(dict(c, delta=0.0), inp, n_learn=1)
    assert r1[0, 6] == 0.0 and np.all(np.isfinite(r1))
    np.testing.assert_array_equal(r1, r0)
    for j in (0, 1):
        for k in o1.actor[j]:
            assert np.all(np.isfinite(o1.actor[j][k])) and np.array_equal(o1.actor[j][k], o0.actor[j][k])


def test_draw_consumes_numpy_like_sample():
    """two choice() calls, both below len(buffer_domain); the bound_buffer switch takes the first from len(buffer)"""
    c = co.case("short")
    inp = co.inputs(c)
    o = co.CemGd3pg(inp, c)
    np.random.seed(5)
    i0, i1 = o.draw(c["batch"])
    np.random.seed(5)
    w0, w1 = np.random.choice(c["n1"], 15, replace=False), np.random.choice(c["n1"], 15, replace=False)
    assert np.array_equal(i0, w0) and np.array_equal(i1, w1) and i0.max() >= c["n0"]       # ... reaching rows `buffer` never wrote
    np.random.seed(5)
    with pytest.raises(ValueError):          # 15 rows from the 12 that `buffer` holds
        co.CemGd3pg(inp, c, switches=("bound_buffer",)).draw(c["batch"])
