"""CPU: the NumPy restatement of MAAC (tests/maac_oracle.py) against torch autograd + clip_grad_norm_ + torch.optim.Adam in double on a
restatement of MAAC_discrete.py:208-280 / Attention.py:63-231 written here with torch modules' semantics: ONE attention block listed in all
n critic optimisers, zero_grad(set_to_none) before each backward, the gradients that agent i's losses leave in other critics' tensors
never stepped.  Also: the float32 oracle against the float64 one as a share of the GPU test's tolerances, what the five switches move,
and the closed-form critic backward against autograd on its own."""
import numpy as np
import pytest
import torch

from tests import maac_oracle as mo

F64 = np.float64


def _tt(a, grad=True):
    return torch.tensor(np.asarray(a, F64), dtype=torch.float64, requires_grad=grad)


def _leaky(x):
    return torch.nn.functional.leaky_relu(x)


def _actor(p, x, eps):
    h = _leaky(x @ p["l1.weight"].T + p["l1.bias"])
    h = _leaky(h @ p["l2.weight"].T + p["l2.bias"])
    z = h @ p["l3.weight"].T + p["l3.bias"]
    probs = torch.softmax(z, dim=1)
    cat = torch.distributions.Categorical(probs)
    k = torch.argmax(cat.probs / eps, dim=1)                 # torch.multinomial(probs, 1) with its exponential draw injected
    logp = torch.log_softmax(z, dim=1).gather(1, k.reshape(-1, 1))
    return k, logp, probs, torch.nn.functional.one_hot(k, num_classes=z.shape[1]).double()


def _critic(own_i, att, own_all, i, obs, act):
    """Attention_Critic.forward + Attention.forward, literally: reshape / permute / matmul over the other agents"""
    s = _leaky(obs[i] @ own_i["encoder_fc_s.weight"].T + own_i["encoder_fc_s.bias"])
    e_q = s.unsqueeze(1)
    e_k = []
    for j in range(len(obs)):
        if j != i:
            sa = torch.cat((obs[j], act[j]), 1)
            e_k.append(_leaky(sa @ own_all[j]["encoder_fc_sa.weight"].T + own_all[j]["encoder_fc_sa.bias"]).unsqueeze(1))
    e_k = torch.cat(e_k, dim=1)
    Q = e_q @ att["attention.query.weight"].T
    K = e_k @ att["attention.key.weight"].T
    V = _leaky(e_k @ att["attention.value.0.weight"].T + att["attention.value.0.bias"])
    nh, hd = mo.HEADS, Q.shape[-1] // mo.HEADS
    Q = Q.reshape(Q.shape[0], Q.shape[1], nh, hd).permute(2, 0, 1, 3)
    K = K.reshape(K.shape[0], K.shape[1], nh, hd).permute(2, 0, 1, 3)
    V = V.reshape(V.shape[0], V.shape[1], nh, hd).permute(2, 0, 1, 3)
    scores = torch.matmul(Q, K.permute(0, 1, 3, 2)) / np.sqrt(hd)
    w = torch.softmax(scores, dim=-1)
    av = torch.matmul(w, V).permute(1, 2, 0, 3)
    av = av.reshape(av.shape[0], av.shape[1], -1)
    other = av.squeeze(1) @ att["attention.fc_out.weight"].T + att["attention.fc_out.bias"]
    x = _leaky(torch.cat([s, other], dim=1) @ own_i["fc1.weight"].T + own_i["fc1.bias"])
    all_q = x @ own_i["fc2.weight"].T + own_i["fc2.bias"]
    return all_q.gather(1, torch.argmax(act[i], dim=1, keepdim=True)), all_q


class TorchMAAC:
    def __init__(self, c, inp):
        n = len(c["dims"])
        self.n, self.c = n, c
        self.att = {k: _tt(v) for k, v in inp["att"].items()}
        self.own = [{k: _tt(v) for k, v in inp["own"][j].items()} for j in range(n)]
        self.actor = [{k: _tt(v) for k, v in inp["actor"][j].items()} for j in range(n)]
        self.att_t = [{k: _tt(v, False) for k, v in inp["att"].items()} for _ in range(n)]
        self.own_t = [{k: _tt(v, False) for k, v in inp["own"][j].items()} for j in range(n)]
        self.actor_t = [{k: _tt(v, False) for k, v in inp["actor"][j].items()} for j in range(n)]
        # critic.parameters(): the attention module first, then the critic's own layers — the SAME attention tensors in every optimiser
        self.cparams = [[self.att[k] for k in mo.ATT_KEYS] + [self.own[j][k] for k in mo.CRITIC_KEYS[6:]] for j in range(n)]
        self.copt = [torch.optim.Adam(self.cparams[j], lr=c["critic_lr"]) for j in range(n)]
        self.aparams = [list(self.actor[j].values()) for j in range(n)]
        self.aopt = [torch.optim.Adam(self.aparams[j], lr=c["actor_lr"]) for j in range(n)]
        t = inp["table"]
        self.tab = [{k: torch.tensor(np.asarray(x[k], F64)) for k in ("obs", "act", "next_obs", "rew", "done")} for x in t]

    def learn(self, idx, eps, gamma, tau):
        n, out = self.n, dict(critic_loss=[], actor_loss=[], critic_norm=[], actor_norm=[])
        alpha = self.c["alpha"]
        for i in range(n):
            rows = torch.as_tensor(np.asarray(idx[i], np.int64))
            e = [torch.tensor(np.asarray(x, F64)) for x in eps[i]]
            obs, act, nobs = [t["obs"][rows] for t in self.tab], [t["act"][rows] for t in self.tab], [t["next_obs"][rows] for t in self.tab]
            nxt = [_actor(self.actor_t[j], nobs[j], e[j]) for j in range(n)]
            qn, _ = _critic(self.own_t[i], self.att_t[i], self.own, i, nobs, [x[3] for x in nxt])
            T = self.tab[i]["rew"][rows][:, None] + gamma * (1 - self.tab[i]["done"][rows][:, None]) * (qn + alpha * -nxt[i][1])
            q, _ = _critic(self.own[i], self.att, self.own, i, obs, act)
            loss = torch.nn.functional.mse_loss(q, T.detach())
            self.copt[i].zero_grad()
            loss.backward()
            out["critic_norm"].append(float(torch.nn.utils.clip_grad_norm_(self.cparams[i], 0.5)))
            self.copt[i].step()
            out["critic_loss"].append(float(loss.detach()))
            new = [_actor(self.actor[j], obs[j], e[n + j]) for j in range(n)]
            _, lp, probs, _ = _actor(self.actor[i], obs[i], e[2 * n])
            q_pi, all_q = _critic(self.own[i], self.att, self.own, i, obs, [x[3] for x in new])
            v = (all_q * probs).sum(dim=1, keepdim=True)
            aloss = (lp * (-(q_pi - v) - alpha * -lp)).mean()
            self.aopt[i].zero_grad()
            aloss.backward()
            out["actor_norm"].append(float(torch.nn.utils.clip_grad_norm_(self.aparams[i], 0.5)))
            self.aopt[i].step()
            out["actor_loss"].append(float(aloss.detach()))
        with torch.no_grad():
            for i in range(n):
                for tgt, src in ((self.actor_t[i], self.actor[i]), (self.own_t[i], self.own[i]), (self.att_t[i], self.att)):
                    for k in tgt:
                        tgt[k].copy_(tgt[k] * (1.0 - tau) + src[k] * tau)
        return out


def _n(t):
    return t.detach().numpy()


@pytest.mark.parametrize("name", ["pair", "hetero", "eight", "wide17"])
def test_oracle_against_torch_in_double(name):
    c = mo.case(name)
    inp = mo.inputs(c)
    o, t = mo.make(c, inp, F64), TorchMAAC(c, inp)
    n = len(c["dims"])
    frozen0 = [{k: _n(t.own[j][k]).copy() for k in mo.FROZEN_KEYS} for j in range(n)]
    for call in range(c["n_learn"]):
        a, b = o.learn_with(inp["idx"][call], inp["eps"][call], c["gamma"], c["tau"]), t.learn(inp["idx"][call], inp["eps"][call], c["gamma"], c["tau"])
        for key in ("critic_loss", "actor_loss", "critic_norm", "actor_norm"):
            np.testing.assert_allclose(np.array(a[key], F64), b[key], rtol=1e-10, atol=1e-12, err_msg="%s call %d %s" % (name, call, key))
    for j in range(n):
        for k in mo.ACTOR_NAMES:
            for suf in (".weight", ".bias"):
                np.testing.assert_allclose(o.actor[j][k + suf], _n(t.actor[j][k + suf]), rtol=1e-10, atol=1e-12)
                np.testing.assert_allclose(o.actor_t[j][k + suf], _n(t.actor_t[j][k + suf]), rtol=1e-10, atol=1e-12)
        on, tg = o.critic(j), o.critic(j, target=True)
        tsd = dict(t.att)
        tsd.update(t.own[j])
        ttg = dict(t.att_t[j])
        ttg.update(t.own_t[j])
        for k in mo.CRITIC_KEYS:
            np.testing.assert_allclose(on[k], _n(tsd[k]), rtol=1e-10, atol=1e-12, err_msg="%s agent %d %s" % (name, j, k))
            np.testing.assert_allclose(tg[k], _n(ttg[k]), rtol=1e-10, atol=1e-12, err_msg="%s agent %d target %s" % (name, j, k))
        # n optimisers on one block: each has its own moments and step count for it; the 8 frozen tensors have no Adam state at all
        st = t.copt[j].state
        assert len(st) == len(mo.TRAINED_KEYS)
        for k in mo.TRAINED_KEYS:
            s = st[tsd[k]]
            assert int(s["step"]) == c["n_learn"] == o.copt[j].t
            np.testing.assert_allclose(o.copt[j].m[k], _n(s["exp_avg"]), rtol=1e-9, atol=1e-14, err_msg="%s agent %d m %s" % (name, j, k))
        for k in mo.FROZEN_KEYS:
            assert tsd[k] not in st
            assert np.array_equal(_n(t.own[j][k]), frozen0[j][k]) and np.array_equal(o.own[j][k], frozen0[j][k])
            # (the soft update of an unchanged tensor, x (1 - tau) + x tau, is a no-op up to rounding: the TARGET copies may move by an ulp)
            np.testing.assert_allclose(o.own_t[j][k], frozen0[j][k], rtol=1e-14)
    if n > 2:       # the n moment sets of the shared block differ: each agent's loss gave it another gradient
        assert not np.allclose(o.copt[0].m["attention.query.weight"], o.copt[1].m["attention.query.weight"])


def test_critic_backward_against_autograd():
    c = mo.case("hetero")
    inp = mo.inputs(c)
    o, t = mo.make(c, inp, F64), TorchMAAC(c, inp)
    rows = np.arange(23)
    obs, act = [x[rows] for x in o.obs], [x[rows] for x in o.act]
    g = np.random.default_rng(3).standard_normal((23, c["dims"][1][1]))
    aq, k = o.all_q(1, obs, act)
    grads = mo.critic_backward(o.own[1], o.att[1], k, g)
    _, taq = _critic(t.own[1], t.att, t.own, 1, [torch.tensor(x) for x in obs], [torch.tensor(x) for x in act])
    np.testing.assert_allclose(aq, _n(taq), rtol=1e-12, atol=1e-13)
    (taq * torch.tensor(g)).sum().backward()
    tsd = dict(t.att)
    tsd.update(t.own[1])
    for kk in mo.TRAINED_KEYS:
        np.testing.assert_allclose(grads[kk], _n(tsd[kk].grad), rtol=1e-9, atol=1e-12, err_msg=kk)
    for kk in mo.FROZEN_KEYS:
        assert t.own[1][kk].grad is None
    assert t.own[0]["encoder_fc_sa.weight"].grad is not None      # what agent 1's loss leaves in agent 0's encoder (never stepped)


_gaps = mo.gaps


@pytest.mark.parametrize("name", list(mo.CASES))
def test_float32_against_float64(name):
    """the float32 oracle stays within a quarter of every tolerance of the GPU test: the tolerances are the project's, unwidened"""
    gap = _gaps(name)
    print("%s: float32 oracle against float64, as shares of the tolerances: %s" % (name, {k: round(v, 4) for k, v in gap.items()}))
    assert max(gap.values()) <= 0.25, gap


def test_switches_move_what_is_compared():
    """every other reading of the reference moves some compared quantity by >= 10 x the GPU test's tolerance in at least one case"""
    for sw in ("own_attention", "final_attention", "one_draw", "stale_actors", "detach_probs"):
        best = 0.0
        for name in ("hetero", "spread3", "eight"):
            best = max(best, max(_gaps(name, F64, **{sw: True}).values()))
        print("%s moves a compared quantity by %.3g x its tolerance" % (sw, best))
        assert best >= 10, (sw, best)


def test_case_conditions():
    """what the cases are for: critic pre-clip norms on both sides of 0.5, both done values, every action stored and drawn, draw 1 != draw 2
    on >= 25 % of each agent's rows, attention weights that differ by >= 0.05 on >= 10 % of the rows where there are two others"""
    for name in ("pair", "hetero", "spread3", "spread5"):
        c = mo.case(name)
        inp = mo.inputs(c)
        o = mo.make(c, inp, F64)
        outs = [o.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"]) for k in range(c["n_learn"])]
        cn = np.array([x["critic_norm"] for x in outs])
        assert (cn > 0.5).any() and (cn < 0.5).any(), (name, cn)
        for j, t in enumerate(inp["table"]):
            assert 0 < t["done"].mean() < 1 and (t["act"].sum(axis=0) > 0).all(), name
        dd = np.array([x["draws_differ"] for x in outs]).mean(axis=0)
        assert (dd >= 0.25).all(), (name, dd)
        if len(c["dims"]) > 2:
            sp = np.array([x["att_spread"] for x in outs]).mean(axis=0)
            assert (sp >= 0.10).all(), (name, sp)
