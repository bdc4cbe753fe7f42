"""CPU: the NumPy restatement of MASAC (tests/masac_oracle.py) against the reference's recorded outputs (tests/golden/masac.npz), float32
against float64, one whole learn() against torch autograd + torch.optim.Adam in double, and the three discrimination switches.

Tolerances are the project's (tests/test_gpu_envelope_ddpg.py: losses rtol 1e-4 / atol 1e-6, norms rtol 1e-3, parameters rtol 5e-4 /
atol 5e-6 on >= 99 % of a tensor's elements).  test_float32_against_float64 prints, per case, the float32 oracle's distance from the
float64 one as a share of each tolerance (DESIGN.md "MASAC" records them)."""
import os

import numpy as np
import pytest
import torch

from tests import masac_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masac.npz")
LOSS_TOL, NORM_RTOL, PARAM_TOL = (1e-4, 1e-6), 1e-3, (5e-4, 5e-6)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


_RUNS = {}


def run(name, dtype, upto=None):
    """the oracle through the calls of a case, once per (case, dtype, calls): (oracle, per-call outputs)"""
    c = mo.case(name)
    calls = upto or c["n_learn"]
    if (name, dtype, calls) not in _RUNS:
        inp = mo.inputs(c)
        o = mo.make(c, inp, dtype)
        _RUNS[(name, dtype, calls)] = (o, [o.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"]) for k in range(calls)])
    return _RUNS[(name, dtype, calls)]


def check_state(fx, pre, o, c, calls, tol):
    for j in range(len(c["dims"])):
        for key, got, names in (("actor", o.actor[j], mo.ACTOR_NAMES), ("critic", o.critic[j], mo.CRITIC_NAMES),
                                ("actor_target", o.actor_t[j], mo.ACTOR_NAMES), ("critic_target", o.critic_t[j], mo.CRITIC_NAMES)):
            p = "%s/%d/%s" % (pre, j, key)
            mo.check_digest(got, names, fx[p + "/stats"], fx[p + "/sample"], tol["param"][0], tol["param"][1], p)
        for key, opt, names in (("actor", o.aopt[j], mo.ACTOR_NAMES), ("critic", o.copt[j], mo.CRITIC_NAMES)):
            p = "%s/%d/%s_m" % (pre, j, key)
            scale = float(np.abs(fx[p + "/sample"]).max())
            mo.check_digest(opt.m, names, fx[p + "/stats"], fx[p + "/sample"], tol["m"], tol["m"] * scale, p)
            assert opt.t == int(fx["%s/%d/%s_step" % (pre, j, key)]) == calls
        la, m, v, alpha, step = fx["%s/%d/alpha_state" % (pre, j)]
        np.testing.assert_allclose(float(o.log_alpha[j]["log_alpha"]), la, rtol=1e-5, err_msg=pre + " log_alpha")
        np.testing.assert_allclose(float(o.alopt[j].m["log_alpha"]), m, rtol=tol["alpha_m"], atol=1e-9, err_msg=pre + " alpha exp_avg")
        np.testing.assert_allclose(float(o.alpha(j)), alpha, rtol=1e-5)
        assert o.alopt[j].t == int(step) == calls


@pytest.mark.parametrize("name", list(mo.CASES))
def test_oracle_float64_against_golden(fx, name):
    c = mo.case(name)
    inp = mo.inputs(c)
    np.testing.assert_array_equal(fx[name + "/idx"], np.stack(inp["idx"]))
    n, B, am = len(c["dims"]), c["batch"], max(a for _, a in c["dims"])
    np.testing.assert_array_equal(fx[name + "/eps"], np.stack([mo.pad_eps(e, n, B, am) for e in inp["eps"]]))
    tol = mo.tolerances(name, "reference")      # (the float64 oracle against the reference's recording)
    lr, la = tol["loss"]
    for calls in mo.RECORD_AFTER:
        o, outs = run(name, np.float64, calls)
        for k, out in enumerate(outs):
            np.testing.assert_allclose(out["critic_loss"], fx[name + "/critic_loss"][k], rtol=lr, atol=la, err_msg="critic loss, call %d" % k)
            np.testing.assert_allclose(out["actor_loss"], fx[name + "/actor_loss"][k], rtol=lr, atol=la, err_msg="actor loss, call %d" % k)
            np.testing.assert_allclose(out["critic_norm"], fx[name + "/critic_norm"][k], rtol=tol["norm"], err_msg="critic norm, call %d" % k)
            np.testing.assert_allclose(out["actor_norm"], fx[name + "/actor_norm"][k], rtol=tol["norm"], err_msg="actor norm, call %d" % k)
            np.testing.assert_allclose(out["alpha"], fx[name + "/alpha"][k], rtol=1e-5, err_msg="alpha, call %d" % k)
        check_state(fx, "%s/after%d" % (name, calls), o, c, calls, tol)


def test_golden_conditions(fx):
    """what the generator asserted, again on the committed file and the oracle"""
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    for name in mo.CASES:
        cn = fx[name + "/critic_norm"]
        assert name in ("seq",) or ((cn > 0.5).any() and (cn < 0.5).any()), name      # (seq's steeper critics are all above the clip)
        t = mo.inputs(mo.case(name))["table"]
        assert all(0 < x["done"].sum() < len(x["done"]) for x in t)
        _, outs = run(name, np.float64)
        for key in ("head0_target", "head0_actor"):
            assert 0.1 <= float(np.mean([o[key] for o in outs])) <= 0.9, (name, key)
    _, outs = run("clamp", np.float64)
    raw = np.concatenate([r.reshape(-1) for o in outs for r in o["raw_log_std"]])
    assert (raw > 2).any() and (raw < -20).any() and ((raw >= -20) & (raw <= 2)).any()


def shares(a, b, o32, o64, lrs, calls):
    """float32 run (a, o32) against float64 run (b, o64) -> each quantity's largest difference as a share of its tolerance"""
    worst = dict(loss=0.0, norm=0.0, alpha=0.0, param=0.0, param_max=0.0)
    for x, y in zip(a, b):
        for key in ("critic_loss", "actor_loss"):
            d = np.abs(np.array(x[key], np.float64) - np.array(y[key]))
            worst["loss"] = max(worst["loss"], float((d / (LOSS_TOL[1] + LOSS_TOL[0] * np.abs(np.array(y[key])))).max()))
        for key in ("critic_norm", "actor_norm"):
            d = np.abs(np.array(x[key]) - np.array(y[key])) / np.abs(np.array(y[key]))
            worst["norm"] = max(worst["norm"], float(d.max()) / NORM_RTOL)
        worst["alpha"] = max(worst["alpha"], float(np.max(np.abs(np.array(x["alpha"], np.float64) - np.array(y["alpha"])) / np.array(y["alpha"]))) / 1e-5)
    for nets32, nets64, lr in ((o32.actor + o32.actor_t, o64.actor + o64.actor_t, lrs[0]), (o32.critic + o32.critic_t, o64.critic + o64.critic_t, lrs[1])):
        for p32, p64 in zip(nets32, nets64):
            for k in p64:
                d = np.abs(p32[k].astype(np.float64) - p64[k])
                worst["param"] = max(worst["param"], float(np.quantile(d / (PARAM_TOL[1] + PARAM_TOL[0] * np.abs(p64[k])), 0.99)))
                worst["param_max"] = max(worst["param_max"], float(d.max()) / (2 * lr * calls))
    return worst


# the share of each tolerance the float32 oracle may take before that tolerance has to be set from the measurement (the issue's rule):
# a quarter, which leaves the device's other summation order three times as much
SHARE = 0.25


@pytest.mark.parametrize("name", list(mo.CASES))
def test_float32_against_float64(name):
    c = mo.case(name)
    o32, a = run(name, np.float32)
    o64, b = run(name, np.float64)
    worst = shares(a, b, o32, o64, (c["actor_lr"], c["critic_lr"]), c["n_learn"])
    print("%s: float32 against float64 as a share of the tolerance: %s" % (name, {k: round(v, 4) for k, v in worst.items()}))
    for k, w in mo.WIDEN.get(name, {}).items():      # (against the oracle only the losses of `clamp` are widened: 4 x the larger of the two measured gaps)
        if k in worst:
            worst[k] /= w
    assert max(worst.values()) <= SHARE + 0.01, worst


@pytest.mark.parametrize("name", list(mo.CASES))
def test_reference_against_float64(fx, name):
    """the same measurement for the reference's float32 recording: losses, norms, alpha, the sampled parameters and Adam's m against the
    float64 oracle, as shares of the unwidened tolerances (printed), each within a quarter of the tolerance the tests apply"""
    c = mo.case(name)
    o, outs = run(name, np.float64)
    w = dict(loss=0.0, norm=0.0, alpha=0.0)
    for k, out in enumerate(outs):
        for key in ("critic_loss", "actor_loss"):
            ref = fx[name + "/" + key][k].astype(np.float64)
            w["loss"] = max(w["loss"], float(np.max(np.abs(np.array(out[key], np.float64) - ref) / (LOSS_TOL[1] + LOSS_TOL[0] * np.abs(ref)))))
        for key in ("critic_norm", "actor_norm"):
            ref = fx[name + "/" + key][k]
            w["norm"] = max(w["norm"], float(np.max(np.abs(np.array(out[key]) - ref) / (NORM_RTOL * np.abs(ref)))))
        ref = fx[name + "/alpha"][k]
        w["alpha"] = max(w["alpha"], float(np.max(np.abs(np.array(out["alpha"], np.float64) - ref) / (1e-5 * ref))))
    w["param"] = w["m"] = 0.0
    pre = "%s/after%d" % (name, c["n_learn"])
    for j in range(len(c["dims"])):
        for key, got, names in (("actor", o.actor[j], mo.ACTOR_NAMES), ("critic", o.critic[j], mo.CRITIC_NAMES)):
            ref = fx["%s/%d/%s/sample" % (pre, j, key)].astype(np.float64)
            w["param"] = max(w["param"], float(np.max(np.abs(mo.compact_digest(got, names)[1] - ref) / (PARAM_TOL[1] + PARAM_TOL[0] * np.abs(ref)))))
        for key, opt, names in (("actor", o.aopt[j], mo.ACTOR_NAMES), ("critic", o.copt[j], mo.CRITIC_NAMES)):
            ref = fx["%s/%d/%s_m/sample" % (pre, j, key)].astype(np.float64)
            w["m"] = max(w["m"], float(np.max(np.abs(mo.compact_digest(opt.m, names)[1] - ref) / (2e-3 * np.abs(ref).max() + 2e-3 * np.abs(ref)))))
    print("%s: the reference's recording against float64 as a share of the tolerance: %s" % (name, {k: round(v, 4) for k, v in w.items()}))
    for k, f in dict(mo.WIDEN.get(name, {}), **mo.WIDEN_RECORDING.get(name, {})).items():
        if k in w:
            w[k] /= f
    assert max(w.values()) <= SHARE + 0.01, w


def _torch_actor(p, x, eps):
    h = torch.relu(torch.relu(x @ p["l1.weight"].T + p["l1.bias"]) @ p["l2.weight"].T + p["l2.bias"])
    mean, ls = h @ p["mean_layer.weight"].T + p["mean_layer.bias"], torch.clamp(h @ p["log_std_layer.weight"].T + p["log_std_layer.bias"], -20, 2)
    std = ls.exp()
    u = mean + std * eps
    lp = torch.distributions.Normal(mean, std).log_prob(u).sum(dim=1, keepdim=True)
    lp = lp - (2 * (np.log(2) - u - torch.nn.functional.softplus(-2 * u))).sum(dim=1, keepdim=True)
    return torch.tanh(u), lp


def _torch_critic(p, s, a):
    x = torch.cat(list(s) + list(a), dim=1)
    f = lambda names: torch.relu(torch.relu(x @ p[names[0] + ".weight"].T + p[names[0] + ".bias"]) @ p[names[1] + ".weight"].T + p[names[1] + ".bias"]) \
        @ p[names[2] + ".weight"].T + p[names[2] + ".bias"]
    return f(mo.Q1), f(mo.Q2)


@pytest.mark.parametrize("name,rtol", [("hetero", 1e-10), ("seq", 1e-10), ("clamp", 1e-6)])
def test_learn_against_autograd(name, rtol):
    """one whole learn() in double: torch autograd, clip_grad_norm_ and torch.optim.Adam on a restatement of MASAC.py:219-277 written here
    with torch ops (torch.min's own backward included) against the NumPy oracle, to 1e-10.  (`clamp` to 1e-6: at log_std = -20 autograd
    forms d log pi / d std from two terms of size eps^2 / std = 5e8 that cancel to their last bits; the oracle's closed form has no such
    terms, and the two differ by 1e-8 on under 1 % of a tensor's elements.)"""
    c = mo.case(name)
    inp = mo.inputs(c)
    o = mo.make(c, inp, np.float64)
    n = len(c["dims"])
    T = lambda x: torch.tensor(np.asarray(x, np.float64))
    tp = lambda ps: [{k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in p.items()} for p in ps]
    actor, critic = tp(inp["actor"]), tp(inp["critic"])
    actor_t = [{k: v.detach().clone() for k, v in p.items()} for p in actor]
    critic_t = [{k: v.detach().clone() for k, v in p.items()} for p in critic]
    a0 = c["alpha0"] or [0.01] * n
    log_alpha = [torch.tensor(np.log(a0[j]), dtype=torch.float64, requires_grad=True) for j in range(n)]
    aopt = [torch.optim.Adam(list(p.values()), lr=c["actor_lr"]) for p in actor]
    copt = [torch.optim.Adam(list(p.values()), lr=c["critic_lr"]) for p in critic]
    lopt = [torch.optim.Adam([la], lr=mo.ALPHA_LR) for la in log_alpha]
    t = inp["table"]
    got = dict(critic_loss=[], actor_loss=[], critic_norm=[], actor_norm=[], alpha=[])
    for i in range(n):
        rows, e = inp["idx"][0][i], [T(x) for x in inp["eps"][0][i]]
        obs, act, nobs = [T(x["obs"][rows]) for x in t], [T(x["act"][rows]) for x in t], [T(x["next_obs"][rows]) for x in t]
        rew, done = T(t[i]["rew"][rows])[:, None], T(t[i]["done"][rows].astype(np.float64))[:, None]
        alpha = log_alpha[i].exp().detach()
        with torch.no_grad():
            nxt = [_torch_actor(actor_t[j], nobs[j], e[j]) for j in range(n)]
            qa, qb = _torch_critic(critic_t[i], nobs, [x[0] for x in nxt])
            target = rew + c["gamma"] * (1 - done) * (torch.min(qa, qb) - alpha * nxt[i][1])
        q1, q2 = _torch_critic(critic[i], obs, act)
        loss = torch.nn.functional.mse_loss(q1, target) + torch.nn.functional.mse_loss(q2, target)
        copt[i].zero_grad()
        loss.backward()
        got["critic_norm"].append(float(torch.nn.utils.clip_grad_norm_(list(critic[i].values()), 0.5)))
        copt[i].step()
        got["critic_loss"].append(float(loss))
        new = [_torch_actor(actor[j], obs[j], e[n + j])[0] for j in range(n)]
        q1, q2 = _torch_critic(critic[i], obs, new)
        lp2 = _torch_actor(actor[i], obs[i], e[2 * n])[1]
        aloss = (-torch.min(q1, q2) + alpha * lp2).mean()
        for opt in aopt:
            opt.zero_grad()
        copt[i].zero_grad()
        aloss.backward()
        got["actor_norm"].append(float(torch.nn.utils.clip_grad_norm_(list(actor[i].values()), 0.5)))
        aopt[i].step()
        got["actor_loss"].append(float(aloss))
        lopt[i].zero_grad()
        (log_alpha[i].exp() * (-lp2.detach() + c["dims"][i][1])).mean().backward()
        lopt[i].step()
        got["alpha"].append(float(log_alpha[i].exp()))
    want = o.learn_with(inp["idx"][0], inp["eps"][0], c["gamma"], c["tau"])
    for key in got:
        np.testing.assert_allclose(np.array(want[key], np.float64), got[key], rtol=rtol, atol=1e-12, err_msg=key)
    for j in range(n):
        for k in actor[j]:
            np.testing.assert_allclose(o.actor[j][k], actor[j][k].detach().numpy(), rtol=rtol, atol=1e-12, err_msg="actor %d %s" % (j, k))
        for k in critic[j]:
            np.testing.assert_allclose(o.critic[j][k], critic[j][k].detach().numpy(), rtol=rtol, atol=1e-12, err_msg="critic %d %s" % (j, k))


def test_min_tie_splits_the_gradient():
    """what torch.min(a, b)'s backward does at a tie — what the oracle and masac_actor_kernel follow (DESIGN.md "MASAC")"""
    a = torch.tensor([1.0, 2.0, 3.0], requires_grad=True)
    b = torch.tensor([1.0, 3.0, 2.0], requires_grad=True)
    torch.min(a, b).sum().backward()
    assert a.grad.tolist() == [0.5, 1.0, 0.0] and b.grad.tolist() == [0.5, 0.0, 1.0]


def test_switches_discriminate():
    """each of the three wrong readings of the reference moves every compared actor quantity of the `seq` case by >= 10 x the GPU test's
    tolerance for it (agents 1.. ; mean_twins: agent 0 too)"""
    c = mo.case("seq")
    n = len(c["dims"])
    o, outs = run("seq", np.float64)
    a = outs[-1]
    inp = mo.inputs(c)
    for sw in ("stale_actors", "one_draw", "mean_twins"):
        x = mo.make(c, inp, np.float64, **{sw: True})
        for k in range(c["n_learn"]):
            b = x.learn_with(inp["idx"][k], inp["eps"][k], c["gamma"], c["tau"])
        for i in range(0 if sw == "mean_twins" else 1, n):
            f_loss = abs(float(a["actor_loss"][i]) - float(b["actor_loss"][i])) / (LOSS_TOL[1] + LOSS_TOL[0] * abs(float(a["actor_loss"][i])))
            f_norm = abs(a["actor_norm"][i] - b["actor_norm"][i]) / (NORM_RTOL * abs(a["actor_norm"][i]))
            f_par = max(float(np.quantile(np.abs(o.actor[i][k] - x.actor[i][k]) / (PARAM_TOL[1] + PARAM_TOL[0] * np.abs(o.actor[i][k])), 0.99)) for k in o.actor[i])
            print("%s agent %d: loss %.3g norm %.3g parameters %.3g x the tolerance" % (sw, i, f_loss, f_norm, f_par))
            assert min(f_loss, f_norm, f_par) >= 10, (sw, i, f_loss, f_norm, f_par)
