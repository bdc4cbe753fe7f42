"""CPU: the NumPy restatement of GAIL's discriminator (tests/gail_oracle.py) against the reference's recorded outputs
(tests/golden/gail.npz), its closed-form penalty gradient against torch's double backward, float32 against float64 on the golden
inputs (the evidence for the GPU tolerances), and ExpertDataset's scaling."""
import os

import numpy as np
import pytest
import torch

from tests import gail_oracle as go
from tests.golden import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = go.NAMES


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "gail.npz")))


def _run(c, inp, **kw):
    o = go.make(c, inp, **kw)
    tuples, pens, norms = [], [], []
    for k in range(c["n_learn"]):
        tuples.append(o.trian_D(inp["expert"][inp["idx"][k]], inp["policy"][k]))
        pens.append(o.penalty)
        norms.append(o.norm)
    return o, np.array(tuples, np.float64), np.array(pens), np.array(norms)


@pytest.mark.parametrize("name", list(go.CASES))
def test_oracle_matches_the_reference(fx, name):
    """Every call's 4-tuple, the rewards on the probe batch, the net, Adam's moments and the step count.  The reference runs in
    float32, the oracle in float64: 1e-5 relative covers the reference's own rounding over three calls."""
    c = go.case(name)
    inp = go.inputs(c)
    o, tuples, _, _ = _run(c, inp)
    np.testing.assert_allclose(tuples, fx[name + "/tuples"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(o.compute_reward(inp["probe"]), fx[name + "/reward"], rtol=1e-5, atol=1e-7)
    assert tuple(fx[name + "/betas"]) == go.betas(c["gp_coef"]) == (o.opt.b1, o.opt.b2)
    assert int(fx[name + "/step"]) == o.opt.t == c["n_learn"]
    synth.check_digest(name + "/net", o.p, fx, rtol=1e-4, atol=1e-6, label=name)
    synth.check_digest(name + "/m", o.opt.m, fx, rtol=1e-3, atol=1e-7, label=name)
    synth.check_digest(name + "/v", o.opt.v, fx, rtol=1e-3, atol=1e-10, label=name)
    if name == "bce":
        assert np.all(fx[name + "/tuples"][:, 3] == 0.0)


@pytest.mark.parametrize("activation", ["LeakyReLU", "ReLU"])
def test_penalty_gradient_matches_autograd(activation):
    """c mean_e ||dl/dx||^2 and its gradient in closed form against torch.autograd.grad(create_graph=True) in float64: 7 rows,
    5 columns, hidden 16.  Both sides are exact up to float64 rounding, so 1e-7 relative of the largest gradient element holds."""
    c = dict(go.COMMON, gp_coef=10.0, seed=4242, hidden=16, n_expert=7, n_policy=3, n_table=7, n_learn=1, activation=activation)
    inp = go.inputs(c, in_dim=5)
    o = go.make(c, inp)
    x = inp["expert"].astype(np.float64)
    _, cache = o.forward(x)
    pen, pg = o.penalty_grads(cache, go.GP_WEIGHT)
    act = torch.nn.LeakyReLU() if activation == "LeakyReLU" else torch.nn.ReLU()
    net = torch.nn.Sequential(torch.nn.Linear(5, 16), act, torch.nn.Linear(16, 16), act, torch.nn.Linear(16, 1)).double()
    lin = [net[0], net[2], net[4]]
    with torch.no_grad():
        for layer, n in zip(lin, NAMES):
            layer.weight.copy_(torch.as_tensor(inp["net"][n + ".weight"], dtype=torch.float64))
            layer.bias.copy_(torch.as_tensor(inp["net"][n + ".bias"], dtype=torch.float64))
    xt = torch.as_tensor(x).requires_grad_(True)
    out = net(xt)
    g = torch.autograd.grad(out, xt, grad_outputs=torch.ones_like(out), create_graph=True, retain_graph=True, only_inputs=True)[0]
    loss = go.GP_WEIGHT * torch.mean(torch.sum(torch.square(g), dim=-1))
    loss.backward()
    np.testing.assert_allclose(go.GP_WEIGHT * pen, loss.item(), rtol=1e-12)
    np.testing.assert_allclose(o.input_grad(cache)[0], g.detach().numpy(), rtol=1e-10, atol=1e-14)
    for layer, n in zip(lin, NAMES):
        want = layer.weight.grad.numpy()
        scale = np.abs(want).max()
        assert scale > 0
        gap = np.abs(pg[n + ".weight"] - want).max()
        print("%s %s: max |closed form - autograd| %.3g of %.3g" % (activation, n, gap, scale))
        assert gap <= 1e-7 * scale
        assert layer.bias.grad is None or float(layer.bias.grad.abs().max()) == 0.0      # biases: nothing


def test_full_step_matches_autograd_float64():
    """One whole trian_D in each mode against torch in float64 (loss, every gradient through Adam): parameters after the step."""
    for gp_coef in (0.0, 10.0):
        c = dict(go.COMMON, gp_coef=gp_coef, seed=77, hidden=16, n_expert=9, n_policy=6, n_table=20, n_learn=1)
        inp = go.inputs(c)
        o = go.make(c, inp)
        act = torch.nn.LeakyReLU()
        net = torch.nn.Sequential(torch.nn.Linear(4, 16), act, torch.nn.Linear(16, 16), act, torch.nn.Linear(16, 1)).double()
        lin = [net[0], net[2], net[4]]
        with torch.no_grad():
            for layer, n in zip(lin, NAMES):
                layer.weight.copy_(torch.as_tensor(inp["net"][n + ".weight"], dtype=torch.float64))
                layer.bias.copy_(torch.as_tensor(inp["net"][n + ".bias"], dtype=torch.float64))
        opt = torch.optim.Adam(net.parameters(), lr=c["d_lr"], betas=go.betas(gp_coef))
        xe = torch.as_tensor(inp["expert"][inp["idx"][0]].astype(np.float64))
        xp = torch.as_tensor(inp["policy"][0].astype(np.float64))
        F = torch.nn.functional
        if gp_coef > 0:
            le, lp = net(xe), net(xp)
            loss = 0.5 * (F.binary_cross_entropy_with_logits(le, torch.ones_like(le)) + F.binary_cross_entropy_with_logits(lp, torch.zeros_like(lp)))
            xd = xe.clone().requires_grad_(True)
            od = net(xd)
            g = torch.autograd.grad(od, xd, grad_outputs=torch.ones_like(od), create_graph=True, retain_graph=True, only_inputs=True)[0]
            loss = loss + 5 * torch.mean(torch.sum(torch.square(g), dim=-1))
        else:
            pe, pp = torch.sigmoid(net(xe)), torch.sigmoid(net(xp))
            loss = F.binary_cross_entropy(pe, torch.ones_like(pe)) + F.binary_cross_entropy(pp, torch.zeros_like(pp))
        opt.zero_grad()
        loss.backward()
        opt.step()
        got = o.trian_D(xe.numpy(), xp.numpy())
        np.testing.assert_allclose(got[0], loss.item(), rtol=1e-12)
        for layer, n in zip(lin, NAMES):
            np.testing.assert_allclose(o.p[n + ".weight"], layer.weight.detach().numpy(), rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(o.p[n + ".bias"], layer.bias.detach().numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", list(go.CASES))
def test_float32_sits_inside_the_gpu_tolerances(name):
    """The oracle in float32 against float64 on the golden inputs, held to tests/test_gpu_gail.py's tolerances WITHOUT the 1 %
    allowance: what two correct implementations of this second-order update differ by in fp32 is far inside them."""
    c = go.case(name)
    inp = go.inputs(c)
    o64, t64, p64, n64 = _run(c, inp)
    o32, t32, p32, n32 = _run(c, inp, dtype=np.float32)
    print("%s: tuples max rel gap %.3g, penalty %.3g, norm %.3g" % (name, np.max(np.abs(t32 - t64) / np.maximum(np.abs(t64), 1e-6)),
                                                                    np.max(np.abs(p32 - p64)), np.max(np.abs(n32 - n64) / n64)))
    np.testing.assert_allclose(t32, t64, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(p32, p64, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(n32, n64, rtol=1e-3)
    for k in o64.p:
        d = np.abs(o32.p[k] - o64.p[k])
        print("   %-18s max |theta32 - theta64| %.3g   max |m32 - m64| %.3g of %.3g" % (k, d.max(), np.abs(o32.opt.m[k] - o64.opt.m[k]).max(), np.abs(o64.opt.m[k]).max()))
        assert np.all(d <= 5e-6 + 5e-4 * np.abs(o64.p[k])), k
        assert np.abs(o32.opt.m[k] - o64.opt.m[k]).max() <= 2e-3 * np.abs(o64.opt.m[k]).max(), k
    np.testing.assert_allclose(o32.compute_reward(inp["probe"]), o64.compute_reward(inp["probe"]), rtol=1e-4)


def test_bce_clamps_at_saturation():
    """Logits of +-20 and +-90 through the head bias: fp32 sigmoid is exactly 1 / exactly 0 there (p32), the log clamps at -100 and
    the backward's divisor at 1e-12 — the loss is 100 per saturated wrong-side row and finite, the gradients are finite."""
    c = dict(go.COMMON, gp_coef=0.0, seed=31, n_learn=1)
    inp = go.inputs(c)
    for bias, want_e, want_p in ((20.0, 0.0, 100.0), (-90.0, 100.0, 0.0), (90.0, 0.0, 100.0)):
        net = {k: v.copy() for k, v in inp["net"].items()}
        net[NAMES[2] + ".bias"][:] = bias
        o = go.Discriminator(net, c["d_lr"], 0.0, dtype=np.float64, p32=True)
        out, grads = o.loss_and_grads(inp["expert"][inp["idx"][0]], inp["policy"][0])
        assert np.isfinite(out[0]) and abs(out[0] - (want_e + want_p)) < 1e-6, (bias, out)
        assert all(np.all(np.isfinite(g)) for g in grads.values())


def test_expert_dataset_scaling_and_refusal(fx):
    from freerl_amd.GAIL import ExpertDataset
    c = go.case("class")
    states, actions = go.raw_expert(c, c["seed"])
    ds = ExpertDataset((states, actions))
    assert len(ds) == int(fx["class/n"]) == c["n_table"]
    synth.check_digest("class/dataset", dict(states=ds.states, actions=ds.actions, space_low=ds.space_low, space_high=ds.space_high,
                                             action_low=ds.action_low, action_high=ds.action_high), fx, rtol=1e-12, atol=1e-12)
    for arr in (ds.states, ds.actions):
        np.testing.assert_allclose(arr.min(axis=0), -1.0, atol=1e-12)
        np.testing.assert_allclose(arr.max(axis=0), 1.0, atol=1e-12)
    want, _, _ = go.minmax_scale(states)
    np.testing.assert_array_equal(ds.states, want)
    s, a = ds[3]
    assert s.dtype == torch.float32 and a.dtype == torch.float32 and s.shape == (c["s_dim"],)
    flat = states.copy()
    flat[:, 1] = 2.5
    with pytest.raises(ValueError, match="states column 1"):
        ExpertDataset((flat, actions))
    with pytest.raises(ValueError, match="actions column 0"):
        ExpertDataset((states, np.zeros_like(actions)))


def test_expert_dataset_from_file(tmp_path):
    from freerl_amd.GAIL import ExpertDataset
    c = go.case("class")
    states, actions = go.raw_expert(c, 5)
    path = os.path.join(str(tmp_path), "expert.npz")
    np.savez(path, states=states, actions=actions)
    a, b = ExpertDataset(path), ExpertDataset((states, actions))
    np.testing.assert_array_equal(a.states, b.states)
    np.testing.assert_array_equal(a.actions, b.actions)
