"""GPU: DDPG.learn with trick['popart'] (DDPG_file/DDPG_simple_with_tricks.py:95-292) on kernels_popart.hip against `Ref`, a float64
restatement of learn() in torch with autograd (checked once on the CPU against the imported reference class).  Losses, norms, parameters
and Adam's m take tests/test_gpu_envelope_ddpg.py's tolerances; {W, b, sigma, mu, nu} take STAT_RTOL: Ref in float32 next to float64 over
these cases deviates by at most 7.5e-7 relative (CPU, three calls per case); four times that, for the device's other summation order,
is below the floor of 1e-4.  Every call keeps var(y) >= 0.1 mean(y^2) (asserted on the float64 run; smallest 0.75)."""
import numpy as np
import pytest
import torch

from tests.hip_helpers import flat_params
from tests.test_gpu_envelope_ddpg import _assert_m, _assert_net

pytestmark = pytest.mark.gpu

NAMES = ("l1", "l2", "l3")
HP = dict(gamma=0.95, tau=0.01, actor_lr=1e-3, critic_lr=2e-3, upper_lr=1e-3, beta=0.99999)
STAT_RTOL = 1e-4
CASES = [(3, 1, 2, 1, 1), (3, 1, 16, 1, 1), (33, 5, 17, 1, 1), (5, 2, 34, 1, 2), (5, 2, 70, 1, 3), (4, 3, 16, 3, 1)]      # O, A, batch, P, FRL_CPS


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    _native.lib()
    return _native


def inputs(O, A, rows, seed, hidden=32, reward_scale=1.0, reward_mean=0.0):
    g = np.random.default_rng(seed)

    def net(dims):
        return {"%s.%s" % (n, k): g.uniform(-1, 1, (o, i) if k == "weight" else (o,)).astype(np.float32) / np.float32(np.sqrt(i))
                for n, (o, i) in zip(NAMES, dims) for k in ("weight", "bias")}
    table = dict(obs=g.normal(size=(rows, O)), act=g.uniform(-1, 1, (rows, A)), rew=reward_scale * (reward_mean + g.normal(size=rows)),
                 done=(g.random(rows) < 0.2).astype(np.float64), next_obs=g.normal(size=(rows, O)))
    return dict(actor=net([(hidden, O), (hidden, hidden), (A, hidden)]), critic=net([(hidden, O + A), (hidden, hidden), (1, hidden)]),
                table={k: v.astype(np.float32) for k, v in table.items()})


def mlp(p, x, tanh=False):
    h = torch.relu(x @ p["l1.weight"].T + p["l1.bias"])
    h = torch.relu(h @ p["l2.weight"].T + p["l2.bias"])
    o = h @ p["l3.weight"].T + p["l3.bias"]
    return torch.tanh(o) if tanh else o


class Ref:
    """learn() restated (:253-292 with PopArt.forward, :128-181) in `dt`; not the reference's: nu - mu_new^2 <= 0 keeps sigma."""

    def __init__(self, inp, state=(1.0, 0.0, 1.0, 0.0, 1.0), dt=torch.float64):
        def mk(d, grad):
            return {k: torch.tensor(v, dtype=dt, requires_grad=grad) for k, v in d.items()}
        self.dt, self.table = dt, {k: torch.tensor(v, dtype=dt) for k, v in inp["table"].items()}
        self.actor, self.critic, self.actor_t, self.critic_t = mk(inp["actor"], True), mk(inp["critic"], True), mk(inp["actor"], False), mk(inp["critic"], False)
        self.W, self.b = (torch.tensor(float(v), dtype=dt, requires_grad=True) for v in state[:2])
        self.sigma, self.mu, self.nu = (torch.tensor(float(v), dtype=dt) for v in state[2:])
        self.opt = {k: torch.optim.Adam(ps, lr=HP[lr]) for k, ps, lr in (("actor", list(self.actor.values()), "actor_lr"),
                    ("critic", list(self.critic.values()), "critic_lr"), ("upper", [self.W, self.b], "upper_lr"))}

    def q(self, critic, s, a):
        return self.sigma * (self.W * mlp(critic, torch.cat([s, a], 1)) + self.b) + self.mu

    def learn(self, idx, beta=HP["beta"]):
        t, clip = self.table, torch.nn.utils.clip_grad_norm_
        s, a, r, d, s2 = (t[k][idx] for k in ("obs", "act", "rew", "done", "next_obs"))
        r, d, beta = r[:, None], d[:, None], float(np.float32(beta))
        with torch.no_grad():
            y = r + HP["gamma"] * (1 - d) * self.q(self.critic_t, s2, mlp(self.actor_t, s2, True))
            mu_new = (1 - beta) * self.mu + beta * y.mean()
            self.nu = (1 - beta) * self.nu + beta * (y * y).mean()
            var = self.nu - mu_new ** 2
            self.var_ratio = float(y.var(unbiased=False) / (y * y).mean())
            fired = not bool(var > 0)
            sigma_new = self.sigma if fired else torch.sqrt(var)
            self.W *= self.sigma / sigma_new
            self.b.copy_(self.b * self.sigma / sigma_new + (self.mu - mu_new) / sigma_new)
            self.sigma, self.mu = sigma_new, mu_new
        [o.zero_grad() for o in self.opt.values()]
        loss = ((self.W * mlp(self.critic, torch.cat([s, a], 1)) + self.b - (y - self.mu) / self.sigma) ** 2).mean()
        loss.backward()
        n_lower = clip(self.critic.values(), 0.5)
        self.opt["critic"].step()
        n_upper = clip([self.W, self.b], 0.5)
        self.opt["upper"].step()
        aloss = -self.q(self.critic, s, mlp(self.actor, s, True)).mean()
        self.opt["actor"].zero_grad()
        aloss.backward()
        n_actor = clip(self.actor.values(), 0.5)
        self.opt["actor"].step()
        with torch.no_grad():
            for tg, src in ((self.critic_t, self.critic), (self.actor_t, self.actor)):
                for k in tg:
                    tg[k].mul_(1 - HP["tau"]).add_(HP["tau"] * src[k])
        return [float(v) for v in (loss.detach(), n_lower, n_upper, aloss.detach(), n_actor, self.sigma, self.mu, -len(idx) if fired else len(idx))]

    def state(self):
        return np.array([float(v.detach()) for v in (self.W, self.b, self.sigma, self.mu, self.nu)])

    def arrays(self, key):
        on, opt = getattr(self, key), self.opt[key]
        return ({k: v.detach().numpy() for k, v in on.items()}, {k: v.numpy() for k, v in getattr(self, key + "_t").items()},
                {k: opt.state[v]["exp_avg"].numpy() for k, v in on.items()})


def engine(N, O, A, cap, P=1, batch_max=16, hidden=32, **kw):
    from freerl_amd.engine import Engine
    return Engine(N.ALGO_DDPG_POPART, O, A, cap, n_learners=P, hidden=hidden, batch_max=batch_max, **kw)


def load(e, inp, p=0, state=None):
    for net, key in ((0, "actor"), (1, "critic")):
        for kind in (0, 1):
            e.set_params(net, flat_params(inp[key], NAMES), kind, learner=p)
    t, lay = inp["table"], e.layout
    rec = np.zeros((len(t["done"]), e.width), np.float32)
    for off, key in ((lay.obs_off[0], "obs"), (lay.act_off[0], "act"), (lay.rew_off, "rew"), (lay.done_off, "done"), (lay.next_obs_off[0], "next_obs")):
        v = t[key].reshape(len(rec), -1)
        rec[:, off:off + v.shape[1]] = v
    e.add_batch(rec, learners=np.full(len(rec), p, np.int32))
    if state is not None:
        e.popart_set(state, learner=p)


def assert_out(got, want, msg):
    # [8] in _native.POPART_OUT's order: losses at the loss tolerance, norms at rtol 1e-3, sigma and mu at STAT_RTOL, the rows exactly
    print("%s\n  engine %s\n  ref    %s" % (msg, got, np.array(want)))
    for col, (rtol, atol) in enumerate(((1e-4, 1e-6), (1e-3, 0), (1e-3, 0), (1e-4, 1e-6), (1e-3, 0), (STAT_RTOL, 0), (STAT_RTOL, 1e-6), (0, 0))):
        np.testing.assert_allclose(got[col], want[col], rtol=rtol, atol=atol, err_msg="out[%d], %s" % (col, msg))


def check_state(e, ref, calls, label, p=0):
    np.testing.assert_allclose(e.popart_get(p), ref.state(), rtol=STAT_RTOL, atol=1e-6, err_msg=label + " {W, b, sigma, mu, nu}")
    for net, key, lr in ((0, "actor", HP["actor_lr"]), (1, "critic", HP["critic_lr"])):
        online, target, m = ref.arrays(key)
        _assert_net(e.get_params(net, 0, p), online, NAMES, 5e-4, 5e-6, lr, calls, "%s %s" % (label, key))
        _assert_net(e.get_params(net, 1, p), target, NAMES, 5e-4, 5e-6, lr, calls, "%s %s target" % (label, key))
        _assert_m(e.get_params(net, 2, p), m, NAMES, "%s %s" % (label, key))
        assert e.opt_step(net, learner=p) == calls


@pytest.mark.parametrize("O,A,batch,P,cps", CASES)
def test_learn_vs_float64(N, monkeypatch, O, A, batch, P, cps):
    """Three calls on given rows, so that the popped W, b and the moved statistics feed the next call's target.  16-row chunks: a short one,
    exactly one, one + 1 row with a wide head and an obs past one k-tile, two workgroups of 2 and 3 chunks, three learners of their own."""
    monkeypatch.setenv("FRL_RC", "16")
    monkeypatch.setenv("FRL_CPS", str(cps))
    cap = 2 * batch + 3
    e = engine(N, O, A, cap, P, batch_max=batch if cps == 1 else 32 * cps)
    assert e.lds_bytes()[1] == 16
    scales, states = (1.0, 30.0, 0.01), ((1.0, 0.0, 1.0, 0.0, 1.0), (0.7, -0.3, 20.0, 5.0, 425.0), (1.5, 0.2, 0.02, 0.001, 0.000401))
    inps = [inputs(O, A, cap, 100 * O + 10 * batch + p, reward_scale=scales[p]) for p in range(P)]
    refs = [Ref(inp, states[p]) for p, inp in enumerate(inps)]
    for p, inp in enumerate(inps):
        load(e, inp, p, states[p])
    g = np.random.default_rng(5 if batch == 2 else batch)      # (two rows: a stream whose three pairs of targets meet the condition below)
    for call in range(3):
        idx = np.stack([g.choice(cap, batch, replace=False) for _ in range(P)])
        got = e.popart_ddpg_learn(batch, idx=idx, **HP)
        for p in range(P):
            want = refs[p].learn(idx[p])
            assert refs[p].var_ratio >= 0.1, "the inputs' condition: var(y) / mean(y^2) = %g" % refs[p].var_ratio
            assert_out(got[p], want, "O %d A %d batch %d learner %d call %d" % (O, A, batch, p, call))
    for p in range(P):
        check_state(e, refs[p], 3, "O%d A%d B%d p%d" % (O, A, batch, p), p)
    e.close()


def test_pop_preserves_outputs(N, monkeypatch):
    """Rewards around 100, every rate 0: sigma and mu move by a factor > 10, sigma (W h + b) + mu on 8 probe rows stays (1e-5 of max|Q| +
    |mu|: a handful of fp32 roundings of that size), no net changes by a bit (tau 0 too: (1 - tau) x + tau x rounds, in torch as here)."""
    monkeypatch.setenv("FRL_RC", "16")
    O, A, B = 4, 2, 24
    inp = inputs(O, A, 40, 7, reward_scale=100.0, reward_mean=1.0)
    e = engine(N, O, A, 40, batch_max=B)
    load(e, inp)
    probe = np.random.default_rng(1).normal(size=(1, 8, O + A)).astype(np.float32)

    def q():
        W, b, sigma, mu, _ = e.popart_get().astype(np.float64)
        return sigma * (W * e.act(1, N.ACT_RAW, probe, out_dim=1)[0, :, 0].astype(np.float64) + b) + mu, sigma, mu
    before, nets = q(), [e.get_params(net, kind) for net in (0, 1) for kind in (0, 1)]
    out = e.popart_ddpg_learn(B, idx=np.arange(B)[None], **dict(HP, actor_lr=0.0, critic_lr=0.0, upper_lr=0.0, tau=0.0))[0]
    after = q()
    assert after[1] > 10 * before[1] and abs(after[2]) > 10 and out[7] == B
    np.testing.assert_allclose(after[0], before[0], rtol=0, atol=1e-5 * (np.abs(before[0]).max() + abs(after[2])))
    for old, (net, kind) in zip(nets, [(n, k) for n in (0, 1) for k in (0, 1)]):
        assert np.array_equal(old, e.get_params(net, kind)), (net, kind)
    e.close()


def test_variance_guard(N, monkeypatch):
    """All rewards 2, done = 1 and beta = 1: nu - mu^2 is exactly 0 in any precision (at the script's beta the old statistics' share keeps
    it positive).  sigma stays, mu and nu move, rows is negated, all finite; the next call, ordinary, matches Ref under the same rule."""
    monkeypatch.setenv("FRL_RC", "16")
    O, A, B = 3, 2, 16
    inp = inputs(O, A, 40, 11)
    inp["table"]["rew"][:B] = 2.0
    inp["table"]["done"][:B] = 1.0
    e, ref = engine(N, O, A, 40, batch_max=B), Ref(inp)
    load(e, inp)
    for idx, beta in ((np.arange(B), 1.0), (np.arange(B, 2 * B), HP["beta"])):
        got, want = e.popart_ddpg_learn(B, idx=idx[None], **dict(HP, beta=beta))[0], ref.learn(idx, beta)
        assert_out(got, want, "beta %g" % beta)
        assert np.isfinite(got).all() and np.isfinite(e.popart_get()).all()
        if beta == 1.0:
            assert got[7] == -B and got[5] == 1.0 and tuple(e.popart_get()[2:]) == (1.0, 2.0, 4.0)
    check_state(e, ref, 2, "guard")
    e.close()


def test_class(N):
    """The class's surface; a host-drawn learn() equals the engine call on the indices NumPy draws; the refusals name the entry point."""
    from freerl_amd.DDPG_simple_with_tricks import DDPG
    from freerl_amd.TD3 import DDPG as Plain
    mk = lambda: DDPG([3, 2], True, 1e-3, 2e-3, 64, "cpu", trick={"popart": True}, hidden=32, batch_max=16, rng="host")
    a, b = [(torch.manual_seed(3), mk())[1] for _ in range(2)]
    keys = ["%s.%s" % (n, k) for n in NAMES for k in ("weight", "bias")]
    for net in (a.agent.actor, a.agent.critic, a.agent.actor_target, a.agent.critic_target):
        assert list(net.state_dict().keys()) == keys
    pa = a.agent.critic_PopArt
    assert pa.upper_layer.output_linear.weight.data.shape == (1, 1) and pa.upper_layer.output_linear.bias.data.shape == (1,)
    assert (float(pa.sigma), float(pa.mu), float(pa.nu)) == (1.0, 0.0, 1.0) and float(pa.normalize(pa.denormalize(torch.tensor(3.0)))) == 3.0
    g = np.random.default_rng(5)
    for _ in range(40):
        row = (g.normal(size=3), g.uniform(-1, 1, 2), g.normal(), g.normal(size=3), g.random() < 0.2)
        a.add(*row)
        b.add(*row)
    np.random.seed(9)
    a.learn(16, 0.95, 0.01)
    idx = np.random.RandomState(9).choice(40, 16, replace=False)
    assert np.array_equal(a.last_indices, idx)
    out = b._e.popart_ddpg_learn(16, gamma=0.95, tau=0.01, actor_lr=1e-3, critic_lr=2e-3, idx=idx[None])[0]
    assert np.array_equal(a.last_out, out) and np.array_equal(a._e.popart_get(), b._e.popart_get())
    obs = g.normal(size=3).astype(np.float32)
    assert np.array_equal(a.select_action(obs), a.agent.actor(obs[None]).numpy()[0]) and a.select_action(obs).shape == (2,)
    x = torch.zeros(4, 3), torch.zeros(4, 2)
    assert torch.equal(pa.output(*x), pa.upper_layer(a.agent.critic(*x))) and pa.output_target(*x).shape == (4, 1)
    plain = DDPG([3, 2], True, 1e-3, 2e-3, 64, "cpu", trick={"popart": False}, hidden=32, batch_max=16)
    assert isinstance(plain, Plain) and plain._e.algo == N.ALGO_DDPG
    with pytest.raises(ValueError, match="argmax"):
        DDPG([3, 2], False, 1e-3, 2e-3, 64, "cpu", trick={"popart": True})
    for eng, call, text in ((plain._e, "popart_ddpg_learn", "frl_popart_ddpg_learn does not serve DDPG engines"),
                            (a._e, "learn", r"frl_learn does not serve PopArt-DDPG engines \(updates: frl_popart_ddpg_learn\)")):
        with pytest.raises(N.FrlError, match="error 4: " + text):
            getattr(eng, call)(16, gamma=0.95, tau=0.01, actor_lr=1e-3, critic_lr=2e-3)
