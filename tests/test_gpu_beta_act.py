"""The Beta actor's device draw (FRL_ACT_PPO_SAMPLE on a PPO engine with actor_dist = 1) through frl_act, frl_ppo_rollout and
PPO(beta=True, rng="device"), against float64 SciPy.  LOGP_ATOL = 4 x 1.237e-7: the float64 log-density on float64 head rows against the
same rows rounded to float32, over test_logp_and_range's inputs (tools/beta_act_gap.py, on the CPU).  KS_BOUND: Dvoretzky-Kiefer-Wolfowitz,
2 exp(-2 n eps^2) = 1e-6 at n = 8192; SciPy's own sampler stays under 0.021 there (same tool)."""
import numpy as np
import pytest
import torch
from scipy import stats
from scipy.special import betaln

pytestmark = pytest.mark.gpu
LOGP_ATOL, N_LAW, O = 4.9e-7, 8192, 5
KS_BOUND = float(np.sqrt(np.log(2 / 1e-6) / (2 * N_LAW)))          # 0.0298


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    return _native


def logpdf_err(z, x, lp):
    """max |lp - float64 Beta log-density at x|, alpha / beta = softplus(z) + 1 of the head rows z = [alpha_layer | beta_layer]."""
    z, x, A = np.asarray(z, np.float64), np.asarray(x, np.float64), x.shape[-1]
    sp = np.where(z > 20, z, np.log1p(np.exp(np.minimum(z, 20)))) + 1
    al, be = sp[..., :A], sp[..., A:]
    return np.abs(lp - ((al - 1) * np.log(x) + (be - 1) * np.log1p(-x) - betaln(al, be))).max()


@pytest.mark.parametrize("A", [1, 3, 8, 17])          # 2A = 16 fills one head tile; 17 (the widest head of the project's configs) takes three
@pytest.mark.parametrize("n_rows", [1, 17, 65])       # one row past a 16-row and a 64-row chunk
def test_logp_and_range(N, n_rows, A):
    from freerl_amd.engine import Engine
    e = Engine(N.ALGO_PPO, O, A, 8, n_learners=2, batch_max=8, extra_cols=A + 1, actor_dist=1, seed=11)
    g = np.random.default_rng(1000 * n_rows + A)
    obs = g.standard_normal((2, n_rows, O)).astype(np.float32)
    par = (g.standard_normal((2, e.num_params(0))) * 0.1).astype(np.float32)
    par[:, -2 * A:] = g.standard_normal((2, 2 * A)) * 1.5          # head biases: alpha, beta from 1.0 to about 6
    for p in range(2):
        e.set_params(0, par[p], learner=p)
    z = e.act(0, N.ACT_RAW, obs, out_dim=2 * A)
    x, lp = e.act(0, N.ACT_PPO_SAMPLE, obs, out_dim=A, want_logp=True)
    assert np.all(np.isfinite(x)) and np.all(x > 0) and np.all(x < 1) and np.all(np.isfinite(lp))
    print("n_rows %d A %d: max |logp - float64| %.3e" % (n_rows, A, logpdf_err(z, x, lp)))
    assert logpdf_err(z, x, lp) <= LOGP_ATOL
    with pytest.raises(N.FrlError, match="eps must be NULL"):      # nothing sensible to inject into a rejection sampler
        e.act(0, N.ACT_PPO_SAMPLE, obs, eps=np.zeros((2, n_rows, A), np.float32), out_dim=A)
    e.close()


def test_law(N):
    """Zero weights, the head bias sets (alpha, beta) per dimension; 8192 identical rows cross 128 workgroups."""
    from freerl_amd.engine import Engine
    al, be = np.array([1 + np.log1p(np.exp(-12.0)), 1.3, 20.0]), np.array([1 + np.log1p(np.exp(-12.0)), 9.0, 20.0])
    e = Engine(N.ALGO_PPO, O, 3, 8, batch_max=8, extra_cols=4, actor_dist=1, seed=5)
    par = np.zeros(e.num_params(0), np.float32)
    par[-6:] = np.log(np.expm1(np.concatenate([al, be]) - 1))      # softplus^-1: -12 for the shapes of 1 + 6e-6
    e.set_params(0, par)
    obs = np.zeros((1, N_LAW, O), np.float32)
    x1 = e.act(0, N.ACT_PPO_SAMPLE, obs, out_dim=3)
    assert (x1 == e.act(0, N.ACT_PPO_SAMPLE, obs, out_dim=3)).mean() < 1e-3      # another launch, another counter value
    for c in range(3):
        ks = stats.kstest(x1[0, :, c].astype(np.float64), stats.beta(al[c], be[c]).cdf).statistic
        print("Beta(%.4g, %.4g): KS distance %.4f (bound %.4f)" % (al[c], be[c], ks, KS_BOUND))
        assert ks <= KS_BOUND
    e.close()


def test_collector(N):
    from freerl_amd.engine import Engine
    from freerl_amd.envpool import EnvPool, ppo_rollout
    P, E, Tseg = 2, 4, 8
    pool = EnvPool("SynLinear-v0", P * E, n_threads=2, seed=4)
    Oe, A, T = pool.obs_dim, pool.act_dim, E * Tseg
    e = Engine(N.ALGO_PPO, Oe, A, T, n_learners=P, batch_max=T, extra_cols=A + 1, actor_dist=1, seed=3)
    g = np.random.default_rng(2)
    for p in range(P):
        e.set_params(0, (g.standard_normal(e.num_params(0)) * 0.1).astype(np.float32), learner=p)
        e.set_params(1, (g.standard_normal(e.num_params(1)) * 0.1).astype(np.float32), learner=p)
    out = ppo_rollout(e, pool, 1, envs_per_learner=E, steps_per_env=Tseg, minibatch=T, k_epochs=1, actor_lr=0.0, critic_lr=0.0)
    assert out["env_steps"] == P * T
    lay, rows = e.layout, np.stack([e.read_rows(p, 0, T) for p in range(P)])
    z = e.act(0, N.ACT_RAW, rows[:, :, lay.obs_off[0]:lay.obs_off[0] + Oe], out_dim=2 * A)      # lr = 0: still the collecting policy
    act, logp = rows[:, :, lay.act_off[0]:lay.act_off[0] + A], rows[:, :, lay.extra_off:lay.extra_off + A]
    assert np.all(act > 0) and np.all(act < 1) and not np.array_equal(act[0], act[1])
    assert logpdf_err(z, act, logp) <= LOGP_ATOL
    assert np.all(rows[:, :, lay.extra_off + A].reshape(P, E, Tseg)[:, :, -1] == 1)      # adv_done on each segment's last row
    pool.close(); e.close()


def test_class():
    from freerl_amd.PPO import PPO
    A, obs = 3, np.random.default_rng(1).standard_normal(O).astype(np.float32)
    torch.manual_seed(3)
    dev = PPO([O, A], True, 1e-3, 1e-3, 16, torch.device("cuda"), trick={}, beta=True, rng="device")
    a, lp = dev.select_action(obs)
    assert a.shape == (A,) and lp.shape == (A,) and np.all((a > 0) & (a < 1)) and not np.array_equal(a, dev.select_action(obs)[0])
    assert logpdf_err(dev.agent.actor(obs.reshape(1, -1)).numpy()[0], a, lp) <= LOGP_ATOL
    host = PPO([O, A], True, 1e-3, 1e-3, 16, torch.device("cuda"), trick={}, beta=True)      # rng="host": torch's own sampler, as before
    torch.manual_seed(7)
    a, lp = host.select_action(obs)
    torch.manual_seed(7)
    dist = torch.distributions.Beta(*host.agent.actor.alpha_beta(obs.reshape(1, -1)))
    want = dist.sample()
    np.testing.assert_array_equal(a, want.numpy()[0])
    np.testing.assert_array_equal(lp, dist.log_prob(want).numpy()[0])
