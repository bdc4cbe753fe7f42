"""frl_ppo_learn at its minibatch, horizon and head-width edges, at Engine level, against the oracle (oracle/ppo.py:
PPO.learn_with) on the same seeded inputs (tests/ppo_edge_cases.py): the on-chip kernel (kernels_ppo2.hip) with minibatches that
are no multiple of its 64-row chunk nor of a wave's 16 rows, short last minibatches, head widths 1 / 5 / 16, k_pad exactly 16
and 32, Categorical heads of 2 / 5 / 16 classes, one raw log_std past the clamp (its column bit-unchanged, its Adam m 0); the streaming kernel (kernels_ppo.hip, FRL_PPO_STREAMING=1) on the same cases
and on the shapes only it serves (obs 33, head 17, hidden 64 / 256, Beta, cautious AdamW); the two kernels against each
other; the GAE scans (gae_scan, ppo_gae_sb3_kernel, frl_gae) at horizons with a short last segment, empty trailing segments
and fewer rows than a wave, with adv_done on segment and wave seams; a population of three learners.

Tolerances are test_ppo_learn's (tests/test_gpu_parity.py), unchanged: actor loss rtol 2e-4 / atol 5e-6, critic loss rtol 2e-4,
every parameter rtol 2e-3 / atol 2e-5, advantages and value targets rtol 1e-4 / atol 1e-5; the cautious-AdamW case uses
test_ppo_py_cautious_adamw's rule for the parameters (fewer than 2e-3 of a tensor's elements outside the parameter
tolerance: the cautious mask flips single elements on rounding-level differences) and the same loss tolerances.  The GAE bound is derived in
tests/ppo_edge_cases.py's docstring and met by a float32 emulation of the scan on the CPU (tests/test_ppo_edge_cases.py).

Measured on an MI355X: the float32 scans stay within 0.08 of that bound at every horizon and pattern (0.06 on the seams),
ppo_gae_sb3_kernel is bit-equal to the float32 cast of the float64 formula (0 ulp of the 2 allowed) everywhere.

Every test asserts the conditions on its inputs (ratios off the clip edges, log_std off its clamp, hidden units off ReLU's kink,
the oracle's own conditioning, TD residuals that are no cancellation; ppo_edge_cases.assert_conditions / assert_gae_conditions)
from the oracle alone before it creates an engine.  No row or element is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest

from tests import ppo_edge_cases as pc
from tests.hip_helpers import flat_params, records, unflat_params

pytestmark = pytest.mark.gpu

F32 = np.float32
ACTOR_TOL = dict(rtol=2e-4, atol=5e-6)
CRITIC_TOL = dict(rtol=2e-4)
PARAM_TOL = dict(rtol=2e-3, atol=2e-5)
ADV_TOL = dict(rtol=1e-4, atol=1e-5)
CADAMW_OUTSIDE = 2e-3
GAUSS_NAMES, AC_NAMES = ["l1", "l2", "mean_layer"], ["l1", "l2", "l3"]
BETA_KEYS = ["l1.weight", "l1.bias", "l2.weight", "l2.bias", "alpha_layer.weight", "beta_layer.weight", "alpha_layer.bias", "beta_layer.bias"]


@pytest.fixture(scope="module")
def N():
    from freerl_amd import _native
    assert _native.device_count() > 0, "no HIP device: the engine has no CPU fallback"
    return _native


# ------------------------------------------------------------------------------------------------ engine side
def actor_flat(c, p):
    if c["kind"] == "beta":
        return np.concatenate([np.asarray(p[k], F32).reshape(-1) for k in BETA_KEYS])
    return flat_params(p, AC_NAMES) if c["kind"] == "cat" else flat_params(p, GAUSS_NAMES, "log_std")


def actor_unflat(c, flat, like):
    if c["kind"] == "beta":
        out, o = {}, 0
        for k in BETA_KEYS:
            out[k] = flat[o:o + like[k].size].reshape(like[k].shape)
            o += like[k].size
        assert o == flat.size
        return out
    return unflat_params(flat, like, AC_NAMES) if c["kind"] == "cat" else unflat_params(flat, like, GAUSS_NAMES, "log_std")


def make_engine(N, c, n_learners=1, with_value=False):
    from freerl_amd.engine import Engine
    disc = c["kind"] == "cat"
    extra = (1 if disc else c["A"]) + 1 + int(with_value)
    return Engine(N.ALGO_PPO, c["O"], c["A"], c["T"], batch_max=c["mb"], extra_cols=extra, discrete=disc, hidden=c["hidden"],
                  hidden_act=N.ACT_TANH if c["tanh"] else N.ACT_RELU, actor_dist=1 if c["kind"] == "beta" else (2 if c["logits"] else 0),
                  n_learners=n_learners)


def add_rows(e, tab, learner=0, with_value=False):
    cols = [tab["logp"]] + ([tab["value"].reshape(-1, 1)] if with_value else []) + [tab["adv_done"].astype(F32).reshape(-1, 1)]
    e.add_batch(records([tab], extra=np.concatenate(cols, axis=1)), learners=np.full(len(tab["rew"]), learner, np.int32))


def load(e, c, inp, learner=0):
    e.set_params(0, actor_flat(c, inp["params"]["actor"]), learner=learner)
    e.set_params(1, flat_params(inp["params"]["critic"], AC_NAMES), learner=learner)
    add_rows(e, inp["table"], learner)


def learn(e, c, perms, **over):
    kw = dict(gamma=pc.GAMMA, lmbda=pc.LMBDA, clip=pc.CLIP, ent_coef=pc.ENT, actor_lr=pc.LR, critic_lr=pc.LR, adv_norm=c["adv_norm"],
              adam_eps=1e-6 if c["c_adamw"] else (1e-5 if c["adam_eps"] else 1e-8), optimizer=int(c["c_adamw"]), want_trace=True, want_adv=True)
    kw.update(over)
    return e.ppo_learn(c["T"], c["mb"], c["K"], perms=perms, **kw)


def result(e, c, out, like, learner=0):
    from freerl_amd import _native
    r = dict(trace=out["trace"][learner].copy(), adv=out["adv"][learner].copy(), v_target=out["v_target"][learner].copy(),
             actor=actor_unflat(c, e.get_params(0, learner=learner), like["actor"]), critic=unflat_params(e.get_params(1, learner=learner), like["critic"], AC_NAMES),
             steps=(e.opt_step(0, learner), e.opt_step(1, learner)), cursor=e.cursor(learner))
    if c["log_std"]:              # a case with a raw log_std past the clamp: the actor's Adam m as well
        r["actor_m"] = actor_unflat(c, e.get_params(0, _native.PARAM_ADAM_M, learner=learner), like["actor"])
    return r


_RUNS = {}


def engine_run(N, c, streaming, monkeypatch):
    """One frl_ppo_learn of the case on a fresh engine, on the on-chip or the streaming kernel; kept for the tests that share it."""
    key = (c["name"], streaming)
    if key not in _RUNS:
        want = pc.oracle_run(c)
        pc.assert_conditions(c, want)
        inp = pc.inputs(c)
        if streaming:
            monkeypatch.setenv("FRL_PPO_STREAMING", "1")
        else:
            monkeypatch.delenv("FRL_PPO_STREAMING", raising=False)
        e = make_engine(N, c)
        load(e, c, inp)
        out = learn(e, c, np.stack(inp["perms"])[None])
        _RUNS[key] = result(e, c, out, want)
        e.close()
    return _RUNS[key]


def assert_close(c, got, ref_trace, ref_actor, ref_critic, label):
    """Loss traces and every parameter of `got` against a reference, at test_ppo_learn's tolerances."""
    n = pc.n_steps(c)
    assert got["trace"].shape == (n, 2), label
    np.testing.assert_allclose(got["trace"][:, 0], ref_trace[0], err_msg=label + " actor loss", **ACTOR_TOL)
    np.testing.assert_allclose(got["trace"][:, 1], ref_trace[1], err_msg=label + " critic loss", **CRITIC_TOL)
    for net, ref in (("actor", ref_actor), ("critic", ref_critic)):
        for k in ref:
            if c["c_adamw"]:
                bad = np.abs(got[net][k] - ref[k]) > (PARAM_TOL["atol"] + PARAM_TOL["rtol"] * np.abs(ref[k]))
                assert bad.mean() < CADAMW_OUTSIDE, (label, net, k, int(bad.sum()), bad.size)
            else:
                np.testing.assert_allclose(got[net][k], ref[k], err_msg="%s %s %s" % (label, net, k), **PARAM_TOL)


def assert_against_oracle(c, got, label):
    want = pc.oracle_run(c)
    n = pc.n_steps(c)
    assert_close(c, got, (want["actor_losses"], want["critic_losses"]), want["actor"], want["critic"], label)
    np.testing.assert_allclose(got["adv"], want["adv"], err_msg=label + " adv", **ADV_TOL)
    np.testing.assert_allclose(got["v_target"], want["v_target"], err_msg=label + " v_target", **ADV_TOL)
    assert got["steps"] == (n, n) and n == c["K"] * -(-c["T"] // c["mb"]), (label, got["steps"])
    assert got["cursor"] == (0, 0), label
    for col, v in c["log_std"] or ():
        # torch.clamp passes no gradient past its bounds: after all n steps the gated column holds the bits that were set and its Adam m is 0,
        # while the interior column has moved
        assert not -20 <= v <= 2, (label, v)
        assert got["actor"]["log_std"][0, col].view(np.uint32) == F32(v).view(np.uint32), (label, "the clamped log_std column moved", got["actor"]["log_std"])
        assert got["actor_m"]["log_std"][0, col] == 0.0, (label, "Adam's m of the clamped log_std column", got["actor_m"]["log_std"])
        others = np.delete(np.arange(c["A"]), [cc for cc, _ in c["log_std"]])
        assert (got["actor"]["log_std"][0, others] != pc.inputs(c)["params"]["actor"]["log_std"][0, others]).all() and got["actor_m"]["log_std"][0, others].all(), label


# ------------------------------------------------------------------------------------------------ (a), (b): the two kernels
case_id = lambda c: c["name"]


@pytest.mark.parametrize("case", pc.ONCHIP, ids=case_id)
def test_onchip_kernel_against_oracle(N, case, monkeypatch):
    assert_against_oracle(case, engine_run(N, case, False, monkeypatch), case["name"] + " on chip")


@pytest.mark.parametrize("case", pc.ONCHIP + pc.STREAMING_ONLY, ids=case_id)
def test_streaming_kernel_against_oracle(N, case, monkeypatch):
    assert_against_oracle(case, engine_run(N, case, True, monkeypatch), case["name"] + " streaming")


@pytest.mark.parametrize("case", pc.ONCHIP, ids=case_id)
def test_the_two_kernels_agree(N, case, monkeypatch):
    a, b = engine_run(N, case, False, monkeypatch), engine_run(N, case, True, monkeypatch)
    assert_close(case, a, (b["trace"][:, 0], b["trace"][:, 1]), b["actor"], b["critic"], case["name"] + " on chip vs streaming")


def test_streaming_only_shapes_take_the_streaming_kernel_unforced(N, monkeypatch):
    """The shapes the on-chip kernel refuses give the same numbers whether or not FRL_PPO_STREAMING is set: bit for bit."""
    for c in pc.STREAMING_ONLY[:2]:
        a, b = engine_run(N, c, True, monkeypatch), engine_run(N, c, False, monkeypatch)
        np.testing.assert_array_equal(a["trace"], b["trace"])
        for k in a["actor"]:
            np.testing.assert_array_equal(a["actor"][k], b["actor"][k])


# ------------------------------------------------------------------------------------------------ (c): horizons and episode ends
def gae_engine_run(N, T, mode1):
    """One engine at horizon T, both learning rates 0, K = 1, mb = T; one learn per adv_done pattern -> {pattern: (adv, v_target)}."""
    g = pc.gae_inputs(T)
    c, inp = g["case"], g["inp"]
    e = make_engine(N, c, with_value=mode1)
    e.set_params(0, actor_flat(c, inp["params"]["actor"]))
    e.set_params(1, flat_params(inp["params"]["critic"], AC_NAMES))
    before = e.get_params(1).copy()
    out = {}
    for name, ad in pc.adv_done_patterns(T).items():
        add_rows(e, dict(inp["table"], adv_done=ad), with_value=mode1)
        o = learn(e, c, np.arange(T)[None, None], actor_lr=0.0, critic_lr=0.0, **(dict(last_value=pc.GAE_LAST_VALUE) if mode1 else {}))
        out[name] = (o["adv"][0].astype(np.float64), o["v_target"][0].astype(np.float64))
        assert e.cursor(0) == (0, 0)
    np.testing.assert_array_equal(e.get_params(1), before)            # learning rate 0: the critic that gave V(s) is the one loaded
    e.close()
    return out


@pytest.mark.parametrize("T", pc.GAE_HORIZONS)
def test_gae_scan_horizons_and_seams(N, T, monkeypatch):
    """ppo_values_kernel + gae_scan: td from the oracle's float32 value forward, then the float64 recurrence; the bound of
    tests/ppo_edge_cases.py on the advantages and on v_target - V(s)."""
    monkeypatch.delenv("FRL_PPO_STREAMING", raising=False)
    pc.assert_gae_conditions(T)
    g = pc.gae_inputs(T)
    got = gae_engine_run(N, T, False)
    for name, ad in pc.adv_done_patterns(T).items():
        A, S = pc.gae_f64(g["td"], ad, pc.gae_c32())
        bound = pc.gae_bound(T, S)
        adv, vt = got[name]
        e1, e2 = np.abs(adv - A), np.abs((vt - g["vs"].astype(np.float64)) - A)
        print("T %d %s: adv err / bound %.3f, (v_target - V) err / bound %.3f" % (T, name, (e1 / bound).max(), (e2 / bound).max()))
        assert (e1 <= bound).all(), (T, name, float((e1 / bound).max()), int((e1 / bound).argmax()))
        assert (e2 <= bound).all(), (T, name, float((e2 / bound).max()), int((e2 / bound).argmax()))


@pytest.mark.parametrize("T", pc.GAE_HORIZONS)
def test_gae_mode_1_horizons_and_seams(N, T, monkeypatch):
    """ppo_gae_sb3_kernel (float64 up to one cast) against BufferForPPO2.compute_returns_and_advantage's formula in float64:
    advantages and returns within 2 ulp of the float32 cast of the float64 result (measured: 0 ulp at every horizon and
    pattern, so the scan's order needs no margin over the 2)."""
    monkeypatch.delenv("FRL_PPO_STREAMING", raising=False)
    tab = pc.gae_inputs(T)["inp"]["table"]
    got = gae_engine_run(N, T, True)
    for name, ad in pc.adv_done_patterns(T).items():
        adv, ret = pc.sb3_f64(tab["rew"], tab["done"], ad, tab["value"], F32(pc.GAE_LAST_VALUE), pc.GAMMA, pc.LMBDA)
        for what, g_, w in (("adv", got[name][0], adv), ("returns", got[name][1], ret)):
            w32 = w.astype(F32)
            ulps = np.abs(g_ - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)
            print("T %d %s %s: %.2f ulp" % (T, name, what, ulps.max()))
            assert (ulps <= 2).all(), (T, name, what, float(ulps.max()), int(ulps.argmax()))


@pytest.mark.parametrize("case", pc.ADV_NORM, ids=case_id)
@pytest.mark.parametrize("streaming", [False, True], ids=["onchip", "streaming"])
def test_adv_norm_through_the_first_actor_loss(N, case, streaming, monkeypatch):
    """(adv - mean) / (std + 1e-8) over a horizon of 2 and of 300 rows (a short last segment): the normalised advantages are
    not returned, the one actor loss of mb = T, K = 1 is."""
    got, want = engine_run(N, case, streaming, monkeypatch), pc.oracle_run(case)
    assert got["trace"].shape == (1, 2) and got["steps"] == (1, 1) and got["cursor"] == (0, 0)
    np.testing.assert_allclose(got["trace"][:, 0], want["actor_losses"], **ACTOR_TOL)
    np.testing.assert_allclose(got["trace"][:, 1], want["critic_losses"], **CRITIC_TOL)
    np.testing.assert_allclose(got["adv"], want["adv"], **ADV_TOL)


def test_frl_gae_dense_sequences(N):
    """frl_gae / gae_dense_kernel through the loaded library on torch device tensors: three sequences of horizon 300 (adv_done on
    the seams, nowhere, everywhere), two of horizon 1; horizon 0, no sequence and a NULL pointer are refused and leave the
    output as it was."""
    import torch
    L = N.lib()
    c = pc.ONCHIP[0]
    e = make_engine(N, c)
    dev = lambda x: torch.tensor(np.ascontiguousarray(x, dtype=F32), device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for T, ads in ((300, [pc.adv_done_patterns(300)[k] for k in ("seams", "none", "all")]), (1, [np.zeros(1, bool), np.ones(1, bool)])):
        d = np.stack([np.random.default_rng(57000 + 10 * T + i).standard_normal(T).astype(F32) for i in range(len(ads))])
        td, ad, out = dev(d), dev(np.stack(ads)), dev(np.full((len(ads), T), 7.0))
        torch.cuda.synchronize()
        assert L.frl_gae(e._h, ptr(td), ptr(ad), len(ads), T, pc.GAMMA, pc.LMBDA, ptr(out)) == 0
        e.sync()
        got = out.cpu().numpy().astype(np.float64)
        for i in range(len(ads)):
            A, S = pc.gae_f64(d[i], ads[i], pc.gae_c32())
            err = np.abs(got[i] - A)
            assert (err <= pc.gae_bound(T, S)).all(), (T, i, float((err / pc.gae_bound(T, S)).max()))
    T = 300
    td, ad, out = dev(np.zeros((3, T))), dev(np.zeros((3, T))), dev(np.full((3, T), 7.0))
    torch.cuda.synchronize()
    null = C.c_void_p(None)
    for args in ((ptr(td), ptr(ad), 3, 0, ptr(out)), (ptr(td), ptr(ad), 0, T, ptr(out)), (null, ptr(ad), 3, T, ptr(out)), (ptr(td), null, 3, T, ptr(out)),
                 (ptr(td), ptr(ad), 3, T, null)):
        assert L.frl_gae(e._h, args[0], args[1], args[2], args[3], pc.GAMMA, pc.LMBDA, args[4]) == 1           # FRL_ERR_INVALID
    e.sync()
    np.testing.assert_array_equal(out.cpu().numpy(), np.full((3, T), 7.0, F32))
    e.close()


# ------------------------------------------------------------------------------------------------ (d): population
@pytest.mark.parametrize("streaming", [False, True], ids=["onchip", "streaming"])
def test_population_of_three_against_their_oracles(N, streaming, monkeypatch):
    """n_learners = 3 at (a)'s first shape, each learner with its own table, parameters and permutations: every learner equals
    its own oracle, its advantages and value targets included."""
    cs = pc.POPULATION
    for c in cs:
        pc.assert_conditions(c)
    if streaming:
        monkeypatch.setenv("FRL_PPO_STREAMING", "1")
    else:
        monkeypatch.delenv("FRL_PPO_STREAMING", raising=False)
    e = make_engine(N, cs[0], n_learners=len(cs))
    for p, c in enumerate(cs):
        load(e, c, pc.inputs(c), learner=p)
    out = learn(e, cs[0], np.stack([np.stack(pc.inputs(c)["perms"]) for c in cs]))
    for p, c in enumerate(cs):
        assert_against_oracle(c, result(e, c, out, pc.oracle_run(c), learner=p), "learner %d" % p)
    assert not np.array_equal(out["trace"][0], out["trace"][1]) and not np.array_equal(out["trace"][1], out["trace"][2])
    e.close()
