"""CPU tier of the PPO edge cases (tests/ppo_edge_cases.py): the conditions on the inputs that tests/test_gpu_ppo_edges.py relies
on hold for every case, from the oracle alone; and a float32 scan in gae_scan's order of operations meets the GAE error
bound at every horizon and adv_done pattern the GPU tests use, so a correct kernel can."""
import numpy as np
import pytest

from tests import ppo_edge_cases as pc


@pytest.mark.parametrize("case", pc.ALL_CASES + pc.ADV_NORM, ids=lambda c: c["name"])
def test_input_conditions(case):
    pc.assert_conditions(case)


def test_case_shapes_reach_the_edges_they_name():
    a = {c["name"]: c for c in pc.ONCHIP}
    sizes = lambda c: [min(c["mb"], c["T"] - s) for s in range(0, c["T"], c["mb"])]
    assert sizes(a["relu-8-2-100-24"]) == [24, 24, 24, 24, 4]
    assert sizes(a["relu-16-1-70-64"]) == [64, 6]
    assert sizes(a["relu-17-16-150-70"]) == [70, 70, 10]
    assert sizes(a["relu-32-5-130-129"]) == [129, 1]
    for c in pc.ALL_CASES:
        assert pc.n_steps(c) <= 10, c["name"]                      # at most 10 Adam steps per net


def test_stored_log_probs_follow_the_policy():
    """The log-ratio of the first minibatch has the perturbation's spread (sd 0.3), whatever the head's width."""
    for name in ("relu-16-1-70-64", "relu-17-16-150-70", "cat-4-16-100-24"):
        lr = np.log(pc.oracle_run(pc.BY_NAME[name])["log"][0][0].astype(np.float64))
        assert 0.15 < lr.std() < 0.45, (name, lr.std())


@pytest.mark.parametrize("T", pc.GAE_HORIZONS)
def test_scan_emulation_meets_the_gae_bound(T):
    from oracle import ppo as oppo
    pc.assert_gae_conditions(T)
    g = pc.gae_inputs(T)
    c = pc.gae_c32()
    for name, ad in pc.adv_done_patterns(T).items():
        assert (ad != g["inp"]["table"]["done"]).any(), name          # truncation: done and adv_done differ somewhere
        A, S = pc.gae_f64(g["td"], ad, c)
        got = pc.gae_scan_f32(g["td"], ad.astype(np.float32), c)
        err = np.abs(got.astype(np.float64) - A)
        assert (err <= pc.gae_bound(T, S)).all(), (T, name, float((err / pc.gae_bound(T, S)).max()))
        # the project's sequential float32 oracle is a correct scan too
        seq = oppo.gae(g["td"], ad.astype(np.float32), pc.GAMMA, pc.LMBDA)
        assert (np.abs(seq.astype(np.float64) - A) <= pc.gae_bound(T, S)).all(), (T, name)


def test_scan_emulation_of_frl_gae_sequences():
    """The dense sequences of the frl_gae test: horizon 300 with the seam pattern, and horizon 1."""
    for T, ads in ((300, [pc.adv_done_patterns(300)[k] for k in ("seams", "none", "all")]), (1, [np.zeros(1, bool), np.ones(1, bool)])):
        for i, ad in enumerate(ads):
            d = np.random.default_rng(57000 + 10 * T + i).standard_normal(T).astype(np.float32)
            A, S = pc.gae_f64(d, ad, pc.gae_c32())
            err = np.abs(pc.gae_scan_f32(d, ad.astype(np.float32), pc.gae_c32()).astype(np.float64) - A)
            assert (err <= pc.gae_bound(T, S)).all(), (T, i)


def test_sb3_formula_is_the_oracle_buffers():
    """sb3_f64 restates BufferForPPO2.compute_returns_and_advantage: equal to it to float64 rounding."""
    T = 300
    g = pc.gae_inputs(T)
    tab = dict(g["inp"]["table"], adv_done=pc.adv_done_patterns(T)["seams"])
    orc = pc.new_oracle(g["case"], g["inp"]["params"], rollout_values=True)
    pc.fill(orc, tab, values=tab["value"])
    orc.buffer.compute_returns_and_advantage(pc.GAMMA, pc.LMBDA, pc.GAE_LAST_VALUE)
    adv, ret = pc.sb3_f64(tab["rew"], tab["done"], tab["adv_done"], tab["value"], pc.GAE_LAST_VALUE, pc.GAMMA, pc.LMBDA)
    np.testing.assert_allclose(orc.buffer.advantages, adv, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(orc.buffer.returns, ret, rtol=1e-13, atol=1e-15)
