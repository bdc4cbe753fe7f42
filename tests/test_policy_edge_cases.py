"""CPU tier of the policy edge cases (tests/policy_edge_cases.py): the conditions that tests/test_gpu_policy_edges.py relies on hold for
every case, from the float64 reference and the float32 oracle alone; the float64 reference restates the project's oracle (it agrees with
oracle.algos.SAC / TD3 on the interior parity cases); the case list reaches every (shape, family) pair it names; and every near miss of
device/policy.hpp that the GPU test is there to catch (policy_edge_cases.MUTATIONS), computed in float64, breaks one of the GPU test's
assertions on the cases it bears on — by a wide margin, so that a kernel with that mistake cannot pass."""
import numpy as np
import pytest

from tests import policy_edge_cases as pc

case_id = lambda c: c["name"]


@pytest.mark.parametrize("case", pc.ALL_CASES, ids=case_id)
def test_input_conditions(case):
    pc.assert_conditions(case)


@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_reference_restates_the_oracle_on_the_interior_parity_cases(kind):
    """tests.golden.cases.CASES["sac"] / ["td3"] (batch 256, alpha 0.01, nothing clamps): the float32 oracle within 0.25 of every
    tolerance of the float64 reference, after every call."""
    sp = pc.golden_spec(kind)
    ref, orc = pc.run_reference(sp), pc.run_oracle(sp)
    assert ref["steps"] == orc["steps"]
    used = pc.shares(orc, ref)
    print(kind, "losses %.3f alpha %.3f parameters %.3f of the tolerance" % used)
    assert max(used) <= pc.ORACLE_SHARE, used


def test_measured_fractions_are_recorded():
    """policy_edge_cases.MEASURED (and the module's docstring) against what the cases give today."""
    worst = {k: [0.0, 0.0, 0.0] for k in pc.MEASURED}
    for c in pc.ALL_CASES:
        group = "td3" if c["algo"] == "td3" else ("sac-satmean" if c["layout"] == "satmean" else "sac-clamp")
        used = pc.shares(pc.oracle_run(c["name"]), pc.reference_run(c["name"]))
        worst[group] = [max(a, b) for a, b in zip(worst[group], used)]
    for group, rec in pc.MEASURED.items():
        print(group, ["%.3f" % w for w in worst[group]], "recorded", rec)
        assert all(w <= r <= pc.ORACLE_SHARE for w, r in zip(worst[group], rec)), (group, worst[group], rec)


def test_case_list_reaches_every_shape_family_batch_and_layout():
    fams = {(c["shape"], f) for c, f in pc.PAIRS}
    assert fams == {("narrow", "rowchunk"), ("narrow", "chained"), ("narrow", "solo"), ("wide", "rowchunk"), ("wide", "ksliced"), ("wide", "solow"),
                    ("h256", "rowchunk"), ("h256", "xstationary"), ("head2", "rowchunk"), ("head2", "ksliced"), ("head2", "solow"),
                    ("head2h256", "rowchunk"), ("head2h256", "xstationary")}
    for algo, shapes in (("sac", ("narrow", "wide", "h256", "head2", "head2h256")), ("td3", ("narrow", "wide", "h256"))):
        assert {c["shape"] for c in pc.ALL_CASES if c["algo"] == algo} == set(shapes)
        assert {c["batch"] for c in pc.ALL_CASES if c["algo"] == algo} == {17, 64}
    assert {c["layout"] for c in pc.SAC_CASES} == {"upper", "lower", "mixed", "seam", "tdiff", "satmean"}
    assert [c["layout"] for c in pc.POPULATION] == ["upper", "lower", "interior"] and len({c["seed"] for c in pc.POPULATION}) == 3
    # the seam layout: gated and on-bound columns either side of the 16-column head tile's seam
    closed, on_bound = pc.gate_columns("sac-head2-seam-b17")
    assert np.flatnonzero(closed).tolist() == [0, 16, 19] and np.flatnonzero(on_bound).tolist() == [3, 15]
    # tdiff: each copy is interior where the other is clamped
    for name in ("sac-narrow-tdiff-b64", "sac-wide-tdiff-b64"):
        sp = pc.spec(name)
        out = lambda ls: ((ls < pc.LS_MIN) | (ls > pc.LS_MAX)).reshape(-1)
        on, tg = out(sp["actor"]["log_std"]), out(sp["actor_t"]["log_std"])
        assert on.any() and tg.any() and not (on & tg).any(), name
    for c in pc.ALL_CASES:                       # every set value is what float32 holds
        for k in ("actor", "actor_t"):
            assert all(v.dtype == np.float32 for v in pc.spec(c["name"])[k].values())


def test_zero_noise_makes_the_lower_edge_exact():
    """u == mean on the lower-edge columns, so the first Adam step of the open column at -20 is +lr to rounding (its gradient is -alpha
    times the clip factor), and the closed one stays where it was set."""
    ref = pc.reference_run("sac-narrow-lower-b64")
    raw = pc.spec("sac-narrow-lower-b64")["actor"]["log_std"].astype(np.float64).reshape(-1)
    after = ref["calls"][0]["actor"]["log_std"].reshape(-1)
    assert abs((after[0] - raw[0]) - pc.LR) < 1e-6 * pc.LR and after[1] == raw[1] == -21.0
    assert ref["calls"][0]["actor_m"]["log_std"].reshape(-1)[0] < 0 and ref["calls"][0]["actor_m"]["log_std"].reshape(-1)[1] == 0.0


def test_unzeroed_noise_on_the_lower_edge_is_the_number_formats():
    """Why the noise is zeroed there: with it, the float32 oracle itself is past the parameter tolerance against float64."""
    sp = pc._spec("sac-narrow-lower-b64", zero_noise=False)
    used = pc.shares(pc.run_oracle(sp), pc.run_reference(sp))
    print("unzeroed: losses %.2f alpha %.2f parameters %.2f of the tolerance" % used)
    assert max(used) > 1.0, used


# which cases a mutation bears on, and the GPU assertion that it breaks
def _loss_share(mut, ref):
    return max(pc.share(mut["critic_loss"], ref["critic_loss"], pc.LOSS_RTOL), pc.share(mut["actor_loss"], ref["actor_loss"], pc.LOSS_RTOL, pc.ACTOR_LOSS_ATOL))


@pytest.mark.parametrize("case", [c for c in pc.ALL_CASES if c["algo"] == "sac" and pc.gate_columns(c["name"])[1].any()], ids=case_id)
def test_mutation_gate_strict_leaves_the_bound_columns_where_they_were(case):
    """`>` / `<` for `>=` / `<=`: the columns at exactly 2.0 / -20.0 never move and their Adam m stays 0 — the GPU test asserts that
    they have moved by 0.5 .. 1.5 lr after the first call and that m is not 0."""
    _, on_bound = pc.gate_columns(case["name"])
    mut = pc.run_reference(pc.spec(case["name"]), "gate-strict")
    raw = pc.spec(case["name"])["actor"]["log_std"].reshape(-1)
    for call in mut["calls"]:
        assert (call["actor"]["log_std"].reshape(-1)[on_bound] == raw[on_bound]).all() and not call["actor_m"]["log_std"].reshape(-1)[on_bound].any()


@pytest.mark.parametrize("case", [c for c in pc.ALL_CASES if c["algo"] == "sac" and pc.gate_columns(c["name"])[0].any()], ids=case_id)
def test_mutation_gate_removed_moves_the_closed_columns(case):
    """No gate: the columns at 2.5 / -21.0 move by about lr in the first call and their Adam m and v are not 0 — the GPU test asserts
    bit-equality with what was set and exact zeros."""
    closed, _ = pc.gate_columns(case["name"])
    mut = pc.run_reference(pc.spec(case["name"]), "gate-removed")
    raw = pc.spec(case["name"])["actor"]["log_std"].reshape(-1)
    first = mut["calls"][0]
    assert (np.abs(first["actor"]["log_std"].reshape(-1)[closed] - raw[closed]) > 0.5 * pc.LR).all()
    assert first["actor_m"]["log_std"].reshape(-1)[closed].all() and first["actor_v"]["log_std"].reshape(-1)[closed].all()


def _target_clamped(c):
    if c["algo"] != "sac":
        return False
    ls = pc.spec(c["name"])["actor_t"]["log_std"]
    return bool(((ls < pc.LS_MIN) | (ls > pc.LS_MAX)).any())


@pytest.mark.parametrize("case", [c for c in pc.ALL_CASES if _target_clamped(c)], ids=case_id)
def test_mutation_target_pass_without_the_clamp_leaves_the_loss_tolerance(case):
    ref, mut = pc.reference_run(case["name"]), pc.run_reference(pc.spec(case["name"]), "target-unclamped")
    used = pc.share(mut["critic_loss"][:1], ref["critic_loss"][:1], pc.LOSS_RTOL)
    print(case["name"], "first critic loss: %.0f x the tolerance" % used)
    assert used > 10, (case["name"], used)


@pytest.mark.parametrize("case", pc.TD3_CASES, ids=case_id)
def test_mutation_clip_before_scale_leaves_the_loss_tolerance(case):
    """The smoothing noise changes by at most 0.1 of an action's range of 4 and the rewards dominate the TD target, so the critic losses
    leave their tolerance by single factors only (1.2 .. 7 x); the critic's gradient carries the difference into every parameter through
    Adam, and the parameters leave theirs by two orders of magnitude."""
    ref, mut = pc.reference_run(case["name"]), pc.run_reference(pc.spec(case["name"]), "clip-before-scale")
    loss, _, param = pc.shares(mut, ref)
    print(case["name"], "losses %.1f x, parameters %.0f x the tolerance" % (loss, param))
    assert loss > 1 and param > 100, (case["name"], loss, param)


@pytest.mark.parametrize("case", [c for c in pc.SAC_CASES if c["layout"] == "satmean"], ids=case_id)
def test_mutation_softplus_threshold_zero_leaves_the_loss_tolerance(case):
    ref, mut = pc.reference_run(case["name"]), pc.run_reference(pc.spec(case["name"]), "softplus-threshold-zero")
    used = min(pc.share(mut[k][:1], ref[k][:1], pc.LOSS_RTOL) for k in ("critic_loss", "actor_loss", "alpha_loss"))
    print(case["name"], "first critic / actor / alpha loss: at least %.0f x the tolerance" % used)
    assert used > 10, (case["name"], used)


def test_wrong_copy_in_a_pass_leaves_the_loss_tolerance():
    """tdiff: a target pass that reads the online log_std (or an online pass that reads the target's) is the reference run on a spec
    whose copies are swapped — the first critic loss (target pass) and the first actor loss (online pass) both leave the tolerance."""
    for name in ("sac-narrow-tdiff-b64", "sac-wide-tdiff-b64"):
        sp = dict(pc.spec(name))
        ref = pc.reference_run(name)
        for which, key in (("actor_t", "critic_loss"), ("actor", "actor_loss")):
            other = "actor" if which == "actor_t" else "actor_t"
            sw = dict(sp)
            sw[which] = dict(sp[which], log_std=sp[other]["log_std"])
            used = pc.share(pc.run_reference(sw)[key][:1], ref[key][:1], pc.LOSS_RTOL, pc.ACTOR_LOSS_ATOL if key == "actor_loss" else 0.0)
            assert used > 10, (name, which, used)
