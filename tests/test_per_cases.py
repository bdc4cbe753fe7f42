"""CPU checks of tests/per_cases.py, the cases tests/test_gpu_per_edges.py replays on the device: the conditions every case
is there for hold on the reference's run, rejected uniforms stay under the cap, and the margin rule does what it is for — a
tree of the device's kind (every touched ancestor recomputed from its children, kernels_per.hip's per_repair) whose every
TD-derived priority sits one float32 ulp above or below the reference's draws the same indices from the same uniforms."""
import numpy as np
import pytest

from tests import per_cases

F32 = np.float32
NAMES = list(per_cases.CASES)


class ChildSumTree:
    """The device's trees in NumPy: a sum-tree and a max-tree of the reference's shape, leaves written first, then every
    ancestor of a written leaf recomputed from its two children, deepest level first."""

    def __init__(self, capacity):
        self.cap, self.nn = capacity, 2 * capacity - 1
        self.sum, self.max = np.zeros(self.nn), np.zeros(self.nn)

    def write(self, leaves, values):
        touched = set()
        for li, v in zip(leaves, values):              # in order: a later entry for the same leaf wins
            node = int(li) + self.cap - 1
            self.sum[node] = self.max[node] = v
            while node:
                node = (node - 1) // 2
                touched.add(node)
        for node in sorted(touched, reverse=True):     # children before parents
            l, r = 2 * node + 1, 2 * node + 2
            self.sum[node] = self.sum[l] + (self.sum[r] if r < self.nn else 0.0)
            self.max[node] = max(self.max[l], self.max[r] if r < self.nn else 0.0)

    def get(self, s):
        node = 0
        while 2 * node + 1 < self.nn:
            l = 2 * node + 1
            if s <= self.sum[l]:
                node = l
            else:
                s -= self.sum[l]
                node = l + 1
        return node - self.cap + 1


def replay_indices(case, ulp_seed):
    """The case's adds, uniforms and TD errors on ChildSumTrees with one-ulp-off priorities -> the indices of every sample."""
    P, cap, B = case["P"], case["capacity"], case["batch"]
    g = np.random.default_rng(ulp_seed)
    trees = [ChildSumTree(cap) for _ in range(P)]
    cursor, size, out = [0] * P, [0] * P, []
    for st in case["steps"]:
        if st["op"] == "add":
            for p in range(P):
                n = int(np.sum(st["learners"] == p))
                if n == 0:
                    continue
                fill = 1.0 if size[p] == 0 else trees[p].max[0]
                leaves = [(cursor[p] + k) % cap for k in range(n)]
                trees[p].write(leaves, [fill] * n)
                cursor[p], size[p] = (cursor[p] + n) % cap, min(cap, size[p] + n)
        elif st["op"] == "sample":
            idx = np.zeros((P, B), np.int64)
            for p in range(P):
                seg = trees[p].sum[0] / B
                for i in range(B):
                    a, b = seg * i, seg * (i + 1)
                    idx[p, i] = trees[p].get(a + (b - a) * st["u"][p, i])
            out.append(idx)
        else:
            for p in range(P):
                pr = (np.abs(st["td"][p]) + F32(per_cases.EPSILON)) ** F32(per_cases.ALPHA)
                assert pr.dtype == F32
                off = np.where(g.random(B) < 0.5, F32(-np.inf), F32(np.inf))
                trees[p].write(st["idx"][p], np.nextafter(pr, off).astype(np.float64))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions_and_rejection_cap(name):
    case = per_cases.build(name)                       # (build asserts the same; a case edited into passing nothing fails here)
    for k in per_cases.CASES[name]["require"]:
        assert case["facts"][k], (name, k)
    assert case["rejected"] <= per_cases.REJECT_CAP * max(case["draws"], 1)
    samples = [s for s in case["steps"] if s["op"] == "sample"]
    assert samples and all(s["idx"].shape == (case["P"], case["batch"]) for s in samples)
    for s in samples:
        assert np.all(s["idx"] >= 0) and np.all(s["idx"] < case["capacity"])
        np.testing.assert_array_equal(s["w"].max(axis=1), 1.0)
    assert case["batch"] <= case["batch_max"] and case["batch"] <= per_cases.PER_SET_MAX


def test_the_named_cases_reach_the_scan_and_the_clip():
    for name in ("two_level", "strided"):
        f = per_cases.build(name)["facts"]
        assert all(f[k] for k in per_cases.ALL), (name, f)
    # batch 61 ends a ragged group of four below a pitch of 64; 1021 is four trips of 256 threads, the last one ragged
    assert per_cases.CASES["two_level"]["batch"] % 4 and per_cases.CASES["strided"]["batch"] > 3 * 256
    assert per_cases.CASES["set_max"]["batch"] == per_cases.PER_SET_MAX
    clip = [s for s in per_cases.build("prob_clip")["steps"] if s["op"] == "sample"][1]
    assert clip["idx"][0, 0] == 0 and clip["w"][0, 0] == 1.0      # the clipped row carries the largest weight
    ties = [s for s in per_cases.build("ties")["steps"] if s["op"] == "sample"][0]
    np.testing.assert_array_equal(ties["idx"][0], [0] + [4 * i - 1 for i in range(1, 16)])


@pytest.mark.parametrize("name", NAMES)
def test_a_child_sum_tree_one_ulp_off_draws_the_same_indices(name):
    case = per_cases.build(name)
    want = [s["idx"] for s in case["steps"] if s["op"] == "sample"]
    for ulp_seed in (1, 2):
        got = replay_indices(case, ulp_seed)
        assert len(got) == len(want)
        for k, (g_, w_) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(g_, w_, err_msg="%s, sample %d, perturbation %d" % (name, k, ulp_seed))


def test_oracle_per_row_weights():
    """oracle.algos.DQN.learn_with(is_weight=w, per_row=True), the oracle of the engine's per = 2: loss = mean(w_i td_i^2); with
    every weight equal it gives the broadcast arithmetic's loss (per_row=False); with one row's weight at zero that row stops
    mattering — the step equals, bit for bit, the one taken with that row's reward changed."""
    from oracle import algos
    from tests.golden import synth
    O, nA, n, B = 5, 3, 40, 24
    prm = synth.mlp_params(8101, [("l1", 128, O), ("l2", nA, 128)])

    def learner(rew0=None):
        tab = synth.transitions(8102, n, O, 1, n_discrete=nA)
        if rew0 is not None:
            tab["rew"][0] = rew0
        orc = algos.DQN(prm, O, nA, 1e-3, n)
        for i in range(n):
            orc.add(tab["obs"][i], tab["act"][i][0], float(tab["rew"][i]), tab["next_obs"][i], bool(tab["done"][i]))
        return orc
    idx = np.arange(B)
    w = np.random.default_rng(8103).uniform(0.2, 1.0, B).astype(F32)
    a = learner()
    loss = a.learn_with(idx, 0.99, 0.01, double=True, is_weight=w, per_row=True)
    td = learner()
    td.learn_with(idx, 0.99, 0.01, double=True)
    np.testing.assert_allclose(loss, np.mean(w.astype(np.float64) * td.last_td.astype(np.float64) ** 2), rtol=1e-6)
    flat_w = np.full(B, 0.625, F32)
    b, c = learner(), learner()
    # (the same float32 products, summed as [B] here and as [B, B] there: a few ulps)
    np.testing.assert_allclose(b.learn_with(idx, 0.99, 0.01, is_weight=flat_w, per_row=True), c.learn_with(idx, 0.99, 0.01, is_weight=flat_w), rtol=1e-6)
    w0 = w.copy()
    w0[0] = 0.0
    d, e = learner(), learner(rew0=7.0)
    assert d.learn_with(idx, 0.99, 0.01, is_weight=w0, per_row=True) == e.learn_with(idx, 0.99, 0.01, is_weight=w0, per_row=True)
    for k in d.q:
        np.testing.assert_array_equal(d.q[k], e.q[k])
    assert any(not np.array_equal(a.q[k], d.q[k]) for k in a.q)
