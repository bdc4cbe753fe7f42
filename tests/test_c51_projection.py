"""The Categorical DQN target projection of the float32 oracle (oracle/algos.py: C51DQN.project, what the HIP kernel is
compared with) against a float64 textbook loop (tests/c51_reference.py), on every support of tests/c51_cases.py and on
rows that sit on the projection's edges: targets exactly on an atom, half way between two, clamped at either end of the
support, and the common `done = 0` row whose top atoms clamp to v_max.

On the three OVERSHOOT supports the float32 quotient (v_max - v_min) / delta_z is atoms - 1 plus one ulp; the reference's
index_add_ raises IndexError there and so did the oracle until it clamped the quotient."""
import numpy as np
import pytest

from oracle import algos
from tests import c51_cases, c51_reference
from tests.golden import synth

F32 = np.float32
O, NA, N_TAB = 6, 3, 96

# Worst |m_fp32 - m_fp64| over every case below, measured on x86-64: 3.85e-6 (64 atoms on [-10, 10]; the reference's own
# support gives 1.4e-6, two and three atoms 1e-7).  That is the size reasoning gives: a bin's weight is b - floor(b) with
# b <= atoms - 1 carrying a few float32 roundings (z_i, gamma z_i, + r, - v_min, / delta_z), i.e. an absolute error of about
# (atoms - 1) 2^-24 = 3.8e-6 at 64 atoms, times a mass <= 1; summing 64 such terms adds less.  Asserted at 4x the
# measurement so that last-bit changes in NumPy do not flip it.
MEASURED_GAP = 3.85e-6
TOL = 4 * MEASURED_GAP


def next_dists(seed, n, atoms):
    """Float32 distributions: softmaxes of Gaussian logits at three temperatures, and every fourth row all its mass on one
    atom (walking the support, ends included)."""
    g = np.random.default_rng(seed)
    lg = g.standard_normal((n, atoms)) * np.array([0.3, 2.0, 6.0])[np.arange(n) % 3, None]
    e = np.exp(lg - lg.max(axis=1, keepdims=True))
    d = (e / e.sum(axis=1, keepdims=True)).astype(F32)
    for r in range(0, n, 4):
        d[r] = 0
        d[r, [0, atoms - 1, atoms // 2, (r // 4) % atoms][(r // 4) % 4]] = 1
    return d


def case(atoms, vmin, vmax):
    tab, rows = c51_cases.structured_table(7, N_TAB, O, NA, atoms, vmin, vmax)
    q = synth.mlp_params(11, [("l1", 128, O), ("l2", NA * atoms, 128)])
    pol = algos.C51DQN(q, O, NA, 1e-3, N_TAB, atoms, vmin, vmax)
    return pol, tab, rows, next_dists(13, N_TAB, atoms)


@pytest.mark.parametrize("atoms,vmin,vmax", c51_cases.SUPPORTS)
def test_oracle_projection_matches_float64(atoms, vmin, vmax):
    pol, tab, rows, nd = case(atoms, vmin, vmax)
    rew, done = tab["rew"].astype(F32).reshape(-1, 1), tab["done"].astype(F32).reshape(-1, 1)
    m = pol.project(nd, rew, done, c51_cases.GAMMA)
    assert m.dtype == F32 and m.shape == (N_TAB, atoms)
    # the same inputs in float64: the float32 rewards, distributions and discount, the exact support
    want = c51_reference.project(nd.astype(np.float64), rew, done, float(F32(c51_cases.GAMMA)), atoms, vmin, vmax)
    # rows sum to 1: next_dist does within atoms 2^-24, each source's two weights sum to 1, and the 2 atoms accumulations
    # of a row round partial sums <= 1
    sums = m.astype(np.float64).sum(axis=1)
    print("atoms %d [%g, %g]: worst |sum - 1| %.3g" % (atoms, vmin, vmax, np.abs(sums - 1).max()))
    assert np.abs(sums - 1).max() <= 4 * atoms * 2.0 ** -24
    gap = np.abs(m.astype(np.float64) - want).max()
    print("atoms %d [%g, %g]: worst |fp32 - fp64| %.3g" % (atoms, vmin, vmax, gap))
    assert gap <= TOL, gap
    # the edges are what they are meant to be, in the float64 reference itself
    top, bot = want[:, -1], want[:, 0]
    for r in rows["on_atom_top"] + rows["all_clamp_hi"]:
        assert top[r] == pytest.approx(nd[r].astype(np.float64).sum(), abs=1e-12)
    for r in rows["on_atom_0"] + rows["all_clamp_lo"]:
        assert bot[r] == pytest.approx(nd[r].astype(np.float64).sum(), abs=1e-12)
    k = min(3, atoms - 1)
    # (float32 rewards: the structured targets sit within a few (atoms - 1) 2^-24 bins of where they were put)
    for r in rows["top_few_clamp"]:                   # the top k sources land whole on the top atom, the next one half a bin below
        p = nd[r].astype(np.float64)
        assert top[r] == pytest.approx(p[atoms - k:].sum() + (1 - 0.5 * c51_cases.GAMMA) * p[atoms - k - 1], abs=1e-5)
    for r in rows["half_way"]:
        j = (atoms - 1) // 2
        assert want[r, j] == pytest.approx(0.5 * nd[r].astype(np.float64).sum(), abs=1e-5)


@pytest.mark.parametrize("atoms,vmin,vmax", c51_cases.OVERSHOOT)
def test_overshoot_supports_do_overshoot_in_float32(atoms, vmin, vmax):
    """The premise of the clamp: on these supports the float32 quotient of a target at v_max exceeds atoms - 1, so an
    unclamped ceil indexes one past the support (the reference's IndexError)."""
    dz = F32(F32(vmax) - F32(vmin)) / F32(atoms - 1)
    b = F32(F32(vmax) - F32(vmin)) / dz
    assert b > F32(atoms - 1) and int(np.ceil(b)) == atoms
    ref = (51, -100.0, 100.0)
    assert F32(F32(ref[2]) - F32(ref[1])) / (F32(F32(ref[2]) - F32(ref[1])) / F32(ref[0] - 1)) == F32(ref[0] - 1)


def test_projection_is_what_learn_with_uses():
    """learn_with calls project(): a learn step on a support that overshoots runs, and its loss is finite."""
    atoms, vmin, vmax = c51_cases.OVERSHOOT[1]
    pol, tab, rows, _ = case(atoms, vmin, vmax)
    for i in range(N_TAB):
        pol.add(tab["obs"][i], tab["act"][i], float(tab["rew"][i]), tab["next_obs"][i], bool(tab["done"][i]))
    loss = pol.learn_with(np.arange(N_TAB), c51_cases.GAMMA, 0.01)
    assert np.isfinite(loss)
