"""Inputs shared by tests/test_c51_projection.py (CPU) and tests/test_gpu_c51_edges.py (GPU): the supports, and a
transition table whose rewards and dones walk the Categorical projection's edges."""
import numpy as np

from tests.golden import synth

F32 = np.float32
GAMMA = 0.99

# (atoms, vmin, vmax): the reference's own support; dz = 0.4 not representable; three whose fp32 quotient
# (vmax - vmin) / dz is atoms - 1 plus one ulp (and whose LDS row pitch equals atoms); every lane live; the two smallest
SUPPORTS = [(51, -100.0, 100.0), (51, -10.0, 10.0), (16, -500.0, 500.0), (24, -7.0, 7.0), (28, -50.0, 100.0),
            (64, -10.0, 10.0), (2, 0.0, 1.0), (3, -1.0, 1.0)]
OVERSHOOT = [(16, -500.0, 500.0), (24, -7.0, 7.0), (28, -50.0, 100.0)]

KINDS = ["on_atom_0", "on_atom_top", "on_atom_mid", "half_way", "all_clamp_hi", "all_clamp_lo", "top_few_clamp", "gaussian"]
N_REPEAT = 6                           # structured rows: N_REPEAT of each kind but the last, then the Gaussian rest


def structured_rewards(atoms, vmin, vmax, gamma=GAMMA):
    """kind -> (reward, done) of one structured row; see structured_table."""
    z = np.linspace(vmin, vmax, atoms, dtype=np.float64).astype(F32).astype(np.float64)      # the float32 atoms
    width, dz = vmax - vmin, (vmax - vmin) / (atoms - 1)
    j = (atoms - 1) // 2
    k = min(3, atoms - 1)              # atoms that clamp to vmax in a "top_few_clamp" row
    return {
        "on_atom_0": (z[0], 1), "on_atom_top": (z[-1], 1), "on_atom_mid": (z[atoms // 2], 1),      # (a) l == u
        "half_way": (0.5 * (z[j] + z[j + 1]), 1),                                                  # (b)
        "all_clamp_hi": (vmax + 1.5 * width, 0), "all_clamp_lo": (vmin - 1.5 * width, 1),          # (c) every atom at one end
        # (d) done = 0: r + gamma z_i >= vmax exactly for the top k atoms (the threshold sits half a bin below atom atoms - k)
        "top_few_clamp": (vmax - gamma * (vmax - (k - 0.5) * dz), 0),
    }


def structured_table(seed, n_tab, obs_dim, n_actions, atoms, vmin, vmax, gamma=GAMMA):
    """A seeded transition table (tests/golden/synth.py) with rewards and dones overwritten: rows [i * 7, i * 7 + 7) for i <
    N_REPEAT are one row of each structured kind (kinds (c) swap their done flags on odd i), the rest are Gaussian rewards
    spread over the support (e).  Returns (table, {kind: row indices})."""
    n_struct = N_REPEAT * (len(KINDS) - 1)
    assert n_tab > n_struct + 8
    tab = synth.transitions(seed, n_tab, obs_dim, 1, n_discrete=n_actions)
    rew = (tab["rew"].astype(np.float64) * 0.15 * (vmax - vmin) + 0.5 * (vmax + vmin))
    done = tab["done"].copy()
    sr = structured_rewards(atoms, vmin, vmax, gamma)
    rows = {kd: [] for kd in KINDS}
    for i in range(N_REPEAT):
        for c, kd in enumerate(KINDS[:-1]):
            r = i * (len(KINDS) - 1) + c
            rew[r], done[r] = sr[kd][0], bool(sr[kd][1])
            if kd.startswith("all_clamp") and i % 2:
                done[r] = not done[r]
            rows[kd].append(r)
    rows["gaussian"] = list(range(n_struct, n_tab))
    tab["rew"], tab["done"] = rew.astype(F32), done
    return tab, rows


def batch_indices(seed, rows, n_tab, batch, call):
    """`batch` distinct rows for learn call `call`.  From 8 rows up: one row of every kind (another repeat each call), the rest
    drawn from the whole table.  Below that a batch cannot hold every kind: "top_few_clamp" (the common case) comes first,
    then the other kinds in an order rotated by the call, so three calls of 5 rows still meet every kind; a batch of ONE
    row is "top_few_clamp", "on_atom_top", "half_way" in turn."""
    g = np.random.default_rng(seed + 1000 * call)
    others = [kd for kd in KINDS if kd != "top_few_clamp"]
    order = ["top_few_clamp"] + [others[(c + 4 * call) % len(others)] for c in range(len(others))]
    if batch == 1:
        order = [["top_few_clamp", "on_atom_top", "half_way"][call % 3]]
    first = [rows[kd][(call + seed) % len(rows[kd])] for kd in order][:batch]
    rest = [r for r in np.argsort(g.random(n_tab), kind="stable") if r not in first]
    idx = np.array(first + rest[:batch - len(first)], dtype=np.int64)
    assert len(set(idx.tolist())) == batch
    return idx[np.argsort(g.random(batch), kind="stable")]            # no kind tied to a row position
