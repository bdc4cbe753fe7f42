"""Float64 reference of the Categorical DQN target projection (DQN_with_tricks.py:134-158), written as the textbook
per-row loop (Bellemare et al. 2017, Algorithm 1) and independent of oracle/algos.py's vectorised float32 restatement."""
import numpy as np


def project(next_dist, rew, done, gamma, atoms, vmin, vmax):
    """next_dist [B, atoms], rew [B], done [B], gamma -> m [B, atoms], all float64.

    Source atom j of row r sits at z_j = vmin + j dz; its target T = clip(rew_r + gamma (1 - done_r) z_j, vmin, vmax) has the
    fractional bin position b = (T - vmin) / dz.  Its mass next_dist[r, j] is split linearly between floor(b) and ceil(b),
    and is left whole on the bin when T lands on one or is clamped to an end of the support."""
    p = np.asarray(next_dist, np.float64)
    rew = np.asarray(rew, np.float64).reshape(-1)
    done = np.asarray(done, np.float64).reshape(-1)
    gamma, vmin, vmax = float(gamma), float(vmin), float(vmax)
    B = p.shape[0]
    assert p.shape == (B, atoms) and rew.shape == (B,) and done.shape == (B,)
    dz = (vmax - vmin) / (atoms - 1)
    m = np.zeros((B, atoms), np.float64)
    for r in range(B):
        for j in range(atoms):
            z = vmin + j * dz
            T = min(max(rew[r] + gamma * (1.0 - done[r]) * z, vmin), vmax)
            b = min(max((T - vmin) / dz, 0.0), float(atoms - 1))
            lo, hi = int(np.floor(b)), int(np.ceil(b))
            if lo == hi:
                m[r, lo] += p[r, j]
            else:
                m[r, lo] += p[r, j] * (hi - b)
                m[r, hi] += p[r, j] * (b - lo)
    return m
