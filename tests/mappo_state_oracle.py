"""NumPy restatement of MAPPO_file/MAPPO_for_mask_action_state.py: what it changes in MAPPO_for_mask_action.py's `learn` (:308-396),
i.e. the critic's input [all observations | state] in the value pass (:322-323) and in the critic's step (:371-373), in float32 where
torch is.  Everything else is tests/mappo_mask_oracle.py's and tests/mappo_oracle.py's.  Test infrastructure: the seeded cases and the
toy environment below are what tests/golden/make_mappo_state_golden.py runs the imported reference on, what
tests/test_mappo_state_oracle.py checks this file against and what tests/test_gpu_mappo_state.py runs the kernels on.

Kept as the reference has it (DESIGN.md "MAPPO_for_mask_action_state"): V(s) = critic([obs | state]) and V(s') = critic([next_obs |
state]) with the SAME state row; in the critic's step `obs_` is indexed by the shuffled permutation and `state` is not, so row r of the
one minibatch is [obs[perm[r]] | state[r]] regressed on v_target[perm[r]] (`state_rows="position"`).  `state_rows="sample"` is the
pairing the reference meant, [obs[perm[r]] | state[perm[r]]]; it has no reference golden.  Rows never written have a zero state.
"""
import numpy as np

from oracle.nn import F32
from tests import mappo_mask_oracle as mm
from tests import mappo_oracle as mo

DIMS = mm.DIMS                           # obs_total 14: state_dim 2 fills a 16-column tile exactly, 3 opens a second tile
STATE_DIM = 7
# The golden maker requires the first critic loss to tell the two pairings, and a dropped state block, apart by > 1e-3 relative for
# every agent of every case.  With unit rewards the value targets dwarf what a freshly initialised critic puts out (loss about 16) and
# a unit state moves that loss by about 1e-3: rewards a tenth the size and states three times the observations' make it tens of per cent
STATE_SCALE = 3.0
REWARD_SCALE = 0.1


def _case(cont, tricks, state_dim=STATE_DIM, **kw):
    c = mm._case(cont, tricks, **dict(dict(reward_scale=REWARD_SCALE), **kw))
    c.update(state_dim=state_dim, state_rows="position")
    return c


CASES = {
    "plain": _case(False, False, seed=81),
    # all tricks: the input LayerNorm runs over both segments; Huber delta 0.5 straddled as in the masked `tricks`
    "tricks": _case(False, True, huber_delta=0.5, reward_scale=0.25, reward_same=True, seed=82),
    "partial": _case(False, False, trick=dict(mo.TRICKS_OFF, adv_norm=True), fill=27, seed=83),      # 13 rows never written: zero state
    "stale": _case(False, True, second=18, seed=84),               # learn, 18 new rows (and states) over the old ones, learn again
    "cont": _case(True, True, seed=85),                            # continuous actors: the masks never read, the state used
    # 3 x (18, 11) + 45 = 99 input columns, hidden 128
    "wide": _case(False, True, state_dim=45, dims=((18, 11),) * 3, hidden=128, horizon=64, k_epochs=1, seed=86),
    # the width edges on 14 observation columns
    "sd1": _case(False, True, state_dim=1, seed=87),
    "sd2": _case(False, False, state_dim=2, seed=88),              # 16 input columns: no padding column
    "sd3": _case(False, True, state_dim=3, seed=89),               # 17: the first column of a second tile
    "sd23": _case(False, False, state_dim=23, seed=90),            # the state wider than all observations
}
FULL_CASES = ("plain", "tricks", "partial", "stale", "cont", "sd1", "sd2", "sd3", "sd23")


def case(name, **kw):
    return dict(CASES[name], name=name, **kw)


def critic_width(c):
    return sum(o for o, _ in c["dims"]) + c["state_dim"]


def inputs(c, seed=None):
    """mappo_mask_oracle.inputs with critics whose first layer is obs_total + state_dim wide, and `state` [T][state_dim]: i.i.d. normal
    rows from a generator of their own, so distinct from every observation"""
    seed = c["seed"] if seed is None else seed
    inp = mm.inputs(c, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 3000))
    H = c["hidden"]
    inp["critics"] = [mo.net_params(rng, mo.CRITIC, [(H, critic_width(c)), (H, H), (1, H)]) for _ in c["dims"]]
    inp["state"] = rng.normal(0, STATE_SCALE, (c["horizon"], c["state_dim"])).astype(F32)
    return inp


calls, perms = mm.calls, mm.perms


def ring_state(c, inp):
    fill = c["horizon"] if c["fill"] is None else c["fill"]
    s = np.zeros_like(inp["state"])
    s[:fill] = inp["state"][:fill]
    return s


def second_rows(c):
    """-> (rows per agent, states) added after the first learn()"""
    inp = inputs(c, seed=c["seed"] + 500)
    return [{k: v[:c["second"]] for k, v in r.items()} for r in inp["rows"]], inp["state"][:c["second"]]


class Oracle(mm.Oracle):
    def __init__(self, c, inp):
        super().__init__(c, inp)
        self.state = ring_state(c, inp)

    def add(self, new_rows, new_state):
        super().add(new_rows)
        self.state[:len(new_state)] = new_state

    def critic_obs(self, i, key="obs", ix=slice(None)):
        obs = np.concatenate([r[key][ix] for r in self.rows], axis=1)
        if isinstance(ix, slice) or self.c["state_rows"] == "sample":
            st = self.state[ix]                  # the value pass (both V(s) and V(s')), or the sampled rows' states
        else:
            # (:373) `state` is the whole buffer, not indexed: it lines up with obs_[index] only as one minibatch of the whole capacity
            assert len(ix) == self.c["horizon"], "torch.cat raises: the minibatch is not the whole capacity"
            st = self.state
        return np.concatenate([obs, st], axis=1).astype(F32)


def run(c, inp=None, perm=None, calls_max=None, zero_state=False):
    """-> the oracle after the case's learn() calls; o.trace [n][calls * K * n_mb][2], o.adv_raw / o.v_target of the LAST call"""
    inp = inputs(c) if inp is None else inp
    perm = perms(c) if perm is None else perm
    o = Oracle(c, inp)
    if zero_state:
        o.state[:] = 0
    traces = [o.learn(perm[0])]
    if c["second"] and (calls_max is None or calls_max > 1):
        o.add(*second_rows(c))
        traces.append(o.learn(perm[1]))
    o.trace = np.concatenate(traces, axis=1)
    return o


# ------------------------------------------------------------------------------------------------ the episode run
# tests/mappo_mask_oracle.py's toy environment with a get_state(): a function of the step alone, from a generator of its own
LOOP = _case(False, True, horizon=16, seed=91)
LOOP_EPISODES, LOOP_HYPER = mm.LOOP_EPISODES, mm.LOOP_HYPER


class ToyEnv(mm.ToyEnv):
    def __init__(self, c=LOOP, seed=None):
        super().__init__(c, seed)
        rng = np.random.Generator(np.random.PCG64((c["seed"] if seed is None else seed) + 9500))
        self.state = rng.normal(0, 1, (sum(LOOP_EPISODES) + 1, c["state_dim"])).astype(F32)

    def get_state(self):
        return self.state[self.t]


def run_loop(algo, env, on_step=None):
    """mappo_mask_oracle.run_loop with the script's `state = env.get_state()` before the step (:661) handed to add (:696-698)"""
    acts, lps = [], []
    for ep_len in LOOP_EPISODES:
        for s in range(ep_len):
            obs, avail = env.observe()
            state = env.get_state()
            if on_step is not None:
                on_step(obs, avail)
            action, logp = algo.select_action(obs, avail)
            nobs, rew, done = env.step(action, s == ep_len - 1)
            algo.add(obs, action, rew, nobs, done, logp, done, avail, state)
            acts.append([int(np.asarray(action[a]).reshape(-1)[0]) for a in env.agents])
            lps.append([float(np.asarray(logp[a]).reshape(-1)[0]) for a in env.agents])
        algo.learn(LOOP["horizon"], LOOP_HYPER["gamma"], LOOP_HYPER["lmbda"], LOOP_HYPER["clip"], LOOP_HYPER["k_epochs"], LOOP_HYPER["ent_coef"],
                   LOOP_HYPER["huber_delta"])
    return np.array(acts, np.int64), np.array(lps, np.float64)
