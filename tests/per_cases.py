"""Cases shared by tests/test_per_cases.py (CPU) and tests/test_gpu_per_edges.py (GPU): prioritised replay (kernels_per.hip,
the PER entry points of frl_api.hip) at its population, batch and capacity edges.

`build(name)` plays one case on the oracle's PERBuffer / SumTree (oracle/buffer.py, the reference's DQN_file/Buffer.py:66-194
restated), ONE ORACLE PER LEARNER, and returns the script a device test replays: a list of steps, each with what goes in and
what the reference left behind.

    {"op": "add",    "recs": f32 [n, width], "learners": i32 [n],          "sum": [P], "max": [P], "exact": bool}
    {"op": "sample", "u": f64 [P, batch],    "idx": i64 [P, batch], "w": f32 [P, batch], "beta": float}
    {"op": "update", "idx": i64 [P, batch],  "td": f32 [P, batch],         "sum": [P], "max": [P], "exact": False}

"exact" says that no TD error has entered any tree yet: every priority is 1.0 and the sums are small integers.

Uniforms are drawn by rejection against the reference tree alone: u[i] is redrawn while any comparison `s <= tree[left]` of its
descent has |s - tree[left]| < MARGIN * tree[0].  MARGIN = 1e-6 is derived, not measured: the device computes priorities with
powf, one float32 ulp from NumPy's (which is why sums and maxima are held to rtol 1e-6), and that moves any partial sum and
the segment start by at most 2^-23 * total each, 2.4e-7 of the total together; the margin is four times that.  Rejected draws
are capped at 2 % of all draws of a case (asserted here).  The two cases with hand-placed uniforms say why they are exempt.

The conditions a case is there for (a leaf sampled three times with different TD errors, duplicate pairs inside and across a
group of four batch positions, a duplicated leaf whose last entry is the batch's last row, a ring that wraps, learners whose
index sets differ) are asserted here, on the reference's run only."""
import functools

import numpy as np

from oracle.buffer import PERBuffer
from tests.golden import synth
from tests.hip_helpers import records

F32 = np.float32
MARGIN = 1e-6
REJECT_CAP = 0.02
OBS = 3
ALPHA, BETA, BETA_INC, EPSILON = 0.6, 0.4, 0.001, 0.01
PER_SET_MAX = 4096                      # kPerSetMax (csrc/kernels.h): rows of one priority update

# `require`: the conditions build() asserts for the case ("triple", "within4", "across4", "last_dup", "wrap", "differ")
ALL = ("triple", "within4", "across4", "last_dup", "wrap", "differ")
CASES = {
    # leaves on two tree levels; batch no multiple of four, smaller than the pitch and LARGER than the capacity
    "two_level": dict(capacity=37, P=3, batch_max=64, batch=61, sigma=2.5, rounds=4, seed=4101, require=ALL),
    "one_level": dict(capacity=64, P=2, batch_max=64, batch=64, sigma=1.0, rounds=4, seed=4206, require=("triple", "wrap", "differ")),
    # four trips per thread in per_sample_kernel (the last one ragged), n > 256 and a long later-entry scan in per_set_kernel
    "strided": dict(capacity=1000, P=5, batch_max=1024, batch=1021, sigma=2.5, rounds=4, seed=4301, require=ALL),
    # kPerSetMax rows in one update; the first add_batch fills the ring, more rows than one flush stages (two per_add launches);
    # the second round samples the skewed tree
    "set_max": dict(capacity=5000, P=1, batch_max=PER_SET_MAX, batch=PER_SET_MAX, sigma=2.5, rounds=2, seed=4401, first=1.0,
                    require=("triple", "within4", "across4", "wrap")),
    "tiny1": dict(capacity=1, P=1, batch_max=4, batch=4, sigma=2.5, rounds=4, seed=4501, require=("wrap",)),
    "tiny2": dict(capacity=2, P=1, batch_max=4, batch=4, sigma=2.5, rounds=4, seed=4502, require=("wrap",)),
    "tiny3": dict(capacity=3, P=1, batch_max=4, batch=4, sigma=2.5, rounds=4, seed=4503, require=("wrap",)),
    "interleaved_adds": dict(capacity=50, P=4, batch_max=16, batch=16, sigma=1.5, seed=4601, script="interleaved", require=("wrap", "differ")),
    "prob_clip": dict(capacity=256, P=1, batch_max=8, batch=8, sigma=1.0, seed=4701, script="prob_clip", require=()),
    "ties": dict(capacity=64, P=1, batch_max=16, batch=16, sigma=1.0, seed=4801, script="ties", require=()),
}


# ------------------------------------------------------------------------------------------------ the reference tree, read only
def descent_clearance(tree, s):
    """(min |s - tree[left]| over the comparisons of SumTree.get(s), min of |s - tree[left]| / tree[left])."""
    node, n, clear, rel = 0, len(tree), np.inf, np.inf
    while True:
        left = 2 * node + 1
        if left >= n:
            return clear, rel
        t = tree[left]
        clear = min(clear, abs(s - t))
        rel = min(rel, abs(s - t) / t if t > 0 else np.inf)
        if s <= t:
            node = left
        else:
            s -= t
            node = left + 1


def margin_uniform(tree, batch, i, g):
    """The margin rule for stratum i of `batch` on a reference tree: (u, draws it took)."""
    total, seg = tree[0], tree[0] / batch
    a, b = seg * i, seg * (i + 1)
    tries = 0
    while True:
        u = g.random()
        tries += 1
        if descent_clearance(tree, a + (b - a) * u)[0] >= MARGIN * total:
            return u, tries


def margin_uniforms(tree, batch, g):
    """One batch of uniforms by the margin rule: (u [batch], draws, rejected)."""
    got = [margin_uniform(tree, batch, i, g) for i in range(batch)]
    draws = sum(t for _, t in got)
    return np.array([u for u, _ in got]), draws, draws - batch


def leaf_intervals(tree, capacity):
    """buffer index -> (start, end) of its leaf's share of the total mass in DESCENT order (left to right through the array
    heap, which on a tree with leaves on two levels is not buffer order)."""
    out, acc, stack = {}, 0.0, [0]
    while stack:
        node = stack.pop()
        left = 2 * node + 1
        if left >= len(tree):
            out[node - capacity + 1] = (acc, acc + tree[node])
            acc += tree[node]
        else:
            stack.append(left + 1)
            stack.append(left)
    return out


def duplicate_facts(idx, td):
    """What one learner's batch of leaves gives per_set_kernel's later-entry scan to get wrong."""
    idx = np.asarray(idx)
    B = len(idx)
    where = {}
    for i, v in enumerate(idx):
        where.setdefault(int(v), []).append(i)
    f = dict(triple=False, within4=False, across4=False, last_dup=False)
    for v, pos in where.items():
        if len(pos) >= 3 and len({float(td[i]) for i in pos}) == len(pos):
            f["triple"] = True
        for a in range(len(pos)):
            vec0 = (pos[a] + 1 + 3) & ~3              # where entry pos[a]'s scan turns from single words to groups of four
            for b in range(a + 1, len(pos)):
                f["within4" if pos[b] < vec0 else "across4"] = True
        if len(pos) >= 2 and pos[-1] == B - 1:
            f["last_dup"] = True
    return f


# ------------------------------------------------------------------------------------------------ playing a case
class _Play:
    def __init__(self, name, c):
        self.name, self.c = name, c
        self.P, self.cap, self.B = c["P"], c["capacity"], c["batch"]
        self.orc = [PERBuffer(self.cap, OBS, 1, ALPHA, BETA, BETA_INC, EPSILON) for _ in range(self.P)]
        self.g = np.random.default_rng(c["seed"])
        n_tab = 4 * self.cap + 200          # every learner its own table, longer than any script hands over
        self.tabs = [synth.transitions(c["seed"] * 100 + p, n_tab, OBS, 1, n_discrete=3) for p in range(self.P)]
        self.recs, self.used = [records([t]) for t in self.tabs], [0] * self.P
        self.steps, self.draws, self.rejected, self.td_seen = [], 0, 0, False
        self.facts = {k: False for k in ALL}
        self.facts["differ"] = self.P > 1
        self.last_idx = None

    def _row(self, p):
        i = self.used[p]
        assert i < len(self.recs[p])
        self.used[p] += 1
        return i

    def _state(self):
        return [o.sumtree.sum() for o in self.orc], [o.sumtree.max() for o in self.orc]

    def add(self, order):
        """One add_batch call: `order` is the learner of every row, in the order the rows are handed over."""
        order = np.asarray(order, np.int32)
        rows = []
        for p in order:
            i = self._row(int(p))
            t = self.tabs[p]
            self.orc[p].add(t["obs"][i], t["act"][i], float(t["rew"][i]), t["next_obs"][i], bool(t["done"][i]))
            rows.append(self.recs[p][i])
        s, m = self._state()
        self.steps.append(dict(op="add", recs=np.stack(rows), learners=order, sum=s, max=m, exact=not self.td_seen))

    def shuffled(self, counts):
        order = np.concatenate([np.full(n, p, np.int32) for p, n in enumerate(counts)])
        return order[np.argsort(self.g.random(len(order)), kind="stable")]

    def alternating(self, counts):
        left, order = list(counts), []
        while any(left):
            for p in range(len(left)):
                if left[p]:
                    order.append(p)
                    left[p] -= 1
        return np.asarray(order, np.int32)

    def draw(self, p, fixed=None, exempt=None):
        """Uniforms of one learner's batch, by the margin rule on its reference tree.  fixed: {row: u} placed by hand;
        exempt: None, or the rule those rows are held to instead ("relative" / "integers")."""
        tree = self.orc[p].sumtree.tree
        total, seg = tree[0], tree[0] / self.B
        u = np.zeros(self.B)
        for i in range(self.B):
            a, b = seg * i, seg * (i + 1)
            if fixed is not None and i in fixed:
                u[i] = fixed[i]
                clear, rel = descent_clearance(tree, a + (b - a) * u[i])
                if exempt == "relative":          # far from every node it is compared with, measured on that node
                    assert rel >= 1e-3, (self.name, i, rel)
                elif exempt == "integers":        # every sum and every s is a small integer: exact in both trees
                    assert np.all(tree == np.round(tree)) and (a + (b - a) * u[i]) == round(a + (b - a) * u[i])
                else:
                    assert clear >= MARGIN * total, (self.name, i, clear)
                continue
            u[i], tries = margin_uniform(tree, self.B, i, self.g)
            self.draws += tries
            self.rejected += tries - 1
        return u

    def sample(self, fixed=None, exempt=None):
        us, idxs, ws = [], [], []
        for p in range(self.P):
            u = self.draw(p, fixed, exempt)
            idx, w = self.orc[p].sample_with(u)
            us.append(u); idxs.append(idx); ws.append(w)
        idxs = np.stack(idxs)
        if self.P > 1:
            self.facts["differ"] &= all(not np.array_equal(idxs[p], idxs[q]) for p in range(self.P) for q in range(p))
        self.last_idx = idxs
        self.steps.append(dict(op="sample", u=np.stack(us), idx=idxs, w=np.stack(ws), beta=float(self.orc[0].beta)))
        return idxs

    def lognormal_td(self, scale=None):
        td = np.exp(self.c["sigma"] * self.g.standard_normal((self.P, self.B))) * np.where(self.g.random((self.P, self.B)) < 0.5, -1.0, 1.0)
        if scale is not None:
            td = td * np.asarray(scale, np.float64).reshape(-1, 1)
        return td.astype(F32)

    def update(self, td=None, idx=None, count_facts=True):
        idx = self.last_idx if idx is None else np.asarray(idx, np.int64)
        td = self.lognormal_td() if td is None else np.asarray(td, F32)
        for p in range(self.P):
            self.orc[p].update_priorities(idx[p], td[p])
            if count_facts:
                for k, v in duplicate_facts(idx[p], td[p]).items():
                    self.facts[k] |= v
        self.td_seen = True
        s, m = self._state()
        self.steps.append(dict(op="update", idx=idx.copy(), td=td, sum=s, max=m, exact=False))

    def finish(self):
        c = self.c
        self.facts["wrap"] = all(n > self.cap for n in self.used)
        for k in c["require"]:
            assert self.facts[k], "case %s: the reference's run does not show %r" % (self.name, k)
        assert self.rejected <= REJECT_CAP * max(self.draws, 1), (self.name, self.rejected, self.draws)
        cursor = [(o.buffer._index, len(o)) for o in self.orc]
        return dict(name=self.name, P=self.P, capacity=self.cap, batch_max=c["batch_max"], batch=self.B, steps=self.steps,
                    cursor=cursor, draws=self.draws, rejected=self.rejected, facts=dict(self.facts))


def _standard(pl):
    """Uneven first adds, then `rounds` of sample, update, more adds; the learners' rows of one call are shuffled together."""
    c, P, cap = pl.c, pl.P, pl.cap
    pl.add(pl.shuffled([min(cap, max(1, int(c.get("first", 0.7) * cap)) + 3 * p) for p in range(P)]))
    for _ in range(c["rounds"]):
        pl.sample()
        pl.update()
        pl.add(pl.shuffled([cap // 5 + 1 + p for p in range(P)]))


def _interleaved(pl):
    """per_add_kernel's three per-learner branches and the host's counting sort of one flush by learner."""
    P, cap, B = pl.P, pl.cap, pl.B
    pl.add(pl.alternating([20, 13, 7, 0]))                 # rows alternate learners, uneven counts; learner 3: no rows in this flush
    # updated priorities before learner 3 has a row.  An update names `batch` leaves of EVERY learner: learner 3's all name
    # leaf 0 of its still empty tree with TD error 0 (priority 0.01^0.6 < 1), which its first add overwrites with 1.0 —
    # so its fill is 1.0 on the device (no rows before this flush) as in the reference (len(buffer) == 0).
    idx = np.stack([pl.g.integers(0, n, B) for n in (20, 13, 7)] + [np.zeros(B, np.int64)])
    td = pl.lognormal_td(scale=[1.0, 3.0, 9.0, 0.0])
    pl.update(td=td, idx=idx, count_facts=False)
    pl.add(pl.alternating([5, 0, 4, 9]))                   # 3: first rows ever (1.0); 0 and 2: each its own current max; 1: none
    assert len({round(m, 9) for m in pl.steps[-1]["max"]}) == P, "the learners' maxima must differ for the fill to show"
    pl.sample(); pl.update()
    pl.add(pl.alternating([3, 45, 2, 4]))                  # 1 holds 13 of 50 rows: 45 more wrap inside one flush
    pl.sample(); pl.update()
    pl.add(pl.alternating([2, 1, cap + 7, 3]))             # 2: more than `capacity` rows in a single call
    pl.sample(); pl.update()
    pl.add(pl.shuffled([cap, cap, 1, cap]))                # (so that every ring has wrapped)
    pl.sample(); pl.update()


def _prob_clip(pl):
    """per_sample_kernel's 1e-7 probability clip.  u[0] = 1e-12 is placed by hand; in the second round it lands s = 2e-7 on
    leaf 0 (priority 0.063) under a total of 1.8e6, closer than MARGIN * total to every sum on its way — but 0.063 and more
    below each of them, which no one-ulp change of a priority (1.2e-7 RELATIVE on every node, its segment start exactly 0)
    can bridge: that row is held to `s` staying 1e-3 of the node away from every node it is compared with instead."""
    B = pl.B
    pl.add(np.zeros(pl.cap, np.int32))
    idx = pl.sample(fixed={0: 1e-12})                      # all priorities 1.0: stratum i lands inside leaves [32 i, 32 i + 32)
    assert idx[0, 0] == 0 and np.all(idx[0, 1:] > 0)
    td = np.full((1, B), 1e9, F32)
    td[0, 0] = 0.0
    pl.update(td=td)
    tree = pl.orc[0].sumtree
    raw = float(F32(tree.tree[pl.cap - 1])) / tree.sum()
    assert raw < 1e-7, "leaf 0's probability %g is not under the clip" % raw
    idx = pl.sample(fixed={0: 1e-12}, exempt="relative")
    assert idx[0, 0] == 0
    pl.update()
    pl.sample(); pl.update()


def _ties(pl):
    """The `s <= left` tie rule: 64 leaves at 1.0, 16 strata, every u = 0, so s = 4 i exactly and `<=` keeps leaf 4 i - 1 (leaf
    0 for i = 0).  EXEMPT from the margin rule on purpose: every sum on the way and every s is a small integer, exact in the
    reference's incremental tree and in one that adds children — the tie itself is what is tested."""
    pl.add(np.zeros(pl.cap, np.int32))
    idx = pl.sample(fixed={i: 0.0 for i in range(pl.B)}, exempt="integers")
    np.testing.assert_array_equal(idx[0], np.maximum(4 * np.arange(pl.B) - 1, 0))
    pl.update()


_SCRIPTS = dict(interleaved=_interleaved, prob_clip=_prob_clip, ties=_ties)


@functools.lru_cache(maxsize=None)
def build(name):
    c = CASES[name]
    pl = _Play(name, c)
    _SCRIPTS.get(c.get("script"), _standard)(pl)
    return pl.finish()
