"""GPU: what the host API decides per algorithm, pinned for every algorithm at once.

Two characterisations of the host API's algorithm table (kAlgo, csrc/engine_plan.hpp), both recorded from the commit before the table existed:

* the refusal matrix: every engine kind x every entry point that serves only some kinds.  REFUSALS holds the return code of each
  pair as a literal; a refused call names the entry point that was called and the one that serves the engine, and launches nothing;
* the create-time decisions: LDS bytes and row chunk, record layout, nets and parameter counts, learn path of every accepted
  configuration against tests/golden/algo_matrix.json, and the code + wording of every refused one.

The same golden is checked without a GPU by tests/test_engine_plan.py (csrc/engine_plan.hpp through a stand-alone probe): the
configurations (_configs) and the comparison (assert_matches_golden) are shared.

`python tests/test_gpu_algo_matrix.py --record [PATH]` re-records the golden (on a GPU; only when a layout is changed on purpose)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "algo_matrix.json")
SMALL = dict(capacity=40, hidden=32, batch_max=32)

# engine kind -> (algo, obs_dim, act_dim, Engine keywords, the entry point that updates it); the smallest shapes of the suite
ENGINES = {
    "dqn": ("ALGO_DQN", 4, 3, dict(discrete=True), "frl_learn"),
    "ddpg": ("ALGO_DDPG", 4, 3, {}, "frl_learn"),
    "td3": ("ALGO_TD3", 4, 3, dict(twin_critic=True), "frl_learn"),
    "sac": ("ALGO_SAC", 4, 3, dict(twin_critic=True), "frl_learn"),
    "maddpg": ("ALGO_MADDPG", [4, 4], [3, 3], {}, "frl_learn"),
    "ppo": ("ALGO_PPO", 4, 3, dict(extra_cols=4), "frl_ppo_learn"),
    "sacd": ("ALGO_SAC_DISCRETE", 4, 3, dict(twin_critic=True), "frl_learn"),
    "reinforce": ("ALGO_REINFORCE", 4, 3, {}, "frl_reinforce_learn"),
    "envelope_dqn": ("ALGO_ENVELOPE_DQN", 4, 3, dict(discrete=True, reward_dim=2), "frl_envelope_learn"),
    "envelope_ddpg": ("ALGO_ENVELOPE_DDPG", 4, 3, dict(reward_dim=2), "frl_envelope_ddpg_learn"),
    "gail": ("ALGO_GAIL", 4, 3, {}, "frl_gail_learn"),
    # two agents, continuous: extra_cols = 3 + 2 log-prob columns + 2 adv_done columns
    "mappo": ("ALGO_MAPPO", [4, 5], [3, 2], dict(extra_cols=7), "frl_mappo_learn"),
    "ippo": ("ALGO_IPPO", [4, 5], [3, 2], dict(extra_cols=7), "frl_mappo_learn"),
    "happo": ("ALGO_HAPPO", [4, 5], [3, 2], dict(extra_cols=7), "frl_happo_learn"),
}
ACT_TANH, ACT_LEAKY_RELU = 2, 3          # enum frl_activation
ENTRIES = ("frl_learn", "frl_learn_path", "frl_learn_work", "frl_learn_work_executed", "frl_ppo_learn", "frl_ppo_rollout",
           "frl_reinforce_learn", "frl_envelope_learn", "frl_envelope_ddpg_learn", "frl_rollout", "frl_act_explore")
# Return codes (0 FRL_OK, 1 FRL_ERR_INVALID, 4 FRL_ERR_STATE), one row per engine kind, columns in ENTRIES' order.
# "R4" / "R1": refused because of the engine's algorithm, with that code.  A bare number: the pair is served (or, frl_rollout with
# its NULL pool, the argument check comes first) and the call ends there, in the validation of the deliberately unusable arguments
# _call() passes, before anything is launched.  "S4": frl_act_explore's single-agent rule, not a matter of the algorithm.
REFUSALS = {
    #                 learn  path  work  w_exe  ppo_l  ppo_r  reinf  env    env_dd roll   explore
    "dqn":           (1,     0,    0,    0,     "R4",  "R4",  "R4",  "R4",  "R4",  1,     1),
    "ddpg":          (1,     0,    0,    0,     "R4",  "R4",  "R4",  "R4",  "R4",  1,     1),
    "td3":           (1,     0,    0,    0,     "R4",  "R4",  "R4",  "R4",  "R4",  1,     1),
    "sac":           (1,     0,    0,    0,     "R4",  "R4",  "R4",  "R4",  "R4",  1,     1),
    "maddpg":        (1,     0,    0,    0,     "R4",  "R4",  "R4",  "R4",  "R4",  1,     "S4"),
    "ppo":           ("R4",  "R1", 0,    0,     1,     1,     "R4",  "R4",  "R4",  1,     1),
    "sacd":          (1,     0,    0,    0,     "R4",  "R4",  "R4",  "R4",  "R4",  "R4",  "R4"),
    "reinforce":     ("R4",  "R4", "R4", "R4",  "R4",  "R4",  1,     "R4",  "R4",  "R4",  "R4"),
    "envelope_dqn":  ("R4",  "R4", "R4", "R4",  "R4",  "R4",  "R4",  1,     "R4",  "R4",  "R4"),
    "envelope_ddpg": ("R4",  "R4", "R4", "R4",  "R4",  "R4",  "R4",  "R4",  1,     "R4",  "R4"),
}

# create-time configurations beyond ENGINES: name -> (engine kind it varies, obs_dim, act_dim, keywords over SMALL and the kind's own)
TWO_WG = ("sacd", "reinforce", "envelope_dqn", "envelope_ddpg")          # row chunks at two workgroups per CU
VARIANTS = {}
for _k in TWO_WG:
    VARIANTS[_k + "/hidden512"] = (_k, 4, 3, dict(hidden=512))
    VARIANTS[_k + "/hidden40"] = (_k, 4, 3, dict(hidden=40))
    VARIANTS[_k + "/reward_dim-1"] = (_k, 4, 3, dict(reward_dim=-1))
    VARIANTS[_k + "/columns"] = (_k, 4, 13 if _k == "envelope_dqn" else 65, dict(reward_dim=5))      # 13 x 5, or 65, > kSacdMaxActions
    VARIANTS[_k + "/obs1000"] = (_k, 1000, 3, dict(hidden=256))
VARIANTS["sac/wide_input"] = ("sac", 376, 17, dict(hidden=256))           # Humanoid's 393 critic columns: 16 rows bumped to 32
VARIANTS["gail/leaky_relu"] = ("gail", 4, 3, dict(hidden_act=ACT_LEAKY_RELU))
VARIANTS["gail/tanh"] = ("gail", 4, 3, dict(hidden_act=ACT_TANH))
VARIANTS["sac/leaky_relu"] = ("sac", 4, 3, dict(hidden_act=ACT_LEAKY_RELU))
VARIANTS["sac/two_agents"] = ("sac", [4, 4], [3, 3], {})
VARIANTS["dqn/c51_atoms65"] = ("dqn", 4, 3, dict(c51=(65, -10.0, 10.0)))
for _k in ("mappo", "ippo", "happo"):
    VARIANTS[_k + "/discrete"] = (_k, None, None, dict(discrete=True, extra_cols=4))          # 2 log-prob + 2 adv_done columns
    VARIANTS[_k + "/hidden272"] = (_k, None, None, dict(hidden=272))
    VARIANTS[_k + "/tanh"] = (_k, None, None, dict(hidden_act=ACT_TANH))
    VARIANTS[_k + "/twin_critic"] = (_k, None, None, dict(twin_critic=True))
    VARIANTS[_k + "/extra_cols"] = (_k, None, None, dict(extra_cols=6))
VARIANTS["mappo/masks"] = ("mappo", None, None, dict(discrete=True, extra_cols=9))               # ... + 3 + 2 mask columns
VARIANTS["mappo/state"] = ("mappo", None, None, dict(state_dim=6, extra_cols=13))                # 5 + 2 + 6 state columns
VARIANTS["mappo/state_discrete"] = ("mappo", None, None, dict(discrete=True, state_dim=6, extra_cols=10))
VARIANTS["mappo/state_masks"] = ("mappo", None, None, dict(discrete=True, state_dim=6, extra_cols=15))
VARIANTS["mappo/state_sample_rows"] = ("mappo", None, None, dict(state_dim=6, state_rows=1, extra_cols=13))
VARIANTS["mappo/state_extra_cols"] = ("mappo", None, None, dict(state_dim=6, extra_cols=7))
VARIANTS["mappo/state_lds"] = ("mappo", None, None, dict(state_dim=3000, extra_cols=3007))     # a first layer of 3009 columns
VARIANTS["ippo/state"] = ("ippo", None, None, dict(state_dim=6, extra_cols=13))
VARIANTS["ppo/discrete"] = ("ppo", 4, 3, dict(discrete=True))
VARIANTS["ppo/beta"] = ("ppo", 4, 3, dict(actor_dist=1))
VARIANTS["ppo/logits"] = ("ppo", 4, 3, dict(discrete=True, actor_dist=2))
VARIANTS["ppo/tanh"] = ("ppo", 4, 3, dict(hidden_act=ACT_TANH))
# the kernel families of frl_learn (hidden 128, batches of 256 unless said) at the populations where one hands over to the next
NARROW, WIDE, MADDPG = ("td3", 8, 2), ("td3", 17, 6), ("maddpg", [18] * 3, [5] * 3)
FAMILY = dict(hidden=128, batch_max=256)
for _p in (1, 16, 17, 32, 33, 128, 129):
    VARIANTS["narrow/P%d" % _p] = NARROW + (dict(FAMILY, n_learners=_p),)
for _p in (16, 17, 129):
    VARIANTS["wide/P%d" % _p] = WIDE + (dict(FAMILY, n_learners=_p),)
for _p in (176, 177):
    VARIANTS["wide256/P%d" % _p] = WIDE + (dict(FAMILY, hidden=256, n_learners=_p),)
VARIANTS["sac/wide_input128"] = ("sac", 376, 17, dict(FAMILY))
for _b, _p in ((1024, 1), (1024, 2), (128, 5), (128, 6), (128, 43)):
    VARIANTS["maddpg/B%d_P%d" % (_b, _p)] = MADDPG + (dict(hidden=128, batch_max=_b, n_learners=_p),)
VARIANTS["dqn/fused"] = ("dqn", 8, 4, dict(FAMILY))
VARIANTS["dqn/rainbow"] = ("dqn", 8, 4, dict(FAMILY, dueling=True, noisy=True, c51=(51, -10.0, 10.0)))
# ... and under the knobs frl_create reads (`env`: set around the create)
VARIANTS["knob/assume_cus40"] = WIDE + (dict(FAMILY, n_learners=3, env=dict(FRL_ASSUME_CUS="40")),)
VARIANTS["knob/solow0"] = ("sac", 376, 17, dict(FAMILY, env=dict(FRL_SOLOW="0")))
VARIANTS["knob/solo0"] = NARROW + (dict(FAMILY, env=dict(FRL_SOLO="0")),)
VARIANTS["knob/critic_v2_1"] = NARROW + (dict(FAMILY, env=dict(FRL_CRITIC_V2="1")),)
VARIANTS["knob/critic_v2_0"] = NARROW + (dict(FAMILY, n_learners=200, env=dict(FRL_CRITIC_V2="0")),)
VARIANTS["knob/rc16"] = NARROW + (dict(FAMILY, n_learners=64, env=dict(FRL_RC="16")),)
VARIANTS["knob/solow_narrow"] = NARROW + (dict(FAMILY, env=dict(FRL_SOLOW_NARROW="1")),)
VARIANTS["knob/solow_helpers0"] = WIDE + (dict(FAMILY, env=dict(FRL_SOLOW_HELPERS="0")),)
VARIANTS["knob/chain_waves4"] = NARROW + (dict(FAMILY, n_learners=200, env=dict(FRL_CHAIN_WAVES="4")),)
# the refused ones: code and the words the suite's other tests look for; every other VARIANT (a limit that does not apply to that
# algorithm: reward_dim is ignored without a reward vector, envelope DDPG has no per-row walk over head columns) is accepted
CREATE_REFUSED = {}
for _k in TWO_WG:
    CREATE_REFUSED[_k + "/hidden512"] = (1, "hidden 512 > 256")
    CREATE_REFUSED[_k + "/hidden40"] = (1, "hidden must be a multiple of 16")
    CREATE_REFUSED[_k + "/obs1000"] = (1, "80 KB")
for _k in ("envelope_dqn", "envelope_ddpg"):
    CREATE_REFUSED[_k + "/reward_dim-1"] = (1, "reward_dim -1")
CREATE_REFUSED["sacd/columns"] = (1, "65 actions")
CREATE_REFUSED["reinforce/columns"] = (1, "65 actions")
CREATE_REFUSED["envelope_dqn/columns"] = (1, "head columns")
# (the wording of these three changed with the algorithm table, after their messages were recorded: the words above are what is pinned;
#  every other refusal is pinned word for word by the golden)
REWORDED = ("sacd/columns", "reinforce/columns", "envelope_dqn/columns")
CREATE_REFUSED["gail/tanh"] = (1, "GAIL: hidden_act FRL_ACT_TANH is refused")
CREATE_REFUSED["sac/leaky_relu"] = (1, "SAC engines do not take it")
CREATE_REFUSED["sac/two_agents"] = (1, "n_agents > 1 needs FRL_ALGO_MADDPG")
CREATE_REFUSED["dqn/c51_atoms65"] = (1, "c51_atoms 65")
for _k in ("mappo", "ippo", "happo"):
    CREATE_REFUSED[_k + "/hidden272"] = (1, "hidden 272 > 256")
    CREATE_REFUSED[_k + "/tanh"] = (1, "hidden_act 2 is refused")
    CREATE_REFUSED[_k + "/twin_critic"] = (1, "twin_critic, dueling, noisy, c51_atoms and actor_dist must be 0")
    CREATE_REFUSED[_k + "/extra_cols"] = (1, "extra_cols 6 != 5 log-prob columns + 2 adv_done columns")
CREATE_REFUSED["ippo/state"] = (1, "state_dim 6: a global-state critic belongs to FRL_ALGO_MAPPO engines")
CREATE_REFUSED["mappo/state_extra_cols"] = (1, "extra_cols 7 != 5 log-prob columns + 2 adv_done columns [+ 5 mask columns] + 6 state columns")
CREATE_REFUSED["mappo/state_lds"] = (1, "3000 of them the state's: state_dim")


def _native():
    from freerl_amd import _native as N
    N.lib()
    return N


def engine_args(N, kind, obs_dim=None, act_dim=None, **over):
    """(positional arguments, keywords) of the Engine of one configuration."""
    algo, O, A, kw, _ = ENGINES[kind]
    kw = dict(SMALL, **dict(kw, **over))
    return (getattr(N, algo), O if obs_dim is None else obs_dim, A if act_dim is None else act_dim, kw.pop("capacity")), kw


def _make(N, kind, obs_dim=None, act_dim=None, **over):
    from freerl_amd.engine import Engine
    args, kw = engine_args(N, kind, obs_dim, act_dim, **over)
    return Engine(*args, **kw)


def _configs():
    """name -> (engine kind, obs_dim, act_dim, keywords, environment of the create)"""
    out = {k: (k, None, None, {}, {}) for k in ENGINES}
    for name, (kind, O, A, over) in VARIANTS.items():
        over = dict(over)
        out[name] = (kind, O, A, over, over.pop("env", {}))
    return out


def describe(e, kind):
    """Everything frl_create decided that the ABI shows."""
    lay = e.layout
    d = dict(lds_bytes=e.lds_bytes()[0], row_chunk=e.lds_bytes()[1], n_nets=e.n_nets, n_params=[e.num_params(i) for i in range(e.n_nets)])
    d["layout"] = {name: (list(getattr(lay, name)) if hasattr(getattr(lay, name), "__len__") else int(getattr(lay, name)))
                   for name, _ in lay._fields_}
    d["learn_path"] = list(e.learn_path(8)) if ENGINES[kind][4] == "frl_learn" else None
    d["learn_path_max"] = list(e.learn_path(e.batch_max)) if ENGINES[kind][4] == "frl_learn" else None
    return d


def collect(N):
    """name -> describe() of every configuration frl_create accepts, or {"refused": code, "message": ...}."""
    out = {}
    for name, (kind, O, A, over, env) in _configs().items():
        with pytest.MonkeyPatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            try:
                e = _make(N, kind, O, A, **over)
            except N.FrlError as err:
                out[name] = dict(refused=int(re.match(r"freerl_hip error (\d+)", str(err)).group(1)), message=str(err))
                continue
        out[name] = describe(e, kind)
        e.close()
    return out


def assert_matches_golden(created):
    """`created` (collect()'s result, or the CPU probe's) against the recorded matrix, entry by entry."""
    with open(GOLDEN) as f:
        want = json.load(f)["configs"]
    assert sorted(created) == sorted(want)
    for name, got in created.items():
        print(name, got)
        if name in CREATE_REFUSED:
            code, words = CREATE_REFUSED[name]
            assert got.get("refused") == code and words in got["message"], (name, got)
            assert "refused" in want[name], name
        else:
            assert "refused" not in got, (name, got)
        if name not in REWORDED:
            assert got == want[name], (name, got, want[name])
    assert created["sac/wide_input"]["row_chunk"] == 32 and created["sac/wide_input"]["lds_bytes"] > 80 * 1024      # the 16 -> 32 bump


@pytest.fixture(scope="module")
def N():
    return _native()


@pytest.fixture(scope="module")
def created(N):
    return collect(N)


def test_create_time_decisions_match_the_recorded_ones(N, created):
    assert_matches_golden(created)


def _call(N, e, pool, entry):
    """Call `entry` on engine e with arguments that end a served call in validation, before any launch -> (code, message)."""
    L, h = e._L, e._h
    i, d = C.c_int(0), C.c_double(0)
    if entry == "frl_learn":
        rc = L.frl_learn(h, C.byref(N.LearnArgs()))                              # batch 0
    elif entry == "frl_learn_path":
        rc = L.frl_learn_path(h, 8, C.byref(i), C.byref(i), C.byref(i))
    elif entry == "frl_learn_work":
        rc = L.frl_learn_work(h, 8, 1, C.byref(d), C.byref(d))
    elif entry == "frl_learn_work_executed":
        rc = L.frl_learn_work_executed(h, 8, 1, C.byref(d))
    elif entry == "frl_ppo_learn":
        rc = L.frl_ppo_learn(h, C.byref(N.PpoArgs()))                            # horizon 0
    elif entry == "frl_ppo_rollout":
        rc = L.frl_ppo_rollout(h, pool._h, C.byref(N.PpoRolloutArgs()), C.byref(N.RolloutStats()))      # envs_per_learner 0
    elif entry == "frl_reinforce_learn":
        a = N.ReinforceArgs()
        a.gamma = float("nan")
        rc = L.frl_reinforce_learn(h, C.byref(a))
    elif entry == "frl_envelope_learn":
        rc = L.frl_envelope_learn(h, C.byref(N.EnvelopeArgs()))                  # batch 0
    elif entry == "frl_envelope_ddpg_learn":
        rc = L.frl_envelope_ddpg_learn(h, C.byref(N.EnvelopeDdpgArgs()))         # batch 0
    elif entry == "frl_rollout":
        rc = L.frl_rollout(h, None, C.byref(N.RolloutArgs()), C.byref(N.RolloutStats()))                # NULL pool
    else:
        assert entry == "frl_act_explore"
        x = N.ExploreArgs()
        x.kind = 99                                                              # no such exploration rule
        obs, out = np.zeros((1, 1, 4), np.float32), np.zeros((2, 8), np.float32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        rc = L.frl_act_explore(h, N.ACT_ARGMAX if e.cfg.discrete else N.ACT_TANHHEAD, 1, fp(obs), C.byref(x), None, fp(out[0]), fp(out[1]))
    return rc, (L.frl_last_error().decode() if rc else "")


def test_refusal_matrix(N):
    from freerl_amd.envpool import EnvPool
    pool = EnvPool("CartPole-v1", 1)
    bad = []
    for kind, row in REFUSALS.items():
        e = _make(N, kind)
        own = ENGINES[kind][4]
        rng = np.random.default_rng(5)
        for net in range(e.n_nets):
            e.set_params(net, rng.standard_normal(e.num_params(net)).astype(np.float32))
        before = [e.get_params(net) for net in range(e.n_nets)]
        for entry, want in zip(ENTRIES, row):
            rc, msg = _call(N, e, pool, entry)
            print("%-14s %-24s -> %d %s" % (kind, entry, rc, msg))
            names_both = entry in msg and re.search(r"\b%s\b" % own, msg) is not None
            if isinstance(want, int):
                ok = rc == want and rc != 4
            elif want == "S4":
                ok = rc == 4 and "frl_act_explore" in msg and "single-agent" in msg
            else:                           # refused: the code, the entry point that was called and the one to use instead
                ok = rc == int(want[1]) and names_both
            if not ok:
                bad.append((kind, entry, want, rc, msg))
        for net in range(e.n_nets):         # nothing was launched
            assert np.array_equal(before[net], e.get_params(net)) and e.opt_step(net) == 0, (kind, net)
        e.close()
    pool.close()
    assert not bad, bad
    # frl_act_explore keeps saying how such an engine does act
    for kind, words in (("sacd", "FRL_ACT_CAT_SAMPLE"), ("reinforce", "FRL_ACT_CAT_SAMPLE"), ("envelope_dqn", "FRL_ACT_RAW"),
                        ("envelope_ddpg", "FRL_ACT_TANHHEAD")):
        e = _make(N, kind)
        rc, msg = _call(N, e, None, "frl_act_explore")
        assert rc == 4 and re.search(r"\bfrl_act\b", msg) and words in msg, (kind, msg)
        e.close()


if __name__ == "__main__":
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert len(sys.argv) >= 2 and sys.argv[1] == "--record", "usage: test_gpu_algo_matrix.py --record [PATH]"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        commit = subprocess.run(["git", "-C", root, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(path, "w") as f:
        json.dump(dict(recorded_at=os.environ.get("FRL_RECORD_COMMIT", commit), configs=collect(_native())), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
