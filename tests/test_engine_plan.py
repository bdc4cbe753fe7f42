"""csrc/engine_plan.hpp — everything frl_create decides before it allocates: refusals, nets, record, kernel family, LDS bytes, row
chunk — on the CPU.  The header is plain C++17 without HIP, so tests/engine_plan_probe.cpp compiles with g++ alone and runs under
AddressSanitizer + UBSan as a stand-alone program (tests/test_host_mem.py's recipe).

The create-time matrix of tests/test_gpu_algo_matrix.py — recorded on a GPU into tests/golden/algo_matrix.json — is checked here on
every machine: each configuration is built as Engine does (freerl_amd.engine.make_config), handed to the probe as the raw struct
bytes with the knob values of its environment, and compared by the GPU test's own comparison."""
import json
import os
import subprocess

import pytest

from freerl_amd import _native as N
from freerl_amd.engine import make_config
from tests import test_gpu_algo_matrix as matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the environment variables frl_create reads -> PlanKnobs fields (csrc/frl_api.hip: create_knobs)
KNOBS = dict(FRL_ASSUME_CUS="assume_cus", FRL_RC="rc", FRL_CPS="cps", FRL_SOLOW_NARROW="solow_narrow", FRL_CRITIC_V2="critic_v2",
             FRL_SOLO="solo", FRL_SOLO_MAXP="solo_maxp", FRL_SOLOW="solow", FRL_SOLOW_HELPERS="solow_helpers", FRL_CHAIN_WAVES="chain_waves")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("engine_plan") / "engine_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "engine_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def test_literals_under_sanitizers(probe):
    r = subprocess.run([probe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "engine_plan ok"


def _line(name, cfg, ext, env):
    knobs = ["%s=%d" % (KNOBS[k], int(v)) for k, v in env.items()]
    return " ".join([name, bytes(cfg).hex(), bytes(ext).hex() if ext is not None else "-", "256", str(160 * 1024)] + knobs)


def _matrix_lines():
    lines = []
    for name, (kind, O, A, over, env) in matrix._configs().items():
        args, kw = matrix.engine_args(N, kind, O, A, **over)
        cfg, ext = make_config(*args, **kw)
        lines.append(_line(name, cfg, ext, env))
    return lines


def test_create_time_matrix_matches_the_recorded_one(probe, tmp_path):
    lines = _matrix_lines()
    path = tmp_path / "configs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([probe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    created = {}
    for line in r.stdout.splitlines():
        d = json.loads(line)
        if "refused" in d:          # (as the binding reports a refused create: _native.check)
            d["message"] = "freerl_hip error %d: %s" % (d["refused"], d["message"])
        created[d.pop("name")] = d
    matrix.assert_matches_golden(created)



# every algorithm whose gradient kernels run on the row-chunk launch shape: (algo, obs_dim, act_dim, Engine keywords)
ROWCHUNK = {
    "dqn": (N.ALGO_DQN, 4, 3, dict(discrete=True)),
    "c51": (N.ALGO_DQN, 4, 3, dict(discrete=True, c51=(51, -10.0, 10.0))),
    "ddpg": (N.ALGO_DDPG, 4, 3, {}),
    "td3": (N.ALGO_TD3, 4, 3, dict(twin_critic=True)),
    "sac": (N.ALGO_SAC, 4, 3, dict(twin_critic=True)),
    "maddpg": (N.ALGO_MADDPG, [4, 5, 3], [3, 2, 2], {}),
    "sacd": (N.ALGO_SAC_DISCRETE, 4, 3, dict(twin_critic=True)),
    "reinforce": (N.ALGO_REINFORCE, 4, 3, {}),
    "envelope_dqn": (N.ALGO_ENVELOPE_DQN, 4, 3, dict(discrete=True, reward_dim=2)),
    "envelope_ddpg": (N.ALGO_ENVELOPE_DDPG, 4, 3, dict(reward_dim=2)),
    "gail": (N.ALGO_GAIL, 4, 3, {}),
    "att": (N.ALGO_MADDPG_ATT, [4, 5, 3], [3, 2, 2], {}),
    "masac": (N.ALGO_MASAC, [4, 5, 3], [3, 2, 2], dict(twin_critic=True)),
}


def _gpu_cps2_cases():
    """The engines of the five test_two_chunks_per_workgroup GPU cases that have no other way to show their cps (the C ABI has no getter
    for it), built from the same case tables as those tests build theirs: name -> make_config arguments.  Created under FRL_RC=16
    FRL_CPS=2, each must plan rc 16, cps 2 and two slabs."""
    from tests import gail_oracle as go, reinforce_oracle as ro, sacd_oracle as so
    from tests.test_gpu_envelope import RAGGED as ENV
    from tests.test_gpu_envelope_ddpg import RAGGED as ENVD
    sd, rf, ga = so.case("o8_a4_bn"), ro.case("o4_a2"), go.COMMON
    return {
        # tests/test_gpu_sac_discrete.py: _engine(N, c, batch_max=64) on a 256-row table
        "gpu/sacd": ((N.ALGO_SAC_DISCRETE, sd["obs_dim"], sd["n_act"], 256), dict(twin_critic=True, hidden=sd["hidden"], batch_max=64)),
        # tests/test_gpu_reinforce.py: _ragged(..., cap=64) (batch_max = capacity)
        "gpu/reinforce": ((N.ALGO_REINFORCE, rf["obs_dim"], rf["n_act"], 64), dict(discrete=True, hidden=rf["hidden"])),
        # tests/test_gpu_envelope.py / test_gpu_envelope_ddpg.py: _engine(N, c, batch_max=64) on RAGGED
        "gpu/envelope_dqn": ((N.ALGO_ENVELOPE_DQN, ENV["obs_dim"], ENV["n_act"], ENV["n_table"]),
                             dict(discrete=True, hidden=ENV["hidden"], batch_max=64, reward_dim=ENV["rdim"])),
        "gpu/envelope_ddpg": ((N.ALGO_ENVELOPE_DDPG, ENVD["obs_dim"], ENVD["act_dim"], ENVD["n_table"]),
                              dict(hidden=ENVD["hidden"], batch_max=64, reward_dim=ENVD["rdim"])),
        # tests/test_gpu_gail.py: _run_against_oracle(..., in_dim=4, batch_max=32) on a 60-row table (a call: up to 2 x batch_max rows)
        "gpu/gail": ((N.ALGO_GAIL, 3, 1, 60), dict(hidden=ga["hidden"], hidden_act=N.ACT_LEAKY_RELU, batch_max=32)),
    }


def test_rowchunk_addresses_stay_inside_the_plans_buffers(probe, tmp_path):
    """csrc/rowchunk_layout.h, the addressing the fifteen row-chunk kernels and the plan's buffer counts share: the probe visits every
    (unit, slice, chunk) at the call sizes {1, rc - 1, rc, rc + 1, the most a call may bring} and asserts that the slices' chunk ranges
    partition the chunks, that every chunk's rows lie inside the call, that slab / part / idx / noise / act_spill offsets plus their
    extents stay inside what the plan allocates, and that no two (unit, slice) pairs share a slab, a part slot or a spill block.

    Forced lines: every row-chunk algorithm under FRL_RC=16 with FRL_CPS in {1, 2, 4} and batch_max in {16, 21, 64, 100} (REINFORCE: the
    capacity, which is its batch_max).  The plan takes FRL_CPS only where it divides the chunks of the largest call (batch_max rows, GAIL
    2 x batch_max): 1, 2, 4 and 7 chunks here (GAIL 2, 3, 8, 13), so cps 2 runs at batch_max 21 and 64 (GAIL 16 and 64), cps 4 at 64 (GAIL
    16 and 64), and the other lines walk the plan's own choice; where the knob divides, the line must say so."""
    lines = _matrix_lines()
    forced = {}      # name -> the cps the plan must have taken, or None where the knob does not divide the chunks
    for name, (algo, O, A, kw) in ROWCHUNK.items():
        for cps in (1, 2, 4):
            for bm in (16, 21, 64, 100):
                cfg, ext = make_config(algo, O, A, bm if algo == N.ALGO_REINFORCE else 128, n_learners=3, hidden=32, batch_max=bm, **kw)
                n_chunks = ((2 * bm if algo == N.ALGO_GAIL else bm) + 15) // 16
                forced["%s/cps%d_bm%d" % (name, cps, bm)] = cps if n_chunks % cps == 0 else None
                lines.append(_line("%s/cps%d_bm%d" % (name, cps, bm), cfg, ext, dict(FRL_RC="16", FRL_CPS=str(cps))))
    gpu = _gpu_cps2_cases()
    for name, (args, kw) in gpu.items():
        cfg, ext = make_config(*args, **kw)
        lines.append(_line(name, cfg, ext, dict(FRL_RC="16", FRL_CPS="2")))
    path = tmp_path / "configs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([probe, "--walk", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = dict(l.split(": ", 1) for l in r.stdout.splitlines())
    assert len(out) == len(lines)
    for name, cps in forced.items():          # none of the forced lines may be refused, rc = 16 and (where it divides) the cps must have been taken
        assert out[name].startswith("rc 16 " if cps is None else "rc 16 cps %d " % cps), (name, out[name])
    assert sum(c is not None for c in forced.values()) >= len(ROWCHUNK) * 7
    for name in gpu:                          # what the GPU cases rely on: two chunks per workgroup, two slabs
        assert out[name].startswith("rc 16 cps 2 S 2:"), (name, out[name])
