"""csrc/actor_park_layout.h — where the eight-wave chained actor stage parks pass A's activations — and what csrc/engine_plan.hpp
allocates for it, on the CPU.  Both headers are plain C++17 without HIP: tests/actor_park_probe.cpp compiles with g++ alone and runs
under AddressSanitizer + UBSan as a stand-alone program (tests/test_engine_plan.py's recipe).  The kernel and the plan include the same
header, so the largest offset a lane touches and the allocated size are one formula; this file pins that formula."""
import os
import subprocess

import pytest

from freerl_amd import _native as N
from freerl_amd.engine import make_config
from tests import test_gpu_algo_matrix as matrix
from tests.test_engine_plan import _line

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAM_CHAINED = 2                      # engine_plan.hpp: LearnFamily
LEARNER_FLOATS = 256 * 128           # kChainBatch rows x the 128 features of h2 = 128 KiB


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("actor_park") / "actor_park_probe"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "actor_park_probe.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("P", [1, 3, 512])
def test_slots_fill_the_planned_size_exactly_and_never_overlap(probe, P):
    r = subprocess.run([probe, "walk", str(P)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    d = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    n = P * 2 * 8 * 8 * 64          # (learner, chunk, tile, wave, lane)
    assert d["slots"] == n
    # the largest slot offset over all (chunk, tile, wave, lane), plus its 16 bytes, is the planned allocation
    assert d["max_end_bytes"] == d["planned_bytes"] == P * LEARNER_FLOATS * 4
    assert d["overlaps"] == 0 and d["outside"] == 0
    assert d["ragged"] == 0          # a wave instruction covers 1 KB contiguously; a lane's tiles lie 8 KB apart


def _plan(probe, tmp_path, lines):
    path = tmp_path / "configs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([probe, "plan", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {}
    for l in r.stdout.splitlines():
        name, rest = l.split(": ", 1)
        f = rest.split()
        out[name] = None if rest == "refused" else {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    assert len(out) == len(lines)
    return out


def test_the_plan_allocates_it_for_chained_engines_only(probe, tmp_path):
    lines, want = [], {}

    def add(name, algo, P, env, chained, O=8, A=2, **kw):
        cfg, ext = make_config(algo, O, A, 512, n_learners=P, batch_max=256, **kw)
        lines.append(_line(name, cfg, ext, env))
        want[name] = P * LEARNER_FLOATS if chained else 0

    for algo, kw in ((N.ALGO_TD3, dict(twin_critic=True)), (N.ALGO_DDPG, {}), (N.ALGO_SAC, dict(twin_critic=True))):
        for P in (1, 3, 512):
            add("chained/%d/%d" % (algo, P), algo, P, dict(FRL_CRITIC_V2="1"), True, **kw)
            add("chained_w4/%d/%d" % (algo, P), algo, P, dict(FRL_CRITIC_V2="1", FRL_CHAIN_WAVES="4"), True, **kw)
        add("default/%d/512" % algo, algo, 512, {}, True, **kw)            # a population past 128 learners: chained without a knob
        add("solo/%d/3" % algo, algo, 3, {}, False, **kw)                  # a few learners: kernels_solo.hip
        add("rowchunk/%d/100" % algo, algo, 100, {}, False, **kw)          # 17 .. 128 learners: the row-chunk kernels
        add("rowchunk_named/%d/512" % algo, algo, 512, dict(FRL_CRITIC_V2="0"), False, **kw)
        add("wide/%d/512" % algo, algo, 512, {}, False, O=376, A=17, **kw)     # the K-sliced family has its own scratch
    add("dqn", N.ALGO_DQN, 512, {}, False, discrete=True)
    add("sacd", N.ALGO_SAC_DISCRETE, 512, {}, False, twin_critic=True)
    add("ppo", N.ALGO_PPO, 512, {}, False)
    add("maddpg", N.ALGO_MADDPG, 512, {}, False, O=[8, 8], A=[2, 2])
    add("replay_only", N.ALGO_REPLAY_ONLY, 512, {}, False)
    out = _plan(probe, tmp_path, lines)
    for name, floats in want.items():
        assert out[name] is not None, name
        assert out[name]["floats"] == floats, (name, out[name])
        assert (out[name]["family"] == FAM_CHAINED) == (floats > 0), (name, out[name])
        assert out[name]["null"] == 1          # a plan carries no device pointer
        assert out[name]["park"] == 1          # the default


def test_the_knob_selects_the_kernel_not_the_allocation(probe, tmp_path):
    cfg, ext = make_config(N.ALGO_TD3, 8, 2, 512, n_learners=512, twin_critic=True, batch_max=256)
    base = " ".join([bytes(cfg).hex(), "-", "256", str(160 * 1024)])
    out = _plan(probe, tmp_path, ["on " + base + " actor_park=1", "off " + base + " actor_park=0"])
    assert out["on"]["park"] == 1 and out["off"]["park"] == 0
    assert out["on"]["floats"] == out["off"]["floats"] == 512 * LEARNER_FLOATS == 64 * 1024 * 1024 // 4


def test_every_configuration_of_the_algorithm_matrix(probe, tmp_path):
    """tests/test_gpu_algo_matrix.py's create-time matrix: the array exists exactly where the plan picked the chained family"""
    lines = []
    for name, (kind, O, A, over, env) in matrix._configs().items():
        args, kw = matrix.engine_args(N, kind, O, A, **over)
        cfg, ext = make_config(*args, **kw)
        lines.append(_line(name, cfg, ext, env))
    out = _plan(probe, tmp_path, lines)
    chained = 0
    for name, d in out.items():
        if d is None:
            continue
        assert (d["floats"] > 0) == (d["family"] == FAM_CHAINED), (name, d)
        chained += d["family"] == FAM_CHAINED
    assert chained >= 1
