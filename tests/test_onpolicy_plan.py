"""CPU: csrc/onpolicy_plan.hpp — what frl_ppo_learn, frl_gail_ppo_learn, frl_mappo_learn and frl_happo_learn decide before they touch the
device: the refusals and their texts, where the permutations come from, every offset into the d_ppo / d_perm scratch and the totals the
scratch is grown to, the range check of a caller's permutations and the seeded host shuffle.

tests/onpolicy_plan_probe.cpp is plain C++17 over that header, compiled with g++ under AddressSanitizer + UBSan and run as its own
program (tests/test_cem_gd3pg_plan.py's recipe).  Its grid: P in {1, 3} x n_agents in {1, 3} x T in {2, 40, 8192, 8193} x mb in
{1, 16, T} x K in {1, 3}, every family, MAPPO with and without HAPPO's part."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("onpolicy_plan") / "onpolicy_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "onpolicy_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def test_every_shape_refusal_and_shuffle(probe):
    r = subprocess.run([probe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "onpolicy_plan ok: %d shapes" % (2 * 2 * 4 * 3 * 2), r.stdout


def test_a_callers_permutation_is_narrowed(probe):
    r = subprocess.run([probe, "perms", "4", "3", "0", "2", "1", "3"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "perms ok", r.stdout + r.stderr


@pytest.mark.parametrize("bad", ["4", "-1"])
def test_a_violation_is_reported(probe, bad):
    """the probe is not vacuous: an entry equal to T (or below 0) is named"""
    r = subprocess.run([probe, "perms", "4", "0", "1", bad, "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "permutation entry %s outside [0,4)" % bad in r.stdout, r.stdout + r.stderr
