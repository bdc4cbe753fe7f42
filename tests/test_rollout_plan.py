"""csrc/rollout_plan.hpp — everything a frl_rollout call decides before it touches the device: refusals, the exploration rule, whether
the vector step is folded into the learn launches, read in place, handed over by flag and pre-armed; the learn-step predicate and the
layout of the per-step block — on the CPU.  The header is plain C++17 without HIP, so tests/rollout_plan_probe.cpp compiles with g++
alone and runs under AddressSanitizer + UBSan as a stand-alone program (tests/test_engine_plan.py's recipe).  The probe's expected
values are literals from the documented rules (include/freerl_hip.h), not from the code under test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rollout_plan") / "rollout_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rollout_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def test_literals_under_sanitizers(probe):
    r = subprocess.run([probe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "rollout_plan ok"


def test_the_rollout_loop_reads_no_environment_variable_itself():
    """The knobs reach the plan through rollout_knobs() and the env_* helpers of frl_api.hip: one place to read, one struct to test."""
    src = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api_rollout.inc")).read()
    assert "getenv" not in src
