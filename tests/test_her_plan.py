"""csrc/her_plan.h - which relabelled rows follow which transition of a finished episode, where they go in the ring, and the rule set
that refuses a frl_her_relabel call - on the CPU.  The header is plain C++17 without HIP, so tests/her_plan_probe.cpp compiles with g++
alone and runs under AddressSanitizer + UBSan as a stand-alone program (tests/test_engine_plan.py's recipe)."""
import os
import subprocess

import pytest

from tests import her_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("her_plan") / "her_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "her_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def test_every_small_episode_is_walked_or_refused_for_its_rule(probe):
    r = subprocess.run([probe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    word, ok, accepted, refused = r.stdout.split()
    assert (word, ok) == ("her_plan", "ok") and int(accepted) > 1000 and int(refused) > 1000


def test_totals_equal_the_python_formula(probe):
    r = subprocess.run([probe, "--totals"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(lines) == 14 * 4 * 4
    for L, k, R, total in lines:
        assert total == oracle.total(L, k, R) == sum(min(k, R, L - i) for i in range(L)), (L, k, R, total)
    assert (40, 4, 200, 154) in lines and (40, 4, 2, 79) in lines and (200, 4, 200, 794) in lines


def test_the_kernel_and_the_host_call_use_the_header():
    csrc = os.path.join(ROOT, "freerl_amd", "csrc")
    kernel, api = open(os.path.join(csrc, "kernels_her.hip")).read(), open(os.path.join(csrc, "frl_api_her.inc")).read()
    for name in ("her_plan(", "her_locate(", "her_src(", "her_dst(", "her_total("):
        assert name in kernel, name
    for name in ("her_check_shape(", "her_check_episode(", "her_total(", "her_refusal_text("):
        assert name in api, name
    assert "% a.capacity" not in kernel and "% h.capacity" not in api      # no ring arithmetic of their own
