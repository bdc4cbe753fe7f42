"""CPU: csrc/learn_plan.hpp — what frl_learn, frl_envelope_learn, frl_envelope_ddpg_learn, frl_gail_learn, frl_cem_gd3pg_learn and
frl_reinforce_learn decide before they touch the device: every refusal with its code, text and precedence, the defaults of a frl_learn's
arguments, the ordered launches of a call per kernel family (the rows of tests/test_gpu_learn_launches.py's CASES, on engines planned by
plan_engine), who draws the rows and with how much LDS, the range check of a caller's idx at its three bounds, the FRL_STAGGER_GROUPS clamp.

tests/learn_plan_probe.cpp is plain C++17 over that header, compiled with g++ under AddressSanitizer + UBSan and run as its own
program (tests/test_onpolicy_plan.py's recipe)."""
import os
import subprocess

import pytest

from tests.test_gpu_learn_launches import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("learn_plan") / "learn_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "learn_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def test_launch_lists_refusals_draws_and_knobs(probe):
    r = subprocess.run([probe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "learn_plan ok: %d launch lists" % len(CASES), r.stdout


def test_the_probe_states_every_row_of_the_gpu_cases():
    """the probe's rows are written out in C++: each id of the GPU test's CASES must stand there, with that row's counts"""
    src = open(os.path.join(ROOT, "tests", "learn_plan_probe.cpp")).read()
    for c in CASES:
        counts = "{%s}" % ", ".join(str(n) for n in c[5])
        line = next((ln for ln in src.splitlines() if 'CASE("%s"' % c[0] in ln), None)
        assert line is not None and ", %d, %s, FAM_" % (c[4], counts) in line, (c[0], line)


# (bound, capacity, size, entries): capacity with negative wrap-around; the rows the learner's ring holds; ring 1 of a ring pair
@pytest.mark.parametrize("args", [("wrap", 40, 7, [0, 39, -1, -40]), ("held", 40, 7, [0, 6]), ("pair", 40, 7, [0, 6])], ids=lambda a: a[0])
def test_a_callers_idx_is_narrowed(probe, args):
    r = subprocess.run([probe, "idx", args[0], str(args[1]), str(args[2])] + [str(v) for v in args[3]], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "idx ok", r.stdout + r.stderr


@pytest.mark.parametrize("bound,bad,text", [
    ("wrap", 40, "refused 1: sample index 40 out of range"), ("wrap", -41, "refused 1: sample index -41 out of range"),
    ("held", 7, "refused 4: idx entry 7 of learner 0 is not one of its 7 stored rows"), ("held", -1, "refused 4: idx entry -1 of learner 0 is not one of its 7 stored rows"),
    ("pair", 7, "refused 1: learner 0: idx entry 7 of ring 1 outside [0, 7) (the rows it holds)"),
    ("pair", -1, "refused 1: learner 0: idx entry -1 of ring 1 outside [0, 7) (the rows it holds)")])
def test_a_violation_is_reported(probe, bound, bad, text):
    """the probe is not vacuous: an entry at the bound (or below its lower end) is named, with the bound's own code and text"""
    r = subprocess.run([probe, "idx", bound, "40", "7", "0", "1", str(bad), "2"], capture_output=True, text=True)
    assert r.returncode == 1 and text in r.stdout, r.stdout + r.stderr


def test_no_knob_is_read_outside_learn_knobs():
    """frl_api_learn.inc and the five entry points' files: nothing reads the environment but learn_knobs(), which names the nine knobs"""
    csrc = os.path.join(ROOT, "freerl_amd", "csrc")
    for name in ("learn", "envelope", "envelope_ddpg", "gail", "cem_gd3pg", "reinforce"):
        src = open(os.path.join(csrc, "frl_api_%s.inc" % name)).read()
        if name == "learn":
            head, rest = src.split("static LearnKnobs learn_knobs() {", 1)
            body, tail = rest.split("\n}\n", 1)
            assert body.count('is("') == 9
            src = head + tail
        for fn in ("env_set(", "env_int(", "env_flag(", "getenv("):
            assert fn not in src, (name, fn)
    assert "getenv" not in open(os.path.join(csrc, "learn_plan.hpp")).read().replace("no getenv", "")
