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


def test_create_time_matrix_matches_the_recorded_one(probe, tmp_path):
    lines = []
    for name, (kind, O, A, over, env) in matrix._configs().items():
        args, kw = matrix.engine_args(N, kind, O, A, **over)
        cfg, ext = make_config(*args, **kw)
        knobs = ["%s=%d" % (KNOBS[k], int(v)) for k, v in env.items()]
        lines.append(" ".join([name, bytes(cfg).hex(), bytes(ext).hex() if ext is not None else "-", "256", str(160 * 1024)] + knobs))
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

