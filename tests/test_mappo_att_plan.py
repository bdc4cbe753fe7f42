"""CPU: the create-time plan of FRL_ALGO_MAPPO_ATT (csrc/engine_plan.hpp through tests/mappo_att_plan_probe.cpp): the three refusals, and
the 8-agent, obs-180 engine whose plain-MAPPO critic input would be 1440 columns."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("matt") / "mappo_att_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mappo_att_plan_probe.cpp"), "-o", str(exe)])
    return lambda *a: json.loads(subprocess.check_output([str(exe)] + [str(x) for x in a]))


@pytest.mark.parametrize("args,text", [((1, 18, 18, 5, 128), "n_agents 1 < 2"), ((3, 18, 17, 5, 128), "obs_dim[2] = 17 != obs_dim[0] = 18"),
                                       ((3, 18, 18, 5, 64), "hidden 64 is refused"), ((3, 18, 18, 5, 256), "hidden 256 is refused")])
def test_refusals(probe, args, text):
    r = probe(*args)
    assert r["refused"] == 1 and text in r["message"], r


@pytest.mark.parametrize("n,obs", [(3, 18), (8, 180)])
def test_accepted_with_a_width_that_does_not_grow_with_n(probe, n, obs):
    r = probe(n, obs, obs, 5, 128)
    assert r["refused"] == 0 and r["rc"] == 16 and r["lds_bytes"] <= 160 * 1024 and r["n_nets"] == 2 * n and r["learn"] == "frl_mappo_att_learn"
    assert r["layers"] == [[128, obs], [128, 256], [1, 128], [128, 128], [256, 128], [128, 128]]
