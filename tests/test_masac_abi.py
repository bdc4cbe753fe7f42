"""CPU: the C ABI and the host plan of MASAC — include/freerl_hip.h declares FRL_ALGO_MASAC = 15 and the per-agent alpha accessors,
csrc/frl_desc.h mirrors the value, freerl_amd/_native.py binds them, the library reports frl_version() >= 111 and exports the symbols,
kernels_masac.hip is a unit of the build and registered as a family; the create-time plan of such an engine (csrc/engine_plan.hpp
through tests/masac_plan_probe.cpp): every net's layer shapes, 2 n + 1 draw sets, the alpha and step-counter storage, the family, and
every refusal with its message; the class refuses discrete actions at construction."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_MAX_NETS = 16


def test_header_enum_binding_and_version():
    from freerl_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "freerl_hip.h")).read()
    assert re.search(r"\bFRL_ALGO_MASAC\s*=\s*15\b", hdr) and re.search(r"\bFRL_ALGO_MADDPG_ATT\s*=\s*14\b", hdr)
    for sym in ("frl_alpha_get_agent(frl_engine* e, int learner, int agent, float* vals4_out, int* step_out)",
                "frl_alpha_set_agent(frl_engine* e, int learner, int agent, const float* vals4, int step)",
                "int frl_alpha_get(frl_engine* e, int learner, float* vals4_out, int* step_out);"):
        assert sym in hdr, sym
    desc = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_desc.h")).read()
    assert re.search(r"\bALGO_MASAC\s*=\s*15\b", desc)
    assert N.ALGO_MASAC == 15 and N.ALGO_MADDPG_ATT == 14
    assert N.SIGNATURES["frl_alpha_get_agent"][1][1:3] == [C.c_int, C.c_int] and "frl_alpha_set_agent" in N.SIGNATURES
    # the structs did not grow
    assert [f[0] for f in N.Config._fields_][-1] == "reward_dim" and [f[0] for f in N.LearnArgs._fields_][-1] == "huber_delta"
    N.build()
    L = C.CDLL(N.LIB_PATH)
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 111
    for sym in ("frl_alpha_get_agent", "frl_alpha_set_agent"):
        assert hasattr(L, sym)


def test_kernel_unit_is_built_and_registered():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_masac.hip" for u in N.units())
    src = open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_masac.hip")).read()
    for k in ("masac_critic_kernel", "masac_actor_kernel", "masac_act_kernel"):
        assert k in src
    assert "asm" not in src
    api = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api.hip")).read()
    assert '#include "kernels_masac.hip"' in api
    learn = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api_learn.inc")).read()
    assert "{FAM_MASAC, LK_CRITIC, 0, kLdsMasac" in learn and "{FAM_MASAC, LK_ACTOR, 0, kLdsMasac" in learn and "launch_masac" in learn
    regs = open(os.path.join(ROOT, "tools", "kernel_regs.py")).read()
    assert '("masac_critic_", ' in regs and '("masac_actor_", ' in regs and '("masac_act_", ' in regs


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("masac_plan") / "masac_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "masac_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def _plan(probe, name, obs, act, hidden=128, batch_max=256, P=1, discrete=0, twin=1, hidden_act=1, algo=None):
    args = [probe, name, str(len(obs))] + [str(x) for x in obs] + [str(x) for x in act] + [str(v) for v in (hidden, batch_max, P, discrete, twin, hidden_act)]
    if algo is not None:
        args.append(str(algo))
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


@pytest.mark.parametrize("name,obs,act,kw", [("spread3", [18] * 3, [5] * 3, dict(P=64)), ("hetero", [8, 10, 10], [1, 2, 1], dict(hidden=64, batch_max=17)),
                                             ("pair", [7, 7], [4, 4], dict(hidden=64, batch_max=5)), ("eight", [3] * 8, [2] * 8, dict(hidden=32, batch_max=32, P=3)),
                                             ("single", [11], [3], {})])
def test_plan_of_a_masac_engine(probe, name, obs, act, kw):
    d = _plan(probe, name, obs, act, **kw)
    assert "refused" not in d, d
    n, H, P = len(obs), kw.get("hidden", 128), kw.get("P", 1)
    T = sum(obs) + sum(act)
    assert d["n_nets"] == 2 * n
    for i in range(n):
        a, c = d["nets"][2 * i], d["nets"][2 * i + 1]
        # the actor: l1, l2 and ONE head of 2 A outputs [mean_layer | log_std_layer], no extra log_std vector, no output activation
        assert a["layers"] == [[H, obs[i]], [H, H], [2 * act[i], H]] and a["heads"] == 1 and a["extra_n"] == 0 and a["out_act"] == 0 and a["hidden_act"] == 1
        # the critic: Q1 then Q2 on [all obs | all actions], six layers in one net
        assert c["layers"] == [[H, T], [H, H], [1, H]] * 2 and c["heads"] == 2
    assert d["noise_sets"] == 2 * n + 1 and d["act_max"] == max(act)
    assert d["noise_count"] == P * n * (2 * n + 1) * kw.get("batch_max", 256) * max(act)
    assert d["alpha_count"] == P * n * 4 and d["steps_count"] == P * (K_MAX_NETS + 1) + P * n
    assert d["family"] == d["fam_masac"] == d["learn_family"] and d["chained"] == 0
    assert d["row_chunk"] in (16, 32, 64) and 0 < d["lds_bytes"] <= 160 * 1024
    assert d["lds_row_extra"] == (2 * max(act) + 3) // 4 * 4


def test_other_algorithms_keep_their_storage(probe):
    from freerl_amd import _native as N
    for algo, obs, act in ((N.ALGO_SAC, [11], [3]), (N.ALGO_MADDPG, [18] * 3, [5] * 3), (N.ALGO_TD3, [11], [3])):
        d = _plan(probe, "other", obs, act, algo=algo, P=2)
        assert d["noise_sets"] == max(2, len(obs)) and d["alpha_count"] == 2 * 4 and d["steps_count"] == 2 * (K_MAX_NETS + 1)
        assert d["family"] != d["fam_masac"] and d["learn_family"] != d["fam_masac"] and d["lds_row_extra"] == 0


def test_refusals(probe):
    bad = dict(discrete=dict(discrete=1), single_critic=dict(twin=0), tanh=dict(hidden_act=2), leaky=dict(hidden_act=3),
               hidden_40=dict(hidden=40), too_wide=dict(hidden=4096))
    want = dict(discrete="discrete is refused (continuous actions only: the reference's discrete branch calls Agent.argmax",
                single_critic="twin_critic = 0 is refused", tanh="hidden_act 2 is refused", leaky="hidden_act 3 is refused",
                hidden_40="hidden must be a multiple of 16", too_wide="of LDS per")
    for name, kw in bad.items():
        d = _plan(probe, name, [8, 10], [2, 3], **kw)
        assert d.get("refused") == 1 and want[name] in d["message"], d
        if name != "hidden_40":
            assert d["message"].startswith("MASAC: "), d
    wide = _plan(probe, "wide_input", [9000, 9000, 9000, 9000], [2] * 4, hidden=128)
    assert wide.get("refused") == 1 and wide["message"].startswith("MASAC: hidden 128 is refused") and "160 KB" in wide["message"]
    nine = _plan(probe, "nine", [3] * 9, [2] * 9)
    assert nine.get("refused") == 1 and "n_agents out of range" in nine["message"]


def test_class_refuses_discrete_actions_at_construction():
    from freerl_amd.MASAC import MASAC, actor_layers, critic_layers
    with pytest.raises(ValueError, match="continuous"):
        MASAC({"a": [4, 3], "b": [4, 3]}, False, 1e-4, 1e-4, 100, "cpu")
    assert [n for n, _, _ in actor_layers(4, 3, 128)] == ["l1", "l2", "mean_layer", "log_std_layer"]
    assert [n for n, _, _ in critic_layers(14, 128)] == ["l1", "l2", "l3", "l1_2", "l2_2", "l3_2"]
    assert actor_layers(4, 3, 128)[2:] == [("mean_layer", 3, 128), ("log_std_layer", 3, 128)]
