"""CPU: the C ABI of ATT-MADDPG - include/freerl_hip.h declares FRL_ALGO_MADDPG_ATT = 14, csrc/frl_desc.h mirrors it, frl_config and
frl_config_ext keep their fields, freerl_amd/_native.py binds the value, the library reports frl_version() >= 110, kernels_att.hip is a
unit of the build and listed in tools/kernel_regs.py; and the create-time plan of such an engine (csrc/engine_plan.hpp through
tests/engine_plan_probe.cpp as it stands): nets, parameter counts, LDS bytes, row chunk, and every refusal with its message."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_enum_binding_and_version():
    from freerl_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "freerl_hip.h")).read()
    assert re.search(r"\bFRL_ALGO_MADDPG_ATT\s*=\s*14\b", hdr) and re.search(r"\bFRL_ALGO_HAPPO\s*=\s*13\b", hdr)
    desc = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_desc.h")).read()
    assert re.search(r"\bALGO_MADDPG_ATT\s*=\s*14\b", desc) and re.search(r"kAttHeads\s*=\s*4\b", desc)
    assert N.ALGO_MADDPG_ATT == 14 and N.ALGO_MADDPG == 4
    # the structs did not grow: the algorithm value alone selects the critic
    assert [f[0] for f in N.Config._fields_][-1] == "reward_dim" and [f[0] for f in N.ConfigExt._fields_] == ["size", "state_dim", "state_rows"]
    N.build()
    L = C.CDLL(N.LIB_PATH)
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 110


def test_kernel_unit_is_built_and_listed():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_att.hip" for u in N.units())
    regs = open(os.path.join(ROOT, "tools", "kernel_regs.py")).read()
    assert '("att_critic_", ' in regs and '("att_actor_", ' in regs and '("att_q_", ' in regs
    src = open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_att.hip")).read()
    for k in ("att_critic_kernel", "att_actor_kernel", "att_q_kernel"):
        assert k in src
    api = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api.hip")).read()
    assert '#include "kernels_att.hip"' in api
    learn = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api_learn.inc")).read()
    assert "{FAM_ATT, LK_CRITIC, 0, kLdsAtt" in learn and "{FAM_ATT, LK_ACTOR, 0, kLdsAtt" in learn and "launch_att" in learn
    assert "case FAM_ATT: launch_rowchunk(e, s, a, fam)" in learn          # FAM_ATT is dispatched to the row-chunk launcher


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("att_plan") / "engine_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "engine_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def _plan(probe, tmp_path, configs):
    """{name: (obs, act, kwargs)} -> {name: the probe's description}"""
    from freerl_amd import _native as N
    from freerl_amd.engine import make_config
    lines = []
    for name, (obs, act, kw) in configs.items():
        cfg, ext = make_config(kw.pop("algo", N.ALGO_MADDPG_ATT), obs, act, 512, **kw)
        lines.append(" ".join([name, bytes(cfg).hex(), "-", "256", str(160 * 1024)]))
    path = tmp_path / "configs.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([probe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {d["name"]: d for d in map(json.loads, r.stdout.splitlines())}


def _critic_params(obs, act, i, H):
    xe, xd = sum(obs) + act[i], sum(act) - act[i]
    return (H * H + H) * 3 + 4 * (H * H + H) + (H * xe + H) + (H * xd + H) + (H + 1)


def test_plan_of_an_att_engine(probe, tmp_path):
    shapes = dict(spread5=([30] * 5, [5] * 5, dict(batch_max=256)), spread3=([18] * 3, [5] * 3, dict(batch_max=64, n_learners=64)),
                  hetero=([8, 10, 10], [1, 2, 1], dict(batch_max=17, hidden=64)), pair=([7, 7], [4, 4], dict(batch_max=5)),
                  eight=([3] * 8, [2] * 8, dict(batch_max=32, hidden=32)))
    got = _plan(probe, tmp_path, {k: (o, a, dict(kw)) for k, (o, a, kw) in shapes.items()})
    for name, (obs, act, kw) in shapes.items():
        d, H, n = got[name], kw.get("hidden", 128), len(obs)
        assert "refused" not in d, d
        assert d["n_nets"] == 2 * n and d["row_chunk"] == 16
        assert 0 < d["lds_bytes"] <= 160 * 1024
        for i in range(n):
            assert d["n_params"][2 * i] == (H * obs[i] + H) + (H * H + H) + (act[i] * H + act[i])
            assert d["n_params"][2 * i + 1] == _critic_params(obs, act, i, H)
        # FAM_ATT: row chunks of 16 rows with the engine's own carve, at every batch and population (never a chained / solo / wide family)
        assert d["learn_path"] == [False, d["lds_bytes"], 16] and d["learn_path_max"] == [False, d["lds_bytes"], 16]
        assert d["layout"]["n_agents"] == n and d["layout"]["rew_off"] == sum(obs) + sum(act)
    # the carve: the common region with x_e as the first-layer input, then x_d, d, u, c, y and the four heads per row
    H, xe, xd, ap = 128, 160, 32, 28
    assert got["spread5"]["lds_bytes"] == 4 * (16 * ((xe + 4) + 2 * (H + 4) + 20 + 2 * ap + (xd + 4) + 4 * (H + 4) + (4 * H + 4)) + 128 + 8)
    # the plain engine of the same shape keeps its plan
    from freerl_amd import _native as N
    plain = _plan(probe, tmp_path, dict(plain=([30] * 5, [5] * 5, dict(algo=N.ALGO_MADDPG, batch_max=256))))["plain"]
    assert plain["n_params"][1] == (128 * 175 + 128) + (128 * 128 + 128) + 129 and plain["row_chunk"] != 16


def test_refusals(probe, tmp_path):
    bad = dict(one_agent=([4], [2], {}), twin=([4, 5], [2, 3], dict(twin_critic=True)), discrete=([4, 5], [2, 3], dict(discrete=True)),
               hidden_40=([4, 5], [2, 3], dict(hidden=40)), hidden_256=([4, 5], [2, 3], dict(hidden=256)),
               wide_encoder=([9000, 4], [2, 3], {}), wide_decoder=([4] * 8, [2000] * 8, {}), leaky=([4, 5], [2, 3], dict(hidden_act=3)))
    want = dict(one_agent="n_agents 1 < 2", twin="twin_critic is refused", discrete="discrete is refused", hidden_40="hidden must be a multiple of 16",
                hidden_256="hidden 256 is refused", wide_encoder="of LDS per 16-row chunk > 160 KB", wide_decoder="of LDS per 16-row chunk > 160 KB",
                leaky="hidden_act 3 is refused")
    got = _plan(probe, tmp_path, {k: (o, a, dict(kw)) for k, (o, a, kw) in bad.items()})
    for name, msg in want.items():
        assert got[name].get("refused") == 1 and msg in got[name]["message"], got[name]
        if name != "hidden_40":
            assert got[name]["message"].startswith("ATT-MADDPG: ")
    # more than one agent still needs a multi-agent algorithm, and nine agents are out of range for every one
    from freerl_amd import _native as N
    other = _plan(probe, tmp_path, dict(td3=([4, 5], [2, 3], dict(algo=N.ALGO_TD3))))["td3"]
    assert other["refused"] == 1 and "n_agents > 1 needs FRL_ALGO_MADDPG" in other["message"]
