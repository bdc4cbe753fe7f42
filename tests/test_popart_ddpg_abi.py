"""CPU: the C ABI of PopArt DDPG (FRL_ALGO_DDPG_POPART = 20; 17 and 19 stay unassigned) in the header, frl_desc.h, _native.py and the built
library; the create-time refusals (tests/gail_ppo_plan_probe.cpp's describer), the call-time ones and the learner block's layout
(tests/popart_plan_probe.cpp) by their wording."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "freerl_amd", "csrc")
FIELDS = ["batch", "gamma", "tau", "actor_lr", "critic_lr", "upper_lr", "beta", "idx", "out"]


def test_header_desc_and_binding_agree():
    from freerl_amd import _native as N
    from freerl_amd.engine import Engine
    from tools.gen_ctypes_stub import parse_later_structs
    hdr = open(os.path.join(ROOT, "include", "freerl_hip.h")).read()
    assert re.search(r"\bFRL_ALGO_DDPG_POPART\s*=\s*20\b", hdr) and re.search(r"\bALGO_DDPG_POPART\s*=\s*20\b", open(os.path.join(CSRC, "frl_desc.h")).read()) and N.ALGO_DDPG_POPART == 20
    for sym in ("int frl_popart_ddpg_learn(frl_engine* e, const frl_popart_ddpg_args* args);", "int frl_popart_get(frl_engine* e, int learner, float* out5);",
                "int frl_popart_set(frl_engine* e, int learner, const float* in5);"):
        assert sym in hdr, sym
    assert [f for f, _ in dict(parse_later_structs())["frl_popart_ddpg_args"]] == FIELDS == [f[0] for f in N.PopartDdpgArgs._fields_]
    assert N.SIGNATURES["frl_popart_ddpg_learn"] == (C.c_int, [C.c_void_p, C.POINTER(N.PopartDdpgArgs)])
    assert N.SIGNATURES["frl_popart_get"][1] == N.SIGNATURES["frl_popart_set"][1] == [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    assert len(N.POPART_OUT) == 8 and callable(Engine.popart_ddpg_learn) and callable(Engine.popart_get) and callable(Engine.popart_set)
    assert subprocess.call(["python", os.path.join(ROOT, "tools", "gen_ctypes_stub.py"), "--check"]) == 0


def test_library_exports_and_unit():
    from freerl_amd import _native as N
    from freerl_amd.engine import make_config
    assert any(os.path.basename(u) == "kernels_popart.hip" for u in N.units())
    src = open(os.path.join(CSRC, "kernels_popart.hip")).read()
    for k in ("popart_target_kernel", "popart_critic_kernel", "popart_step_kernel", "popart_actor_kernel"):
        assert "void %s(" % k in src
    api = open(os.path.join(CSRC, "frl_api.hip")).read()
    assert '#include "kernels_popart.hip"' in api and '#include "frl_api_popart.inc"' in api
    N.build()
    L = C.CDLL(N.LIB_PATH)
    L.frl_version.restype, L.frl_last_error.restype = C.c_int, C.c_char_p
    assert L.frl_version() >= 115
    assert L.frl_popart_ddpg_learn(None, None) == 1 and b"engine is NULL" in L.frl_last_error()
    assert L.frl_popart_get(None, 0, None) == 1 and L.frl_popart_set(None, 0, None) == 1
    cfg, _ = make_config(N.ALGO_DDPG_POPART, [3, 3], [1, 1], 40)
    h = C.c_void_p()
    L.frl_create.argtypes = [C.POINTER(N.Config), C.POINTER(C.c_void_p)]
    assert L.frl_create(C.byref(cfg), C.byref(h)) == 1 and b"n_agents" in L.frl_last_error()


def _probe(tmp, source, *args):
    exe = tmp / source[:-4]
    if not exe.exists():
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", source), "-o", str(exe)])
    return json.loads(subprocess.check_output([str(exe)] + [str(a) for a in args]))


def test_create_time_plan_and_refusals(tmp_path):
    def run(name, algo=20, discrete=0, hidden_act=1, extra_cols=0, hidden=128):      # name algo obs act hidden batch_max P discrete hidden_act extra_cols capacity
        return _probe(tmp_path, "gail_ppo_plan_probe.cpp", name, algo, 3, 1, hidden, 256, 1, discrete, hidden_act, extra_cols, 2048)
    r = run("script")
    assert r["algo_name"] == "PopArt-DDPG" and r["learn"] == "frl_popart_ddpg_learn" and r["rollout"] == 0 and "net 1" in r["act_hint"] and r["family"] == 0
    assert [n["layers"] for n in r["nets"]] == [[[128, 3], [128, 128], [1, 128]], [[128, 4], [128, 128], [1, 128]]]
    assert [(n["hidden_act"], n["out_act"]) for n in r["nets"]] == [(1, 2), (1, 0)]      # ReLU with a tanh head; ReLU with a linear head
    for kw, text in ((dict(hidden_act=2), "PopArt-DDPG: hidden_act 2 is refused (FRL_ACT_RELU"), (dict(hidden_act=3), "hidden_act 3 is refused"),
                     (dict(discrete=1), "PopArt-DDPG: discrete is refused"), (dict(extra_cols=1), "extra_cols must be 0"), (dict(hidden=40), "multiple of 16")):
        r = run("refusal", **kw)
        assert r.get("refused") == 1 and text in r["message"], (kw, r)
    for algo in (17, 19, 21):
        assert run("unknown", algo=algo)["message"].startswith("unknown algo")


@pytest.mark.parametrize("args,rc,text", [
    ((16, 0, 40, 40, 0.99999, 0, 0), 1, "batch 0 must be >= 1"),
    ((16, 16, 40, 0, 0.99999, 0, 0), 4, "the ring of learner 1 is empty"),
    ((16, 32, 40, 40, 0.99999, 1, 0), 1, "= 32 rows > batch_max 16"),
    ((16, 16, 40, 40, "nan", 1, 0), 1, "beta is NaN"),
    ((16, 16, 40, 40, 1.5, 1, 0), 1, "beta 1.5 outside [0, 1]"),
    ((16, 16, 40, 40, 0.99999, 1, 40), 1, "sample index 40 out of range"),
    ((16, 16, 40, 20, 0.99999, 0, 0), 4, "device index draw needs len(buffer) >= 2*batch (have 20); pass idx"),
    ((16, 16, 40, 9, 0.99999, 1, -40), 0, "")])
def test_call_time_refusals(tmp_path, args, rc, text):
    r = _probe(tmp_path, "popart_plan_probe.cpp", "call", *args)
    assert r["rc"] == rc and text in r["message"], r
    if rc == 0:
        assert (r["rows"], r["ns"]) == (9, 1)          # min(len(buffer), batch) of the smallest ring; idx -40 wraps to row 0


@pytest.mark.parametrize("batch_max,rc,cps", [(16, 16, 1), (17, 16, 1), (96, 16, 3), (256, 0, 0), (1023, 64, 2)])
def test_block_layout(tmp_path, batch_max, rc, cps):
    assert _probe(tmp_path, "popart_plan_probe.cpp", "walk", batch_max, rc, cps)["ok"] == 1
