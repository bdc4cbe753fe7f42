"""CPU: the C ABI and the host plan of CEM_GD3PG — include/freerl_hip.h declares FRL_ALGO_CEM_GD3PG = 18 (17 stays unassigned), frl_cem_gd3pg_args, frl_cem_gd3pg_learn
and the four ring entry points; csrc/frl_desc.h mirrors the value; freerl_amd/_native.py binds them with the struct's fields in the header's
order, size and offsets; INTEGRATION.md's generated block is current; the library exports the symbols at frl_version() >= 114 and
kernels_cem_gd3pg.hip is a unit of the build; the refusals that need no device carry their wording (through the plan, compiled into
tests/gail_ppo_plan_probe.cpp's describer); the class and sepCEM are importable without a device."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["batch", "gamma", "tau", "actor_lr", "critic_lr", "lambda", "f1_more", "delta", "idx", "out"]
RING_CALLS = ("int frl_ring_add(frl_engine* e, int learner, int ring, const float* record);",
              "int frl_ring_cursor_get(const frl_engine* e, int learner, int ring, int* index_out, int* size_out);",
              "int frl_ring_cursor_set(frl_engine* e, int learner, int ring, int index, int size);")


def _tool():
    spec = importlib.util.spec_from_file_location("gen_ctypes_stub", os.path.join(ROOT, "tools", "gen_ctypes_stub.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_desc_and_binding_agree():
    from freerl_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "freerl_hip.h")).read()
    assert re.search(r"\bFRL_ALGO_CEM_GD3PG\s*=\s*18\b", hdr) and re.search(r"\bFRL_ALGO_GAIL_PPO\s*=\s*16\b", hdr)
    desc = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_desc.h")).read()
    assert re.search(r"\bALGO_CEM_GD3PG\s*=\s*18\b", desc)
    assert N.ALGO_CEM_GD3PG == 18
    for sym in ("int frl_cem_gd3pg_learn(frl_engine* e, const frl_cem_gd3pg_args* args);", "int frl_ring_add_batch(frl_engine* e, int ring, int n,") + RING_CALLS:
        assert sym in hdr, sym
    parsed = dict(_tool().parse_later_structs())
    assert [f for f, _ in parsed["frl_cem_gd3pg_args"]] == FIELDS == [f[0] for f in N.CemGd3pgArgs._fields_]
    assert N.SIGNATURES["frl_cem_gd3pg_learn"] == (C.c_int, [C.c_void_p, C.POINTER(N.CemGd3pgArgs)])
    assert N.SIGNATURES["frl_ring_add"][1] == [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
    assert N.SIGNATURES["frl_ring_cursor_get"][1][1:3] == [C.c_int, C.c_int] and len(N.SIGNATURES["frl_ring_cursor_set"][1]) == 5
    assert len(N.CEM_OUT) == 8 and N.CEM_OUT[6] == "KL"
    # frl_config stays as it is
    assert [f[0] for f in N.Config._fields_][-1] == "reward_dim"
    from freerl_amd.engine import Engine
    assert callable(Engine.cem_gd3pg_learn) and callable(Engine.ring_add) and callable(Engine.ring_cursor)


def test_struct_has_the_c_compilers_size_and_offsets(tmp_path):
    from freerl_amd import _native as N
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "freerl_hip.h"\nint main(void) {\n  printf("%zu", sizeof(frl_cem_gd3pg_args));\n' +
                   "".join('  printf(" %%zu", offsetof(frl_cem_gd3pg_args, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    ns = {}
    tool = _tool()
    exec(tool.extract(), ns)                                              # INTEGRATION.md's block carries the struct too
    for cls in (N.CemGd3pgArgs, ns["frl_cem_gd3pg_args"]):
        assert got[0] == C.sizeof(cls)
        assert got[1:] == [getattr(cls, f).offset for f in FIELDS]
    assert subprocess.call(["python", os.path.join(ROOT, "tools", "gen_ctypes_stub.py"), "--check"]) == 0


def test_library_exports_and_unit():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_cem_gd3pg.hip" for u in N.units())
    src = open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_cem_gd3pg.hip")).read()
    for k in ("cem_draw_kernel", "cem_critic_kernel", "cem_actor_kernel", "cem_step_kernel", "cem_act_kernel"):
        assert "void %s(" % k in src
    assert "asm" not in src
    api = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api.hip")).read()
    assert '#include "kernels_cem_gd3pg.hip"' in api and '#include "frl_api_cem_gd3pg.inc"' in api
    table = open(os.path.join(ROOT, "tools", "kernel_regs.py")).read()
    assert "cem_critic_" in table and "cem_actor_" in table
    N.build()
    L = C.CDLL(N.LIB_PATH)
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 114
    for sym in ("frl_cem_gd3pg_learn", "frl_ring_add", "frl_ring_add_batch", "frl_ring_cursor_get", "frl_ring_cursor_set"):
        assert hasattr(L, sym)
    # refusals that need no device carry a message
    L.frl_last_error.restype = C.c_char_p
    assert L.frl_cem_gd3pg_learn(None, None) == 1 and b"engine is NULL" in L.frl_last_error()
    assert L.frl_ring_cursor_get(None, 0, 0, None, None) == 1 and b"engine is NULL" in L.frl_last_error()
    assert L.frl_ring_add(None, 0, 0, None) == 1
    # frl_create's argument check runs ahead of its device check: two agents are refused by name on any machine
    cfg, _ = __import__("freerl_amd.engine", fromlist=["make_config"]).make_config(N.ALGO_CEM_GD3PG, [3, 3], [1, 1], 40, hidden_act=N.ACT_TANH)
    h = C.c_void_p()
    L.frl_create.argtypes = [C.POINTER(N.Config), C.POINTER(C.c_void_p)]
    assert L.frl_create(C.byref(cfg), C.byref(h)) == 1 and b"n_agents" in L.frl_last_error()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cem_abi") / "plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "gail_ppo_plan_probe.cpp"), "-o", str(exe)])

    def run(name, algo=18, obs=24, act=4, hidden=128, batch_max=256, P=1, discrete=0, hidden_act=2, extra_cols=0, capacity=2048):
        out = subprocess.check_output([str(exe), name] + [str(x) for x in (algo, obs, act, hidden, batch_max, P, discrete, hidden_act, extra_cols, capacity)])
        return json.loads(out)
    return run


def test_plan_of_the_scripts_shape(probe):
    r = probe("script")
    assert r["algo_name"] == "CEM-GD3PG" and r["learn"] == "frl_cem_gd3pg_learn" and r["rollout"] == 0 and "net 2" in r["act_hint"]
    assert r["n_nets"] == 4
    a1, a2, critic, dom = r["nets"]
    assert a1["layers"] == a2["layers"] == dom["layers"] == [[128, 24], [128, 128], [4, 128]] and critic["layers"] == [[128, 28], [128, 128], [1, 128]]
    assert a1["hidden_act"] == a2["hidden_act"] == dom["hidden_act"] == 2 and a1["out_act"] == 2           # tanh, tanh head
    assert critic["hidden_act"] == 3 and critic["out_act"] == 0                                         # LeakyReLU, linear head
    assert (r["width"], r["act_cols"], r["extra"]) == (24 + 4 + 1 + 1 + 24, 4, 0)
    assert r["lds_bytes"] == r["lds_for_rc"] <= 80 * 1024


def test_plan_refusals_and_their_wording(probe):
    for kw, text in ((dict(hidden_act=1), "CEM-GD3PG: hidden_act 1 is refused (FRL_ACT_TANH"), (dict(hidden_act=3), "hidden_act 3 is refused"),
                     (dict(discrete=1), "CEM-GD3PG: discrete is refused"), (dict(extra_cols=1), "extra_cols must be 0"), (dict(hidden=40), "multiple of 16")):
        r = probe("refusal", **kw)
        assert r.get("refused") == 1 and text in r["message"], (kw, r)
    for algo in (17, 19):          # 17 stays unassigned (tests/test_gail_ppo_abi.py holds it to "unknown"), 19 is the first value past the enum
        assert probe("unknown", algo=algo, hidden_act=2)["message"].startswith("unknown algo")


def test_class_and_search_need_no_device():
    from freerl_amd.CEM_GD3PG import CEM_GD3PG, sepCEM
    assert callable(CEM_GD3PG.learn) and callable(CEM_GD3PG.load)
    np.random.seed(0)
    es = sepCEM(6, mu_init=np.zeros(6), sigma_init=1e-3, pop_size=4, antithetic=True, parents=2)
    pop = es.ask(8)
    assert pop.shape == (8, 6) and pop.dtype == np.float64 and np.array_equal(pop[4:], -pop[:4])          # antithetic around mu = 0
    es.tell(pop, [1.0, 5.0, 3.0, 2.0, 0.0, -1.0, 4.0, 2.5])
    mu, cov = es.get_distrib_params()
    w = np.log(3 / np.array([1.0, 2.0])) / np.log(3 / np.array([1.0, 2.0])).sum()
    np.testing.assert_allclose(mu, w @ pop[[1, 6]], rtol=1e-15)                                          # the two best, by score
    np.testing.assert_allclose(cov, 0.5 * (w @ (pop[[1, 6]] ** 2)) + (1e-3 * 0.95 + 0.05 * 1e-5), rtol=1e-14)
    assert np.array_equal(es.elite, pop[1]) and es.elite_score == -5.0
    with pytest.raises(AssertionError):
        sepCEM(6, pop_size=5, antithetic=True)
