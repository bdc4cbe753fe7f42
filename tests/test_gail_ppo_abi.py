"""CPU: the C ABI and the host plan of GAIL's policy side — include/freerl_hip.h declares FRL_ALGO_GAIL_PPO = 16, frl_gail_ppo_args,
frl_gail_ppo_learn and the log_std range accessors; csrc/frl_desc.h mirrors the value; freerl_amd/_native.py binds them with the struct's
fields in the header's order, size and offsets; INTEGRATION.md's generated block is current; the library exports the symbols at
frl_version() >= 113 and kernels_gail_ppo.hip is a unit of the build; and the create-time plan (csrc/engine_plan.hpp through
tests/gail_ppo_plan_probe.cpp) accepts and refuses what it should, without a GPU — every other algorithm still refuses LeakyReLU."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["horizon", "minibatch", "k_epochs", "gamma", "lam", "clip", "ent_weight", "value_loss_coef", "p_lr", "v_lr", "clip_norm", "last_value",
          "rewards", "perms", "adv_out", "returns_out", "logp_old_out", "loss_trace_out"]


def _tool():
    spec = importlib.util.spec_from_file_location("gen_ctypes_stub", os.path.join(ROOT, "tools", "gen_ctypes_stub.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_desc_and_binding_agree():
    from freerl_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "freerl_hip.h")).read()
    assert re.search(r"\bFRL_ALGO_GAIL_PPO\s*=\s*16\b", hdr) and re.search(r"\bFRL_ALGO_MASAC\s*=\s*15\b", hdr)
    desc = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_desc.h")).read()
    assert re.search(r"\bALGO_GAIL_PPO\s*=\s*16\b", desc)
    assert N.ALGO_GAIL_PPO == 16
    for sym in ("int frl_gail_ppo_learn(frl_engine* e, const frl_gail_ppo_args* args);", "int frl_log_std_range_set(frl_engine* e, float lo, float hi);",
                "int frl_log_std_range_get(const frl_engine* e, float* lo_out, float* hi_out);"):
        assert sym in hdr, sym
    # the struct: the header's field order is the binding's
    parsed = dict(_tool().parse_later_structs())
    assert [f for f, _ in parsed["frl_gail_ppo_args"]] == FIELDS == [f[0] for f in N.GailPpoArgs._fields_]
    assert N.SIGNATURES["frl_gail_ppo_learn"][1][1] == C.POINTER(N.GailPpoArgs)
    assert N.SIGNATURES["frl_log_std_range_set"][1][1:] == [C.c_float, C.c_float]
    # no existing struct grew
    assert [f[0] for f in N.Config._fields_][-1] == "reward_dim" and [f[0] for f in N.PpoArgs._fields_][-1] == "gae_lmbda"


def test_struct_has_the_c_compilers_size_and_offsets(tmp_path):
    from freerl_amd import _native as N
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "freerl_hip.h"\nint main(void) {\n  printf("%zu", sizeof(frl_gail_ppo_args));\n' +
                   "".join('  printf(" %%zu", offsetof(frl_gail_ppo_args, %s));\n' % f for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(N.GailPpoArgs)
    assert got[1:] == [getattr(N.GailPpoArgs, f).offset for f in FIELDS]


def test_integration_document_is_current():
    tool = _tool()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index(tool.BEGIN):doc.index(tool.END)]
    assert "class frl_gail_ppo_args(C.Structure):" in block
    assert subprocess.call(["python", os.path.join(ROOT, "tools", "gen_ctypes_stub.py"), "--check"]) == 0


def test_library_exports_and_unit():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_gail_ppo.hip" for u in N.units())
    src = open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_gail_ppo.hip")).read()
    for k in ("gail_ppo_prepare_kernel", "gail_ppo_gae_kernel", "gail_ppo_update_kernel", "gail_ppo_act_kernel"):
        assert k in src
    assert "asm" not in src
    assert src.count("mlp_bwd(") == 1            # one backward call site for both nets and both distributions
    api = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api.hip")).read()
    assert '#include "kernels_gail_ppo.hip"' in api and '#include "frl_api_gail_ppo.inc"' in api
    # gae_scan moved to a device header; kernels_ppo.hip uses it from there
    assert "gae_scan(" in open(os.path.join(ROOT, "freerl_amd", "csrc", "device", "gae.hpp")).read()
    assert '#include "device/gae.hpp"' in open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_ppo.hip")).read()
    N.build()
    L = C.CDLL(N.LIB_PATH)
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 113
    for sym in ("frl_gail_ppo_learn", "frl_log_std_range_set", "frl_log_std_range_get"):
        assert hasattr(L, sym)
    # refusals that need no device carry a message
    L.frl_last_error.restype = C.c_char_p
    assert L.frl_gail_ppo_learn(None, None) == 1 and b"engine is NULL" in L.frl_last_error()
    assert L.frl_log_std_range_get(None, None, None) == 1


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gail_ppo_plan") / "gail_ppo_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "gail_ppo_plan_probe.cpp"), "-o", str(exe)])

    def run(name, algo=16, obs=3, act=1, hidden=128, batch_max=64, P=1, discrete=0, hidden_act=3, extra_cols=0, capacity=2048):
        out = subprocess.check_output([str(exe), name] + [str(x) for x in (algo, obs, act, hidden, batch_max, P, discrete, hidden_act, extra_cols, capacity)])
        return json.loads(out)
    return run


def test_plan_of_the_scripts_shape(probe):
    r = probe("script")
    assert r["algo_name"] == "GAIL-PPO" and r["learn"] == "frl_gail_ppo_learn" and r["rollout"] == 0 and r["act_hint"]
    assert r["n_nets"] == 2 and r["n_discrete"] == 0 and (r["log_std_min"], r["log_std_max"]) == (-10, 2)
    actor, critic = r["nets"]
    assert actor["layers"] == [[128, 3], [128, 128], [1, 128]] and critic["layers"] == [[128, 3], [128, 128], [1, 128]]
    assert actor["hidden_act"] == critic["hidden_act"] == 3 and actor["out_act"] == 2 and critic["out_act"] == 0      # LeakyReLU; tanh on the mean
    assert actor["extra_n"] == 1 and actor["extra_off"] > 0 and critic["extra_n"] == 0
    # the standard record, nothing behind next_obs: [obs 3 | act 1 | rew | done | next_obs 3]
    assert (r["width"], r["act_cols"], r["extra"], r["rew_off"], r["done_off"]) == (9, 1, 0, 4, 5)
    # a minibatch of 64 rows is ONE row chunk, as on a FRL_ALGO_PPO engine of the same dims (two chunks cost 15 % of the call: profiles/gail_ppo)
    assert r["lds_bytes"] == r["lds_for_rc"] <= 80 * 1024 and r["row_chunk"] == 64
    relu = probe("relu", hidden_act=1)
    assert relu["nets"][0]["hidden_act"] == 1


@pytest.mark.parametrize("shape", [dict(obs=17, act=6, hidden=64, batch_max=24), dict(obs=8, act=17, hidden=128, batch_max=33), dict(obs=3, act=1, hidden=256, batch_max=64, P=64),
                                   dict(obs=4, act=5, hidden=32, batch_max=7, discrete=1), dict(obs=4, act=2, hidden=32, batch_max=7, discrete=1)],
                         ids=lambda s: "-".join("%s%s" % kv for kv in s.items()))
def test_plan_accepts_the_tested_shapes(probe, shape):
    r = probe("shape", **shape)
    assert "refused" not in r, r
    # the head delta's staging row: the padded logits when discrete, the log_std terms' act_dim columns otherwise
    assert r["lds_act_pad"] >= ((shape["act"] + 15) // 16 * 16 if shape.get("discrete") else shape["act"])
    assert r["lds_bytes"] <= 160 * 1024
    if shape.get("discrete"):
        assert r["n_discrete"] == shape["act"] and r["cat_logits"] == 1 and r["act_cols"] == 1 and r["nets"][0]["extra_n"] == 0 and r["nets"][0]["out_act"] == 0


def test_plan_refusals(probe):
    for kw, text in ((dict(hidden_act=2), "GAIL-PPO: hidden_act FRL_ACT_TANH is refused"), (dict(hidden=512), "hidden 512 > 256"),
                     (dict(extra_cols=1), "extra_cols 1 must be 0"), (dict(discrete=1, act=1), "needs act_dim >= 2"),
                     (dict(discrete=1, act=65), "65 actions > 64"), (dict(hidden=40), "multiple of 16"), (dict(hidden_act=0), "hidden_act 0 is refused")):
        r = probe("refusal", **kw)
        assert r.get("refused") == 1 and text in r["message"], (kw, r)


def test_every_other_algorithm_still_refuses_leaky_relu_but_gail(probe):
    """The walk over algorithms with this engine's own configuration: LeakyReLU stays GAIL's (10) and GAIL-PPO's (16)."""
    for algo in range(0, 17):
        kw = dict(extra_cols=2) if algo == 5 else {}
        r = probe("walk", algo=algo, **kw)
        if algo in (10, 16):
            assert "refused" not in r, (algo, r)
        else:
            assert r.get("refused") == 1, (algo, r)
    r = probe("ppo", algo=5, extra_cols=2)
    assert "FRL_ACT_LEAKY_RELU" in r["message"] and "PPO engines do not take it" in r["message"]
    assert probe("unknown", algo=17)["message"].startswith("unknown algo")


def test_class_refusals_need_no_device():
    from freerl_amd.PPO2 import PPO
    base = dict(seed=0, s_dim=3, a_dim=1, PPO=dict(policy_mlp_dim=32, activation="LeakyReLU", dropout=0.0, layernorm=False, log_std_min=-10, log_std_max=2,
                                                     p_lr=1e-3, v_lr=1e-3, horizon=64, mini_batch_size=16))
    for bad in (dict(activation="Tanh"), dict(layernorm=True), dict(dropout=0.1)):
        with pytest.raises(ValueError):
            PPO(dict(base, PPO=dict(base["PPO"], **bad)))
    with pytest.raises(ValueError, match="at least 2 logits"):
        PPO(dict(base, discrete=True))
