"""CPU: the C ABI of MAPPO / IPPO — include/freerl_hip.h declares FRL_ALGO_MAPPO = 11, FRL_ALGO_IPPO = 12, frl_mappo_learn,
frl_mappo_args and frl_net_norm_set while frl_config keeps reward_dim as its LAST field, freerl_amd/_native.py binds them, the struct
mirrors (_native.MappoArgs, INTEGRATION.md's generated block) have the C compiler's size and field offsets, and the refusals that
need no device are reachable."""
import ctypes as C
import os
import re

from tests.test_abi_and_host import HEADER, _gcc_layout, _load_stub_tool

FIELDS = ["horizon", "minibatch", "k_epochs", "gamma", "lmbda", "clip", "ent_coef", "actor_lr", "critic_lr", "adam_eps", "clip_norm",
          "adv_norm", "value_clip", "loss_kind", "huber_delta", "perms", "adv_out", "vtarget_out", "loss_trace_out"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    assert re.search(r"\bFRL_ALGO_MAPPO\s*=\s*11\b", src) and re.search(r"\bFRL_ALGO_IPPO\s*=\s*12\b", src)
    assert re.search(r"\bFRL_ALGO_GAIL\s*=\s*10\b", src)
    assert re.search(r"\bint\s+frl_mappo_learn\s*\(\s*frl_engine\s*\*\s*e\s*,\s*const\s+frl_mappo_args\s*\*\s*args\s*\)\s*;", src)
    assert re.search(r"\bint\s+frl_net_norm_set\s*\(\s*frl_engine\s*\*\s*e\s*,\s*int\s+feature_norm\s*,\s*int\s+layer_norm\s*\)\s*;", src)
    assert re.search(r"(?<!typedef )\bstruct\s+frl_mappo_args\s*\{", src)
    assert re.search(r"\btypedef\s+struct\s+frl_mappo_args\s+frl_mappo_args\s*;", src)
    cfg = re.search(r"typedef\s+struct\s+frl_config\s*\{(.*?)\}\s*frl_config\s*;", src, flags=re.S).group(1)
    assert [d.split()[-1] for d in cfg.split(";") if d.strip()][-1] == "reward_dim"       # frl_config gained no field


def test_native_binds_them():
    from freerl_amd import _native as N
    assert (N.ALGO_MAPPO, N.ALGO_IPPO) == (11, 12)
    res, args = N.SIGNATURES["frl_mappo_learn"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(N.MappoArgs)]
    res, args = N.SIGNATURES["frl_net_norm_set"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int]
    assert [f for f, _ in N.MappoArgs._fields_] == FIELDS
    assert N.Config._fields_[-1][0] == "reward_dim"
    from freerl_amd.engine import Engine
    assert callable(Engine.mappo_learn) and callable(Engine.net_norm_set)


def test_library_exports_and_version():
    from freerl_amd import _native as N
    N.build()
    L = C.CDLL(N.LIB_PATH)
    assert hasattr(L, "frl_mappo_learn") and hasattr(L, "frl_net_norm_set")
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 106


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from freerl_amd import _native as N
    want = _gcc_layout(tmp_path, [("frl_mappo_args", [(f, None) for f in FIELDS])])
    tool = _load_stub_tool()
    later = dict(tool.parse_later_structs())
    assert [f for f, _ in later["frl_mappo_args"]] == FIELDS              # the generator sees the struct ...
    ns = {}
    exec(tool.extract(), ns)                                              # ... and INTEGRATION.md's block carries it
    for cls in (N.MappoArgs, ns["frl_mappo_args"]):
        assert C.sizeof(cls) == want["frl_mappo_args"][0]
        for f in FIELDS:
            assert getattr(cls, f).offset == want["frl_mappo_args"][1][f], f


def test_refusals_without_a_device():
    """NULL arguments are refused before the engine is looked at, with a message; a NULL config creates nothing"""
    from freerl_amd import _native as N
    N.build()
    L = N.lib()
    assert L.frl_mappo_learn(None, None) == 1 and b"engine is NULL" in L.frl_last_error()
    assert L.frl_net_norm_set(None, 1, 1) == 1 and b"engine is NULL" in L.frl_last_error()
    h = C.c_void_p()
    assert L.frl_create(None, C.byref(h)) == 1 and not h.value


def test_kernel_unit_is_built():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_mappo.hip" for u in N.units())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = open(os.path.join(root, "tools", "kernel_regs.py")).read()
    assert "mappo_update_" in table and "mappo_values_" in table and "mappo_act_" in table
