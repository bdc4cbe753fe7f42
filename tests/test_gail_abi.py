"""CPU: the C ABI of GAIL's discriminator — include/freerl_hip.h declares frl_gail_learn, frl_gail_reward, frl_gail_args,
FRL_ALGO_GAIL = 10 and FRL_ACT_LEAKY_RELU = 3 while frl_config keeps reward_dim as its LAST field, freerl_amd/_native.py binds them,
and the struct mirrors (_native.GailArgs, INTEGRATION.md's generated block) have the C compiler's size and field offsets."""
import ctypes as C
import os
import re

from tests.test_abi_and_host import HEADER, _gcc_layout, _load_stub_tool

FIELDS = ["n_expert", "n_policy", "gp", "gp_weight", "lr", "beta1", "beta2", "adam_eps", "idx", "policy_rows", "out", "idx_out"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    assert re.search(r"\bFRL_ALGO_GAIL\s*=\s*10\b", src) and re.search(r"\bFRL_ALGO_ENVELOPE_DDPG\s*=\s*9\b", src)
    assert re.search(r"\bFRL_ACT_LEAKY_RELU\s*=\s*3\b", src)
    assert re.search(r"\bint\s+frl_gail_learn\s*\(\s*frl_engine\s*\*\s*e\s*,\s*const\s+frl_gail_args\s*\*\s*args\s*\)\s*;", src)
    assert re.search(r"\bint\s+frl_gail_reward\s*\(\s*frl_engine\s*\*\s*e\s*,\s*int\s+gp\s*,\s*int\s+n_rows\s*,\s*const\s+float\s*\*\s*rows_host\s*,\s*float\s*\*\s*reward_out\s*\)\s*;", src)
    assert re.search(r"(?<!typedef )\bstruct\s+frl_gail_args\s*\{", src)
    assert re.search(r"\btypedef\s+struct\s+frl_gail_args\s+frl_gail_args\s*;", src)
    cfg = re.search(r"typedef\s+struct\s+frl_config\s*\{(.*?)\}\s*frl_config\s*;", src, flags=re.S).group(1)
    assert [d.split()[-1] for d in cfg.split(";") if d.strip()][-1] == "reward_dim"       # frl_config gained no field


def test_native_binds_them():
    from freerl_amd import _native as N
    assert N.ALGO_GAIL == 10 and N.ACT_LEAKY_RELU == 3
    res, args = N.SIGNATURES["frl_gail_learn"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(N.GailArgs)]
    res, args = N.SIGNATURES["frl_gail_reward"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    assert [f for f, _ in N.GailArgs._fields_] == FIELDS
    assert N.Config._fields_[-1][0] == "reward_dim"
    from freerl_amd.engine import Engine
    assert callable(Engine.gail_learn) and callable(Engine.gail_reward)
    from freerl_amd import GAIL
    assert callable(GAIL.GAIL) and callable(GAIL.ExpertDataset) and GAIL.GP_WEIGHT == 5.0


def test_library_exports_and_version():
    from freerl_amd import _native as N
    N.build()
    L = C.CDLL(N.LIB_PATH)
    assert hasattr(L, "frl_gail_learn") and hasattr(L, "frl_gail_reward")
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 105


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from freerl_amd import _native as N
    want = _gcc_layout(tmp_path, [("frl_gail_args", [(f, None) for f in FIELDS])])
    tool = _load_stub_tool()
    later = dict(tool.parse_later_structs())
    assert [f for f, _ in later["frl_gail_args"]] == FIELDS               # the generator sees the struct ...
    ns = {}
    exec(tool.extract(), ns)                                              # ... and INTEGRATION.md's block carries it
    for cls in (N.GailArgs, ns["frl_gail_args"]):
        assert C.sizeof(cls) == want["frl_gail_args"][0]
        for f in FIELDS:
            assert getattr(cls, f).offset == want["frl_gail_args"][1][f], f


def test_kernel_unit_and_register_table():
    """The new translation unit is part of the library's build, and tools/kernel_regs.py lists its kernels."""
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_gail.hip" for u in N.units())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = open(os.path.join(root, "tools", "kernel_regs.py")).read()
    assert "gail_disc_" in table and "gail_forward_" in table
