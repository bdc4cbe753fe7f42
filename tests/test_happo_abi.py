"""CPU: the C ABI of HAPPO - include/freerl_hip.h declares FRL_ALGO_HAPPO = 13, frl_happo_args (frl_mappo_args' fields, then
agent_order and factor_out) and frl_happo_learn while frl_config keeps reward_dim as its LAST field, freerl_amd/_native.py binds them
with the same field order, the struct mirrors have the C compiler's size and field offsets, and the refusals that need no device are
reachable."""
import ctypes as C
import os
import re

from tests.test_abi_and_host import HEADER, _gcc_layout, _load_stub_tool
from tests.test_mappo_abi import FIELDS as MAPPO_FIELDS

FIELDS = MAPPO_FIELDS + ["agent_order", "factor_out"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_point():
    src = _header()
    assert re.search(r"\bFRL_ALGO_HAPPO\s*=\s*13\b", src) and re.search(r"\bFRL_ALGO_IPPO\s*=\s*12\b", src)
    assert re.search(r"\bint\s+frl_happo_learn\s*\(\s*frl_engine\s*\*\s*e\s*,\s*const\s+frl_happo_args\s*\*\s*args\s*\)\s*;", src)
    body = re.search(r"(?<!typedef )\bstruct\s+frl_happo_args\s*\{(.*?)\}\s*;", src, flags=re.S).group(1)
    names = [re.sub(r"[\s\*]", "", n) for d in body.split(";") if d.strip() for n in (d.split(",")[0].split()[-1:] + d.split(",")[1:])]
    assert names == FIELDS
    assert re.search(r"\btypedef\s+struct\s+frl_happo_args\s+frl_happo_args\s*;", src)
    assert re.search(r"const\s+int32_t\s*\*\s*agent_order\s*;", src) and re.search(r"float\s*\*\s*factor_out\s*;", src)
    cfg = re.search(r"typedef\s+struct\s+frl_config\s*\{(.*?)\}\s*frl_config\s*;", src, flags=re.S).group(1)
    assert [d.split()[-1] for d in cfg.split(";") if d.strip()][-1] == "reward_dim"       # frl_config gained no field


def test_native_binds_it():
    from freerl_amd import _native as N
    assert N.ALGO_HAPPO == 13
    res, args = N.SIGNATURES["frl_happo_learn"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(N.HappoArgs)]
    assert [f for f, _ in N.HappoArgs._fields_] == FIELDS
    assert N.HappoArgs._fields_[:len(MAPPO_FIELDS)] == N.MappoArgs._fields_
    assert N.Config._fields_[-1][0] == "reward_dim"
    from freerl_amd.engine import Engine
    assert callable(Engine.happo_learn)
    from freerl_amd import HAPPO, IPPO, MAPPO
    assert issubclass(HAPPO.HAPPO, MAPPO.MultiAgentPPO) and HAPPO.HAPPO._algo == 13 and HAPPO.HAPPO._file == "HAPPO.pth"
    assert HAPPO.HAPPO.lr_decay is IPPO.IPPO.lr_decay


def test_library_exports_and_version():
    from freerl_amd import _native as N
    N.build()
    L = C.CDLL(N.LIB_PATH)
    assert hasattr(L, "frl_happo_learn")
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 107


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from freerl_amd import _native as N
    want = _gcc_layout(tmp_path, [("frl_happo_args", [(f, None) for f in FIELDS]), ("frl_mappo_args", [(f, None) for f in MAPPO_FIELDS])])
    tool = _load_stub_tool()
    later = dict(tool.parse_later_structs())
    assert [f for f, _ in later["frl_happo_args"]] == FIELDS
    ns = {}
    exec(tool.extract(), ns)
    for cls in (N.HappoArgs, ns["frl_happo_args"]):
        assert C.sizeof(cls) == want["frl_happo_args"][0]
        for f in FIELDS:
            assert getattr(cls, f).offset == want["frl_happo_args"][1][f], f
    # the library copies frl_mappo_args' fields out of the front of a frl_happo_args
    assert want["frl_happo_args"][1]["agent_order"] == want["frl_mappo_args"][0]
    for f in MAPPO_FIELDS:
        assert want["frl_happo_args"][1][f] == want["frl_mappo_args"][1][f], f


def test_refusals_without_a_device():
    from freerl_amd import _native as N
    N.build()
    L = N.lib()
    assert L.frl_happo_learn(None, None) == 1 and b"engine is NULL" in L.frl_last_error()


def test_kernel_unit_is_built_and_the_train_flags_are_the_scripts():
    from freerl_amd import _native as N
    from freerl_amd import train
    assert any(os.path.basename(u) == "kernels_happo.hip" for u in N.units())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert '("happo_", 0)' in open(os.path.join(root, "tools", "kernel_regs.py")).read()
    a = train.build_parser("happo").parse_args([])               # HAPPO.py:547-583
    assert (a.env_name, a.policy_name, a.continuous_actions, a.max_episodes, a.save_freq) == ("simple_spread_v3", "HAPPO", False, 120000, 1250)
    assert (a.actor_lr, a.critic_lr, a.gamma, a.horizon, a.minibatch_size, a.K_epochs, a.lmbda, a.huber_delta) == (1e-4, 1e-4, 0.95, 256, 256, 15, 0.95, 10.0)
    assert train.build_parser("happo").parse_args(["--continuous_actions", "0"]).continuous_actions is True      # type=bool, as in the script
