"""CPU: the C ABI of envelope multi-objective DDPG — include/freerl_hip.h declares frl_envelope_ddpg_learn,
frl_envelope_ddpg_args and FRL_ALGO_ENVELOPE_DDPG = 9 while frl_config keeps reward_dim as its LAST field,
freerl_amd/_native.py binds them, and the struct mirrors (_native.EnvelopeDdpgArgs, INTEGRATION.md's generated block) have the
C compiler's size and field offsets."""
import ctypes as C
import os
import re

from tests.test_abi_and_host import HEADER, _gcc_layout, _load_stub_tool

FIELDS = ["batch", "weight_num", "gamma", "tau", "actor_lr", "critic_lr", "beta", "idx", "weights", "critic_loss_out",
          "actor_loss_out", "weights_out"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_point():
    src = _header()
    assert re.search(r"\bFRL_ALGO_ENVELOPE_DDPG\s*=\s*9\b", src) and re.search(r"\bFRL_ALGO_ENVELOPE_DQN\s*=\s*8\b", src)
    assert re.search(r"\bint\s+frl_envelope_ddpg_learn\s*\(\s*frl_engine\s*\*\s*e\s*,\s*const\s+frl_envelope_ddpg_args\s*\*\s*args\s*\)\s*;", src)
    # declared in two steps (struct, then typedef), as frl_envelope_args is
    assert re.search(r"(?<!typedef )\bstruct\s+frl_envelope_ddpg_args\s*\{", src)
    assert re.search(r"\btypedef\s+struct\s+frl_envelope_ddpg_args\s+frl_envelope_ddpg_args\s*;", src)
    cfg = re.search(r"typedef\s+struct\s+frl_config\s*\{(.*?)\}\s*frl_config\s*;", src, flags=re.S).group(1)
    assert [d.split()[-1] for d in cfg.split(";") if d.strip()][-1] == "reward_dim"       # frl_config gained no field


def test_native_binds_it():
    from freerl_amd import _native as N
    assert N.ALGO_ENVELOPE_DDPG == 9
    res, args = N.SIGNATURES["frl_envelope_ddpg_learn"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(N.EnvelopeDdpgArgs)]
    assert [f for f, _ in N.EnvelopeDdpgArgs._fields_] == FIELDS
    assert N.Config._fields_[-1][0] == "reward_dim"
    from freerl_amd.engine import Engine
    assert callable(Engine.envelope_ddpg_learn)
    from freerl_amd import ENVELOPE_DDPG, ENVELOPE_DQN
    assert callable(ENVELOPE_DDPG.ENVELOPE_DDPG)
    assert ENVELOPE_DDPG._random_preference is ENVELOPE_DQN._random_preference       # shared, not copied
    assert ENVELOPE_DDPG._prioritised_draw is ENVELOPE_DQN._prioritised_draw


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from freerl_amd import _native as N
    want = _gcc_layout(tmp_path, [("frl_envelope_ddpg_args", [(f, None) for f in FIELDS])])
    tool = _load_stub_tool()
    later = dict(tool.parse_later_structs())
    assert [f for f, _ in later["frl_envelope_ddpg_args"]] == FIELDS      # the generator sees the struct ...
    ns = {}
    exec(tool.extract(), ns)                                              # ... and INTEGRATION.md's block carries it
    for cls in (N.EnvelopeDdpgArgs, ns["frl_envelope_ddpg_args"]):
        assert C.sizeof(cls) == want["frl_envelope_ddpg_args"][0]
        for f in FIELDS:
            assert getattr(cls, f).offset == want["frl_envelope_ddpg_args"][1][f], f


def test_kernel_unit_and_register_table():
    """The new translation unit is part of the library's build, and tools/kernel_regs.py lists its two kernels."""
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_envelope_ddpg.hip" for u in N.units())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = open(os.path.join(root, "tools", "kernel_regs.py")).read()
    assert "envelope_ddpg_critic_" in table and "envelope_ddpg_actor_" in table
