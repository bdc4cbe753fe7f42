"""CPU: the C ABI of REINFORCE — include/freerl_hip.h declares frl_reinforce_learn, frl_reinforce_args and
FRL_ALGO_REINFORCE = 7, freerl_amd/_native.py binds them, and the struct mirrors (_native.ReinforceArgs, INTEGRATION.md's
generated block) have the C compiler's sizes and field offsets."""
import ctypes as C
import os
import re

from tests.test_abi_and_host import HEADER, _gcc_layout, _load_stub_tool

FIELDS = ["n_steps", "gamma", "lr", "adam_eps", "loss_out", "returns_out"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_point():
    src = _header()
    assert re.search(r"\bFRL_ALGO_REINFORCE\s*=\s*7\b", src)
    assert re.search(r"\bint\s+frl_reinforce_learn\s*\(\s*frl_engine\s*\*\s*e\s*,\s*const\s+frl_reinforce_args\s*\*\s*args\s*\)\s*;", src)
    assert re.search(r"\bstruct\s+frl_reinforce_args\s*\{", src) and re.search(r"\bfrl_reinforce_args\s*;", src)


def test_native_binds_it():
    from freerl_amd import _native as N
    assert N.ALGO_REINFORCE == 7
    res, args = N.SIGNATURES["frl_reinforce_learn"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(N.ReinforceArgs)]
    assert [f for f, _ in N.ReinforceArgs._fields_] == FIELDS
    from freerl_amd.engine import Engine
    assert callable(Engine.reinforce_learn)


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from freerl_amd import _native as N
    want = _gcc_layout(tmp_path, [("frl_reinforce_args", [(f, None) for f in FIELDS])])["frl_reinforce_args"]
    tool = _load_stub_tool()
    later = dict(tool.parse_later_structs())
    assert [f for f, _ in later["frl_reinforce_args"]] == FIELDS          # the generator sees the struct ...
    ns = {}
    exec(tool.extract(), ns)                                              # ... and INTEGRATION.md's block carries it
    for cls in (N.ReinforceArgs, ns["frl_reinforce_args"]):
        assert C.sizeof(cls) == want[0]
        for f in FIELDS:
            assert getattr(cls, f).offset == want[1][f], f
    assert N.ReinforceArgs.gamma.size == 8 and want[1]["gamma"] % 8 == 0   # the scan's gamma is a double


def test_kernel_unit_and_register_table():
    """The new translation unit is part of the library's build, and tools/kernel_regs.py lists its two kernels."""
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_reinforce.hip" for u in N.units())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = open(os.path.join(root, "tools", "kernel_regs.py")).read()
    assert "reinforce_returns_kernel" in table and "reinforce_grad_kernel" in table
