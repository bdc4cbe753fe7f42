"""CPU: the C ABI of action-masked MAPPO - include/freerl_hip.h declares frl_action_mask_set and frl_act_masked while frl_mappo_args
and frl_config keep their fields, freerl_amd/_native.py binds the two entry points, the library exports them at frl_version() >= 108,
the refusals that need no device carry a message, and the new kernel unit is built and listed in tools/kernel_regs.py."""
import ctypes as C
import os
import re

from tests.test_abi_and_host import HEADER
from tests.test_mappo_abi import FIELDS as MAPPO_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_entry_points():
    src = _header()
    assert re.search(r"\bint\s+frl_action_mask_set\s*\(\s*frl_engine\s*\*\s*e\s*,\s*int\s+on\s*\)\s*;", src)
    assert re.search(r"\bint\s+frl_act_masked\s*\(\s*frl_engine\s*\*\s*e\s*,\s*int\s+net\s*,\s*int\s+n_rows\s*,\s*int\s+in_dim\s*,\s*const\s+float\s*\*\s*in_host\s*,"
                     r"\s*const\s+float\s*\*\s*mask_host\s*,\s*const\s+float\s*\*\s*eps_host\s*,\s*float\s*\*\s*out_host\s*,\s*float\s*\*\s*logp_host\s*\)\s*;", src)
    # frl_mappo_args, frl_config and frl_act are as they were
    body = re.search(r"(?<!typedef )\bstruct\s+frl_mappo_args\s*\{(.*?)\}\s*;", src, flags=re.S).group(1)
    names = [re.sub(r"[\s\*]", "", n) for d in body.split(";") if d.strip() for n in (d.split(",")[0].split()[-1:] + d.split(",")[1:])]
    assert names == MAPPO_FIELDS
    cfg = re.search(r"typedef\s+struct\s+frl_config\s*\{(.*?)\}\s*frl_config\s*;", src, flags=re.S).group(1)
    assert [d.split()[-1] for d in cfg.split(";") if d.strip()][-1] == "reward_dim"
    assert re.search(r"\bint\s+frl_act\s*\(\s*frl_engine\s*\*\s*e\s*,\s*int\s+net\s*,\s*int\s+mode\s*,\s*int\s+head\s*,\s*int\s+use_target\s*,\s*int\s+n_rows\s*,"
                     r"\s*int\s+in_dim\s*,", src)


def test_native_binds_them():
    from freerl_amd import _native as N
    fp = C.POINTER(C.c_float)
    assert N.SIGNATURES["frl_action_mask_set"] == (C.c_int, [C.c_void_p, C.c_int])
    assert N.SIGNATURES["frl_act_masked"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, fp])
    assert [f for f, _ in N.MappoArgs._fields_] == MAPPO_FIELDS
    assert N.Config._fields_[-1][0] == "reward_dim"
    from freerl_amd.engine import Engine
    assert callable(Engine.action_mask_set) and callable(Engine.act_masked)
    import freerl_amd
    from freerl_amd import IPPO, MAPPO, MAPPO_for_mask_action as M
    assert issubclass(M.MAPPO, MAPPO.MultiAgentPPO) and M.MAPPO is not MAPPO.MAPPO and M.MAPPO._algo == N.ALGO_MAPPO
    assert freerl_amd.MAPPO.MAPPO is MAPPO.MAPPO               # not re-exported over freerl_amd.MAPPO
    assert M.MAPPO._file == "MAPPO.pth"
    assert M.MAPPO.lr_decay.__code__.co_code == IPPO.IPPO.lr_decay.__code__.co_code


def test_library_exports_and_version():
    from freerl_amd import _native as N
    N.build()
    L = C.CDLL(N.LIB_PATH)
    assert hasattr(L, "frl_action_mask_set") and hasattr(L, "frl_act_masked")
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 108


def test_refusals_without_a_device():
    from freerl_amd import _native as N
    N.build()
    L = N.lib()
    assert L.frl_action_mask_set(None, 1) == 1 and b"engine is NULL" in L.frl_last_error()
    assert L.frl_act_masked(None, 0, 1, 1, None, None, None, None, None) == 1 and b"engine is NULL" in L.frl_last_error()


def test_kernel_unit_is_built_and_listed():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_mappo_mask.hip" for u in N.units())
    assert '("mappo_mask_", 0)' in open(os.path.join(ROOT, "tools", "kernel_regs.py")).read()
    src = open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_mappo_mask.hip")).read()
    assert "mappo_mask_update_kernel" in src and "mappo_mask_act_kernel" in src and "mappo_steps<false, true>" in src
