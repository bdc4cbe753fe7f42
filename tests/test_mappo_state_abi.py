"""CPU: the C ABI of MAPPO with a global-state critic - include/freerl_hip.h declares frl_config_ext, frl_state_rows, frl_create_ex
and frl_state_info while frl_config, frl_mappo_args and frl_record_layout keep their fields; freerl_amd/_native.py binds them and its
struct mirror has the C compiler's size and offsets; the library exports them at frl_version() >= 109; the refusals that need no device
carry a message; the new kernel unit is built and listed in tools/kernel_regs.py."""
import ctypes as C
import os
import re
import subprocess

from tests.test_abi_and_host import HEADER
from tests.test_mappo_abi import FIELDS as MAPPO_FIELDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_FIELDS = ["size", "state_dim", "state_rows"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _fields(body):
    return [re.sub(r"[\s\*]", "", n) for d in body.split(";") if d.strip() for n in (d.split(",")[0].split()[-1:] + d.split(",")[1:])]


def test_header_declares_the_extension():
    src = _header()
    body = re.search(r"\bstruct\s+frl_config_ext\s*\{(.*?)\}", src, flags=re.S).group(1)
    assert _fields(body) == EXT_FIELDS and all(d.split()[0] == "int" for d in body.split(";") if d.strip())
    assert re.search(r"\}\s*frl_config_ext\s*;|typedef\s+struct\s+frl_config_ext\s+frl_config_ext\s*;", src)
    enum = re.search(r"\benum\s+frl_state_rows\s*\{(.*?)\}", src, flags=re.S).group(1)
    assert re.sub(r"\s", "", enum) == "FRL_STATE_ROWS_POSITION=0,FRL_STATE_ROWS_SAMPLE=1"
    assert re.search(r"\bint\s+frl_create_ex\s*\(\s*const\s+frl_config\s*\*\s*cfg\s*,\s*const\s+frl_config_ext\s*\*\s*ext\s*,\s*frl_engine\s*\*\*\s*out\s*\)\s*;", src)
    assert re.search(r"\bint\s+frl_state_info\s*\(\s*const\s+frl_engine\s*\*\s*e\s*,\s*int\s*\*\s*state_dim_out\s*,\s*int\s*\*\s*state_col_out\s*\)\s*;", src)
    # frl_config, frl_mappo_args, frl_record_layout and frl_create are as they were
    cfg = re.search(r"typedef\s+struct\s+frl_config\s*\{(.*?)\}\s*frl_config\s*;", src, flags=re.S).group(1)
    assert [d.split()[-1] for d in cfg.split(";") if d.strip()][-1] == "reward_dim"
    body = re.search(r"(?<!typedef )\bstruct\s+frl_mappo_args\s*\{(.*?)\}\s*;", src, flags=re.S).group(1)
    assert _fields(body) == MAPPO_FIELDS
    lay = re.search(r"typedef\s+struct\s+frl_record_layout\s*\{(.*?)\}\s*frl_record_layout\s*;", src, flags=re.S).group(1)
    assert _fields(lay)[-2:] == ["extra_off", "extra"] and len(_fields(lay)) == 12
    assert re.search(r"\bint\s+frl_create\s*\(\s*const\s+frl_config\s*\*\s*cfg\s*,\s*frl_engine\s*\*\*\s*out\s*\)\s*;", src)


def test_native_binds_them(tmp_path):
    from freerl_amd import _native as N
    ip = C.POINTER(C.c_int)
    assert N.SIGNATURES["frl_create_ex"] == (C.c_int, [C.POINTER(N.Config), C.POINTER(N.ConfigExt), C.POINTER(C.c_void_p)])
    assert N.SIGNATURES["frl_state_info"] == (C.c_int, [C.c_void_p, ip, ip])
    assert [f for f, _ in N.ConfigExt._fields_] == EXT_FIELDS
    assert (N.STATE_ROWS_POSITION, N.STATE_ROWS_SAMPLE) == (0, 1)
    assert N.Config._fields_[-1][0] == "reward_dim" and [f for f, _ in N.MappoArgs._fields_] == MAPPO_FIELDS
    # the mirror against the C compiler's view of the header
    probe = tmp_path / "ext.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "freerl_hip.h"\nint main(void){'
                     'printf("%zu %zu %zu %zu %d %d\\n", sizeof(frl_config_ext), offsetof(frl_config_ext, size), offsetof(frl_config_ext, state_dim),'
                     ' offsetof(frl_config_ext, state_rows), (int)FRL_STATE_ROWS_POSITION, (int)FRL_STATE_ROWS_SAMPLE); return 0;}')
    exe = tmp_path / "ext"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(N.ConfigExt), N.ConfigExt.size.offset, N.ConfigExt.state_dim.offset, N.ConfigExt.state_rows.offset, 0, 1]
    from freerl_amd.engine import Engine
    assert callable(Engine.state_info)
    import inspect
    assert {"state_dim", "state_rows"} <= set(inspect.signature(Engine.__init__).parameters)


def test_the_class():
    import inspect
    import freerl_amd
    from freerl_amd import MAPPO, MAPPO_for_mask_action as M, MAPPO_for_mask_action_state as S
    assert issubclass(S.MAPPO, M.MAPPO) and S.MAPPO is not M.MAPPO and S.MAPPO._algo == M.MAPPO._algo
    assert freerl_amd.MAPPO.MAPPO is MAPPO.MAPPO               # not re-exported over freerl_amd.MAPPO
    sig = inspect.signature(S.MAPPO.__init__).parameters
    assert list(sig)[1:9] == ["dim_info", "is_continue", "actor_lr", "critic_lr", "horizon", "device", "trick", "state_dim"]
    assert sig["state_dim"].default is None and sig["state_rows"].default == "position" and sig["state_rows"].kind == inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(S.MAPPO.add).parameters)[-2:] == ["avail_actions", "state"]
    for name in ("select_action", "evaluate_action", "lr_decay", "save", "load"):      # inherited
        assert name not in vars(S.MAPPO)
    assert "no port" not in M.__doc__ and "MAPPO_for_mask_action_state" in M.__doc__


def test_library_exports_and_version():
    from freerl_amd import _native as N
    N.build()
    L = C.CDLL(N.LIB_PATH)
    assert hasattr(L, "frl_create_ex") and hasattr(L, "frl_state_info")
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 109


def test_refusals_without_a_device():
    from freerl_amd import _native as N
    N.build()
    L = N.lib()
    h = C.c_void_p()
    cfg, ext = N.Config(), N.ConfigExt(C.sizeof(N.ConfigExt), 3, 0)
    assert L.frl_create_ex(None, C.byref(ext), C.byref(h)) == 1 and b"cfg/out is NULL" in L.frl_last_error()
    assert L.frl_create_ex(C.byref(cfg), C.byref(ext), None) == 1 and b"cfg/out is NULL" in L.frl_last_error()
    assert L.frl_state_info(None, None, None) == 1 and b"engine is NULL" in L.frl_last_error()
    # the extension block is judged before a device is looked for
    cfg.algo, cfg.n_learners, cfg.n_agents, cfg.capacity = N.ALGO_MAPPO, 1, 1, 8
    cfg.obs_dim[0], cfg.act_dim[0] = 3, 2
    for bad, msg in ((N.ConfigExt(8, 3, 0), b"frl_config_ext.size"), (N.ConfigExt(12, -1, 0), b"state_dim -1"), (N.ConfigExt(12, 3, 2), b"state_rows 2")):
        assert L.frl_create_ex(C.byref(cfg), C.byref(bad), C.byref(h)) == 1 and msg in L.frl_last_error(), L.frl_last_error()
        assert not h.value
    cfg.algo = N.ALGO_TD3
    assert L.frl_create_ex(C.byref(cfg), C.byref(ext), C.byref(h)) == 1 and b"FRL_ALGO_MAPPO" in L.frl_last_error() and not h.value


def test_kernel_unit_is_built_and_listed():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_mappo_state.hip" for u in N.units())
    assert '("mappo_state_", 0)' in open(os.path.join(ROOT, "tools", "kernel_regs.py")).read()
    src = open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_mappo_state.hip")).read()
    for k in ("mappo_state_values_kernel", "mappo_state_update_kernel", "mappo_state_mask_update_kernel", "mappo_steps<false, false, true>", "mappo_steps<false, true, true>"):
        assert k in src
    # the existing instantiations stay as written
    assert "mappo_steps<false, true>(" in open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_mappo_mask.hip")).read()
    assert "mappo_steps<false>(" in open(os.path.join(ROOT, "freerl_amd", "csrc", "kernels_mappo.hip")).read()
    api = open(os.path.join(ROOT, "freerl_amd", "csrc", "frl_api.hip")).read()
    assert '#include "kernels_mappo_state.hip"' in api and "return 109;" in api
