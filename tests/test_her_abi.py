"""CPU: the C ABI of hindsight relabelling - include/freerl_hip.h declares frl_her_mode, frl_her_args and frl_her_relabel,
freerl_amd/_native.py binds them and its struct mirror has the C compiler's size and offsets, the library exports the symbol at
frl_version() >= 112, the refusals that need no device carry a message, and the kernel unit is built, listed and wired in."""
import ctypes as C
import inspect
import os
import re
import subprocess

from tests.test_abi_and_host import HEADER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["n_episodes", "learners", "lengths", "state_dim", "goal_dim", "sample_num", "sample_range", "mode", "weights", "tolerance",
          "env_actions", "picks", "rows_out"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_call():
    src = _header()
    body = re.search(r"(?<!typedef )\bstruct\s+frl_her_args\s*\{(.*?)\}\s*;", src, flags=re.S).group(1)
    names = [re.sub(r"[\s\*]", "", n) for d in body.split(";") if d.strip() for n in (d.split(",")[0].split()[-1:] + d.split(",")[1:])]
    assert names == FIELDS
    assert re.search(r"typedef\s+struct\s+frl_her_args\s+frl_her_args\s*;", src)
    enum = re.search(r"\benum\s+frl_her_mode\s*\{(.*?)\}", src, flags=re.S).group(1)
    assert re.sub(r"\s", "", enum) == "FRL_HER_SPARSE=0,FRL_HER_SHAPING=1"
    assert re.search(r"\bint\s+frl_her_relabel\s*\(\s*frl_engine\s*\*\s*e\s*,\s*const\s+frl_her_args\s*\*\s*args\s*\)\s*;", src)


def test_native_mirror_has_the_c_layout(tmp_path):
    from freerl_amd import _native as N
    assert N.SIGNATURES["frl_her_relabel"] == (C.c_int, [C.c_void_p, C.POINTER(N.HerArgs)])
    assert [f for f, _ in N.HerArgs._fields_] == FIELDS and (N.HER_SPARSE, N.HER_SHAPING) == (0, 1)
    probe = tmp_path / "her.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "freerl_hip.h"\nint main(void){printf("%zu", sizeof(frl_her_args));'
                     + "".join('printf(" %%zu", offsetof(frl_her_args, %s));' % f for f in FIELDS)
                     + 'printf(" %d %d\\n", (int)FRL_HER_SPARSE, (int)FRL_HER_SHAPING); return 0;}')
    exe = tmp_path / "her"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(N.HerArgs)] + [getattr(N.HerArgs, f).offset for f in FIELDS] + [0, 1]
    from freerl_amd.engine import Engine
    sig = inspect.signature(Engine.her_relabel).parameters
    assert list(sig)[1:3] == ["learners", "lengths"] and {"state_dim", "goal_dim", "sample_num", "sample_range", "mode", "weights", "tolerance",
                                                           "env_actions", "picks"} <= set(sig)


def test_library_exports_and_version():
    from freerl_amd import _native as N
    N.build()
    L = C.CDLL(N.LIB_PATH)
    assert hasattr(L, "frl_her_relabel")
    L.frl_version.restype = C.c_int
    assert L.frl_version() >= 112


def test_refusal_without_a_device():
    from freerl_amd import _native as N
    N.build()
    L = N.lib()
    assert L.frl_her_relabel(None, None) == 1 and b"engine is NULL" in L.frl_last_error()


def test_kernel_unit_is_built_listed_and_wired():
    from freerl_amd import _native as N
    assert any(os.path.basename(u) == "kernels_her.hip" for u in N.units())
    csrc = os.path.join(ROOT, "freerl_amd", "csrc")
    assert "her_relabel_kernel" in open(os.path.join(csrc, "kernels_her.hip")).read()
    assert "her_relabel_kernel" in open(os.path.join(csrc, "kernels.h")).read()
    api = open(os.path.join(csrc, "frl_api.hip")).read()
    assert '#include "kernels_her.hip"' in api and '#include "frl_api_her.inc"' in api and '#include "her_plan.h"' in api
    assert '("her_", 0)' in open(os.path.join(ROOT, "tools", "kernel_regs.py")).read()
