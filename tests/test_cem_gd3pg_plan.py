"""CPU: every address kernels_cem_gd3pg.hip forms, walked against the plan's buffer sizes before anything runs on a GPU.

tests/cem_gd3pg_plan_probe.cpp is plain C++17 over csrc/engine_plan.hpp and csrc/rowchunk_layout.h — the headers the kernels and
frl_create share — compiled with g++ under AddressSanitizer + UBSan and run as its own program (tests/test_engine_plan.py's recipe).
SHAPES lists every engine shape and call size of tests/test_gpu_cem_gd3pg.py (that file builds its engines from these rows): the golden
cases, the ragged rows, FRL_RC=16 with FRL_CPS in {1, 2, 3}, the populations and the benchmark's shape."""
import os
import subprocess

import pytest

from tests import cem_gd3pg_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# FRL_RC=16: the seam between the two rings' halves at row 1, 5, 15, 17 and 35 (inside a 16-row chunk) and, at 32 rows, on a chunk boundary
RAGGED_ROWS = (2, 10, 30, 32, 34, 70)
RAGGED_DIMS = ((3, 1), (3, 4), (33, 16), (33, 4))
SPLIT_ROWS = (34, 70)                      # 3 and 5 chunks of 16 rows
POPULATIONS = (3, 40)


def shapes():
    """name -> (obs_dim, act_dim, hidden, n_learners, capacity, batch_max, FRL_RC, FRL_CPS, call sizes)"""
    out = {}
    for name in co.CASES:
        c = co.case(name)
        out["golden_" + name] = (c["obs_dim"], c["act_dim"], c["hidden"], 1, c["cap"], max(c["batch"], 2), 0, 0, (2 * (min(c["n1"], c["batch"]) // 2),))
    for O, A in RAGGED_DIMS:
        out["ragged_o%d_a%d" % (O, A)] = (O, A, 32, 1, 80, 70, 16, 0, RAGGED_ROWS)
    for cps in (1, 2, 3):
        # the plan takes FRL_CPS where it divides the chunks of batch_max rows: 96 rows = 6 chunks of 16 take all three
        out["split_cps%d" % cps] = (5, 2, 32, 1, 80, 96, 16, cps, SPLIT_ROWS)
    for P in POPULATIONS:
        out["population_%d" % P] = (4, 3, 32, P, 40, 16, 0, 0, (16, 10))
    out["bench_1"] = (24, 4, 128, 1, 4096, 256, 0, 0, (256,))
    out["bench_64"] = (24, 4, 128, 64, 4096, 256, 0, 0, (256,))
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cem_plan") / "cem_gd3pg_plan_probe"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cem_gd3pg_plan_probe.cpp"), "-o", str(exe)])
    return str(exe)


def test_every_offset_stays_inside_the_plans_buffers(probe, tmp_path):
    path = tmp_path / "shapes.txt"
    sh = shapes()
    path.write_text("".join("%s %s %s\n" % (name, " ".join(str(x) for x in s[:8]), " ".join(str(r) for r in s[8])) for name, s in sh.items()))
    r = subprocess.run([probe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = dict(l.split(": ", 1) for l in r.stdout.splitlines())
    assert set(out) == set(sh)
    for cps in (1, 2, 3):          # the knobs were taken: a workgroup walks 1, 2 and 3 chunks, over 6, 3 and 2 slabs
        assert out["split_cps%d" % cps].startswith("rc 16 cps %d S %d " % (cps, 6 // cps)), out["split_cps%d" % cps]
    print(r.stdout)


def test_a_violation_is_reported(probe, tmp_path):
    """the probe is not vacuous: a call larger than batch_max is named"""
    path = tmp_path / "bad.txt"
    path.write_text("bad 3 1 32 1 40 16 0 0 18\n")
    r = subprocess.run([probe, str(path)], capture_output=True, text=True)
    assert r.returncode == 1 and "batch_max" in r.stdout, r.stdout + r.stderr
