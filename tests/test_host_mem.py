"""csrc/host_mem.hpp — the owner of every device and pinned allocation of an engine and of an env pool — on the CPU: the
header is plain C++17 over a backend, so tests/host_mem_probe.cpp instantiates it with a counting malloc / free fake that can
fail the k-th allocation, and runs under AddressSanitizer + UBSan as a stand-alone program.  The probe pins what no GPU test can
see: every block freed exactly once through the matching free, newest first; grow()'s capacity after a failed allocation; a routine
that fails half-way leaving nothing behind."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_probe_under_sanitizers(tmp_path):
    exe = tmp_path / "host_mem_probe"
    # (the sanitizer runtimes linked statically: the probe does not depend on what else the process's library list holds)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "freerl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_mem_probe.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "host_mem ok"

