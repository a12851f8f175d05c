"""
The owners of device and pinned host memory (directdemod_amd/csrc/dd_devbuf.h) on the host alone: tests/host/devbuf_check.cpp
defines hipMalloc / hipFree / hipHostMalloc / hipHostFree itself, over malloc, with a set of live pointers (a free of a pointer
that is not live aborts) and a k-th allocation that fails.  It is compiled with ROCm's clang++ against the HIP headers, without
the HIP runtime, and run: every assertion is in the program, which exits 0 and prints one line when all of them hold.

Built here without sanitizer flags; the same program under AddressSanitizer and UBSan: tools/README.md.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "devbuf_check.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _clangxx():
    for c in (os.path.join(ROCM, "llvm", "bin", "clang++"), os.path.join(ROCM, "bin", "amdclang++")):
        if os.path.exists(c):
            return c
    return shutil.which("clang++")


def test_devbuf_owners_on_the_host(tmp_path):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not found")
    exe = str(tmp_path / "devbuf_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "compile failed:\n%s\n%s" % (r.stdout, r.stderr)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, "devbuf_check failed (%d):\n%s\n%s" % (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith("devbuf_check: ok"), r.stdout


def test_devbuf_header_stands_alone():
    """the header includes the HIP API header and nothing of the project's, and stays small"""
    src = open(os.path.join(ROOT, "directdemod_amd", "csrc", "dd_devbuf.h")).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert "<hip/hip_runtime_api.h>" in incs
    assert not [i for i in incs if i.startswith('"')], incs
    assert len(src.splitlines()) <= 80
