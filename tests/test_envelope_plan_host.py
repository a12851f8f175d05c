"""
The plan of the Hilbert envelope's block walk (envelope_plan, directdemod_amd/csrc/dd_audio_envelope.h) on the host alone:
tests/host/envelope_plan_check.cpp includes the header's plan section (pure host code under DD_ENVELOPE_PLAN_ONLY), is compiled
with ROCm's clang++ without HIP, and run: every assertion is in the program, which exits 0 and prints one line when all of them
hold.  Once as the library runs by default and once under DD_AM_HILBERT=lib.

Built here without sanitizer flags; the same program under AddressSanitizer and UBSan: tools/README.md.
"""
import os
import subprocess

import pytest

from test_devbuf_host import ROOT, _clangxx

SRC = os.path.join(ROOT, "tests", "host", "envelope_plan_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = _clangxx()
    if cxx is None:
        pytest.skip("clang++ not found")
    out = str(tmp_path_factory.mktemp("envelope_plan") / "envelope_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, "compile failed:\n%s\n%s" % (r.stdout, r.stderr)
    return out


@pytest.mark.parametrize("mode", ["own", "lib"])
def test_envelope_plan_on_the_host(exe, mode):
    env = {k: v for k, v in os.environ.items() if k != "DD_AM_HILBERT"}
    if mode == "lib":
        env["DD_AM_HILBERT"] = "lib"
    r = subprocess.run([exe] + (["lib"] if mode == "lib" else []), capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, "envelope_plan_check failed (%d):\n%s\n%s" % (r.returncode, r.stdout, r.stderr)
    assert r.stdout.startswith("envelope_plan_check: ok"), r.stdout
