"""The pipelined task loop of the persistent bucket accumulation against the plain loop, on the host under AddressSanitizer and
UBSan: tests/host_acc_pipeline/main.cpp is a stand-alone program (its own main), built here with g++ and run as a child.  It exits
non-zero when the two loops differ in a single limb or flag, when a bound assertion of the radix-2^29 layer fires, or when the
look-ahead reads one word past the index list or one record past the table (the sanitizer ends the program).  The sanitizer
runtimes are linked into the program, so it needs nothing from the environment it is started in."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pipelined_loop_equals_the_plain_loop_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "acc_pipeline_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DLURK_F29_CHECK=1", os.path.join(ROOT, "tests", "host_acc_pipeline", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "pipelined == plain" in r.stdout and " 160 cases" in r.stdout, r.stdout[-500:]
