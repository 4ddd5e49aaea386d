"""Task sums and buckets as radix-2^29 records against the 8 x 32 round trip they replace, on the host under AddressSanitizer and
UBSan: tests/host_bucket_records/main.cpp is a stand-alone program (its own main), built here with g++ and run as a child.  It exits
non-zero when a bucket or a first-level merge differs between the two paths (0 / 1 / 2 / many tasks per bucket, identity task sums,
doublings), when a stored record is not R-bounded (plane_store asserts it under LURK_F29_CHECK) or when a store or load leaves the
record array, which is allocated to the exact size (the sanitizer ends the program).  The sanitizer runtimes are linked into the
program, so it needs nothing from the environment it is started in."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_records_equal_the_8x32_round_trip_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "bucket_records_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DLURK_F29_CHECK=1", os.path.join(ROOT, "tests", "host_bucket_records", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "records == 8 x 32 round trip" in r.stdout and " 12 cases" in r.stdout, r.stdout[-500:]
