"""The mixed addition on signed limbs against the unsigned one, on the host under AddressSanitizer and UBSan:
tests/host_signed_madd/main.cpp is a stand-alone program (its own main), built here with g++ and run as a child.  It exits non-zero
when a signed sum differs from the unsigned one as an affine point, when a bound assertion of the signed contract fires on an operand
inside the contract, or when the end-of-task normalisation leaves a record plane_store does not accept.  Run as `trip <name>` it puts
ONE operand a single step past a stated extreme and must be stopped by the assertion."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import coracle as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIPS = ["limb_above", "limb_below", "top_above", "top_below", "row_limb", "acc_above", "acc_below", "acc_limb", "norm_above"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("signed_madd") / "signed_madd_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-DLURK_F29_CHECK=1", os.path.join(ROOT, "tests", "host_signed_madd", "main.cpp"), "-o", out], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


def test_signed_madd_equals_the_unsigned_one_under_sanitizers(exe, tmp_path):
    pts = tmp_path / "points.txt"
    with open(pts, "w") as f:
        for c in (0, 1):  # points 640..703 of each synthetic key, as the 16 32-bit words of their table records
            for rec in np.ascontiguousarray(C.synth_bases(c, 704)[640:]).view(np.uint32).reshape(64, 16):
                f.write("%d %s\n" % (c, " ".join("%x" % w for w in rec)))
    r = subprocess.run([exe, str(pts)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "signed == unsigned as affine points" in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("name", TRIPS)
def test_one_past_each_extreme_trips_the_assertion(exe, name):
    r = subprocess.run([exe, "trip", name], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "F29 bound violated" in r.stdout and "passed every assertion" not in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-500:])
