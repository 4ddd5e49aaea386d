"""CPU-only: the plan of a batch of short commitments (lurk_beta_amd/csrc/msm_batch_plan.hpp) and the split of the signed window digits,
by a stand-alone program (tests/host_msm_batch/main.cpp, its own main) built on the host with AddressSanitizer and UBSan.  Nothing is
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_msm_batch", "main.cpp")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("host_msm_batch") / "main")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_header_exists_and_is_plain_cxx():
    """the plan header compiles without HIP: no hip include, no device qualifier outside the guarded macro"""
    text = open(os.path.join(ROOT, "lurk_beta_amd", "csrc", "msm_batch_plan.hpp")).read()
    assert "hip_runtime" not in text and "__global__" not in text
    assert "LURK_MSM_BATCH_MAX_VECTORS" in open(os.path.join(ROOT, "include", "lurk_hip.h")).read()


def test_split_segments_and_refusals_under_the_sanitizers(program):
    """for every c in 16..20 and the digit magnitudes 1, 2^h - 1, 2^h, 2^h + 1, 2^(c-1): lo + 2^h hi == |d|, both halves within B, the key
    of (vector, piece, value) unique and below NB; the segment lookup at the first and last element of every vector (empty vectors between
    non-empty ones); the plan's refusals (count 0 / 65, a length of 2^16 + 1, a total of 2^20 + 1)"""
    r = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 1000, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
