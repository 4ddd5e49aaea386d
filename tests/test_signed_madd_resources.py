"""Register, scratch and instruction budgets of the accumulate kernels with the mixed addition on signed limbs (curve29.cuh:
xyzz29_madd_s), on the compiler's own resource remarks and on the gfx950 listing.

The signed form must not cost occupancy: the persistent pipelined kernel stays within 192 VGPRs (two launches beside a
128-register tail wave), the persistent kernel's plain loop within 176, the plain launch within 168 (three waves per SIMD), and
scratch stays at the 192 bytes per lane of the out-of-line doubling's frame.

Instructions: bench_tools/issue_model.py on the steady task loop of the persistent pipelined kernel (the shortest loop with at
least 1 000 64-bit mads: one general mixed addition per trip).  The group law's own multiplies are 6 x 126 + 2 x 90 + 207 (the Y3
row) = 1 143; the parent's loop issued 1 154, the 11 others being the two f29_reduce (5 each) and one quotient estimate.  The signed
loop has no f29_reduce, so its count may only be lower: it is held to [1 143, 1 154].  The parent's loop, counted the same way, is
2 166 VALU instructions and 8 448 issue cycles per trip (profiles/r15_signed_madd_issue_model.txt); the signed loop must be
below both by at least what the construction removes for certain: four carry passes of 8 x (add, and, shift) = 96 instructions (the
floor asked here is 80 instructions and 250 issue cycles; the listing gives 109 and 332)."""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import kernel_resources as KR

ROOT, CSRC, FLAGS = KR.ROOT, KR.CSRC, KR.FLAGS
PARENT_VALU, PARENT_CYCLES = 2166, 8448


def _listing(src, out_dir):
    path = os.path.join(out_dir, src + ".s")
    r = subprocess.run(["hipcc", *FLAGS, "-S", "--cuda-device-only", src, "-o", path], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    return path


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = str(tmp_path_factory.mktemp("signed_madd_resources"))
    with ThreadPoolExecutor(max_workers=3) as ex:
        a = ex.submit(KR.usage, "msm_acc_persistent.hip", d)
        b = ex.submit(KR.usage, "msm_acc.hip", d)
        c = ex.submit(_listing, "msm_acc_persistent.hip", d)
        return {"persistent": a.result(), "plain": b.result(), "listing": c.result()}


def test_register_and_scratch_budgets_hold(built):
    seen = 0
    for k, v in built["persistent"].items():
        if "msm_accumulate_persistent_kernel" not in k or "Pallas" not in k:
            continue
        print(k, v)
        seen += 1
        assert v["vgprs"] + v["agprs"] <= (192 if "ELb1E" in k else 176), (k, v)   # <field, true>: the pipelined loop; <field, false>: the plain loop
        assert v["scratch"] <= 192, (k, v)
    assert seen == 4                                                                # two Pasta fields x two loops
    plain = {k: v for k, v in built["plain"].items() if "msm_accumulate_kernel" in k and "Pallas" in k}
    assert len(plain) == 2, sorted(built["plain"])
    for k, v in plain.items():
        print(k, v)
        assert v["vgprs"] + v["agprs"] <= 168 and v["scratch"] <= 192, (k, v)


@pytest.mark.parametrize("field", ["8PallasFp", "8PallasFq"])
def test_steady_loop_keeps_the_mad_count_and_issues_fewer_instructions(built, field):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tools", "issue_model.py"), built["listing"], "msm_accumulate_persistent_kernelINS_" + field + "ELb1E", "1",
                        "mads>=1000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    print(r.stdout)
    valu = int(re.search(r"(\d+) VALU instructions per trip", r.stdout).group(1))
    mads = int(re.search(r"mad64\s+(\d+) x", r.stdout).group(1))
    cycles = int(re.search(r"issue cycles per wave-trip: (\d+)", r.stdout).group(1))
    signed = int(re.search(r"v_mad_i64_i32 (\d+)", r.stdout).group(1))
    assert 1143 <= mads <= 1154, r.stdout
    assert signed == 6 * 81 + 2 * 45 + 162, r.stdout          # every operand-by-operand product of the group law is a signed mad
    assert valu <= PARENT_VALU - 80 and cycles <= PARENT_CYCLES - 250, (valu, cycles)
