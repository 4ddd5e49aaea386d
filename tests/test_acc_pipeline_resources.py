"""Register and scratch budget of the pipelined persistent accumulation, on the compiler's own resource remarks (as
tests/test_cabi_exports.py::test_sort_kernels_fit_beside_a_resident_accumulation reads them).

gfx950 allocates wave64 VGPRs in granules of 8 out of 512 per SIMD.  Two persistent launches are resident beside a 128-register tail
wave (finalize, the bit-plane levels): 128 + 2 x 192 = 512, so 192 is the most the persistent kernel may take - one granule more
and the second launch waits for the tail kernels.  The pipelined loop holds a table record in flight (16 registers) and must do
so without new scratch: the parent's kernels had 192 bytes per lane on the Pasta fields (the frame of the out-of-line doubling)
and none on the BN254 fields.  The persistent kernel has a second instantiation with the plain loop, for launches with two or more
waves per SIMD; it keeps the parent's footprint (176 / 178 registers: granule 184 at most).  The plain launch keeps the plain loop
and its three waves per SIMD (<= 168 registers)."""
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import kernel_resources as KR

UNITS = ("msm_acc_persistent.hip", "msm_acc_persistent_bn254.hip", "msm_acc.hip")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = str(tmp_path_factory.mktemp("acc_pipeline_resources"))
    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        return dict(zip(UNITS, ex.map(lambda s: KR.usage(s, d), UNITS)))


def _granule(v):
    return -(-v // 8) * 8


def test_persistent_kernels_keep_the_192_register_budget_without_new_scratch(usage):
    seen = []
    for unit, parent_scratch in (("msm_acc_persistent.hip", 192), ("msm_acc_persistent_bn254.hip", 0)):
        kernels = {k: v for k, v in usage[unit].items() if "msm_accumulate_persistent_kernel" in k}
        assert len(kernels) == 4, (unit, sorted(usage[unit]))   # two fields x (pipelined, plain loop)
        for k, v in kernels.items():
            print(unit, k, v)
            assert _granule(v["vgprs"] + v["agprs"]) <= 192, (k, v)
            assert v["scratch"] <= 192, (k, v)                 # the bound every instantiation is held to
            assert v["scratch"] <= parent_scratch, (k, v)      # and none more than its parent had
            if "ELb0E" in k:                                   # the plain loop of the launches with two or more waves per SIMD: the parent's footprint
                assert _granule(v["vgprs"] + v["agprs"]) <= 184, (k, v)
            seen.append(k)
    for field in ("PallasFp", "PallasFq", "Bn254Fq", "Bn254Fr"):   # <field, true> is the pipelined instantiation, <field, false> the plain loop
        assert sum(field + "ELb1E" in k for k in seen) == 1 and sum(field + "ELb0E" in k for k in seen) == 1, (field, seen)


def test_plain_accumulate_kernels_stay_at_three_waves_per_simd(usage):
    kernels = {k: v for k, v in usage["msm_acc.hip"].items() if "msm_accumulate_kernel" in k}
    assert len(kernels) == 2, sorted(usage["msm_acc.hip"])
    for k, v in kernels.items():
        print(k, v)
        assert _granule(v["vgprs"] + v["agprs"]) <= 168, (k, v)
        assert v["scratch"] <= 192, (k, v)
