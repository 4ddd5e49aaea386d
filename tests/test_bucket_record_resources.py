"""Register and scratch budgets of the kernels that keep task sums and buckets on the radix-2^29 layer, on the compiler's own resource
remarks of a gfx950 cross-compile (as tests/test_acc_pipeline_resources.py reads them).

gfx950 allocates wave64 VGPRs in granules of 8 out of 512 per SIMD.  A tail wave (finalize, the hot-bucket kernel, the bit-plane levels)
has to fit beside TWO resident one-wave accumulations of 192 registers: 128 + 2 x 192 = 512.  The hot-bucket kernel is launched for every
commitment, with an empty list under uniform scalars; in its 8 x 32 form it took 133 registers (granule 136) and that empty launch
waited for an accumulation to end.  The accumulate kernels store a record instead of converting their sum: their budgets are the
parent's (192 pipelined, 184 for the persistent plain loop, three waves per SIMD for the plain launch) and their scratch may not grow
(parent: 192 bytes per lane on the Pasta fields - the frame of the out-of-line doubling - and none on the BN254 fields)."""
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import kernel_resources as KR

UNITS = ("msm_finalize.hip", "msm_acc_persistent.hip", "msm_acc_persistent_bn254.hip", "msm_acc.hip", "msm_acc_bn254.hip")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = str(tmp_path_factory.mktemp("bucket_record_resources"))
    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        return dict(zip(UNITS, ex.map(lambda s: KR.usage(s, d), UNITS)))


def _granule(v):
    return -(-(v["vgprs"] + v["agprs"]) // 8) * 8


def test_finalize_and_hot_bucket_kernels_fit_beside_two_accumulations_on_the_pasta_fields(usage):
    for needle in ("msm_finalize_kernel", "msm_big_bucket_kernel"):
        kernels = {k: v for k, v in usage["msm_finalize.hip"].items() if needle in k}
        assert len(kernels) == 2, (needle, sorted(usage["msm_finalize.hip"]))   # PallasFp, PallasFq
        for k, v in kernels.items():
            print(k, v)
            assert _granule(v) <= 128, (k, v)
            assert _granule(v) + 2 * 192 <= 512, (k, v)


def test_accumulate_kernels_keep_their_budgets_and_the_parents_scratch(usage):
    for unit, parent_scratch in (("msm_acc_persistent.hip", 192), ("msm_acc_persistent_bn254.hip", 0)):
        kernels = {k: v for k, v in usage[unit].items() if "msm_accumulate_persistent_kernel" in k}
        assert len(kernels) == 4, (unit, sorted(usage[unit]))   # two fields x (pipelined, plain loop)
        for k, v in kernels.items():
            print(unit, k, v)
            assert _granule(v) <= (192 if "ELb1E" in k else 176), (k, v)   # <P, true>: the pipelined loop; <P, false>: the plain loop
            assert v["scratch"] <= parent_scratch, (k, v)
    for unit, parent_scratch in (("msm_acc.hip", 192), ("msm_acc_bn254.hip", 0)):
        kernels = {k: v for k, v in usage[unit].items() if "msm_accumulate_kernel" in k}
        assert len(kernels) == 2, (unit, sorted(usage[unit]))
        for k, v in kernels.items():
            print(unit, k, v)
            assert _granule(v) <= 168, (k, v)                 # three waves per SIMD
            assert v["scratch"] <= parent_scratch, (k, v)
