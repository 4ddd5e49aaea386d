"""Register and scratch budgets of every kernel that calls the shared row product (r1cs_shape.cuh: r1cs_row) and the shared row
classes, on the compiler's own resource remarks of a gfx950 cross-compile.

The budgets are what the kernels took while each file carried its own copy of the row loop (fold_row_lane / fold_row_wave, sat_row,
mle_row; VGPRs + AGPRs, scratch bytes per lane, -O3): sharing the code has no reason to spend registers.  Two of them are occupancy
bounds as well - the cached cross term and the satisfiability kernel stay within 168 registers, their third wave per SIMD."""
import re
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import kernel_resources as KR

UNITS = ("fold.hip", "r1cs_sat.hip", "verify.hip")
PASTA, BN = ("8PallasFp", "8PallasFq"), ("7Bn254Fr",)
# (unit, pattern of the mangled name after the field, instantiations per field): {fields: (registers, scratch)}
BUDGETS = [
    ("fold.hip", r"r1cs_multiply_vec_kernelINS_%sELb0E", 1, {PASTA: (104, 0), BN: (103, 0)}),
    ("fold.hip", r"r1cs_multiply_vec_kernelINS_%sELb1E", 1, {PASTA: (100, 0), BN: (92, 0)}),
    ("fold.hip", r"r1cs_cross_term_kernelINS_%sE", 1, {PASTA: (172, 240), BN: (139, 240)}),
    ("fold.hip", r"r1cs_cross_term_cached_kernelINS_%sE", 1, {PASTA: (144, 0), BN: (148, 0)}),
    ("r1cs_sat.hip", r"r1cs_sat_kernelINS_%sELi(4|8|16)E", 3, {PASTA: (168, 0), BN: (165, 0)}),
    ("r1cs_sat.hip", r"r1cs_sat_lds_kernelINS_%sELi(4|8)E", 2, {PASTA: (189, 0), BN: (199, 0)}),
    ("r1cs_sat.hip", r"r1cs_sat_lds_kernelINS_%sELi16E", 1, {PASTA: (188, 0), BN: (198, 0)}),
    ("verify.hip", r"sparse_mle_kernelINS_%sE", 1, {PASTA: (124, 0), BN: (122, 0)}),
]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = str(tmp_path_factory.mktemp("r1cs_row_resources"))
    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        return dict(zip(UNITS, ex.map(lambda s: KR.usage(s, d), UNITS)))


def test_row_kernels_keep_their_registers_and_scratch(usage):
    seen = {}
    for unit, pattern, per_field, budgets in BUDGETS:
        for fields, (regs, scratch) in budgets.items():
            for field in fields:
                hits = {k: v for k, v in usage[unit].items() if re.search(pattern % field, k)}
                assert len(hits) == per_field, (pattern % field, sorted(usage[unit]))
                for k, v in hits.items():
                    print(k, v, "budget", (regs, scratch))
                    assert v["vgprs"] + v["agprs"] <= regs and v["scratch"] <= scratch, (k, v, regs, scratch)
                    assert k not in seen
                    seen[k] = re.sub(r"INS_.*", "", re.sub(r"^_ZN4lurk\d+", "", k))
    count = lambda name: sum(1 for n in seen.values() if n == name)
    # three fields x (lane, long) of multiply_vec, the two cross terms, three group widths of the two sat kernels, sparse_mle
    assert (count("r1cs_multiply_vec_kernel"), count("r1cs_cross_term_kernel"), count("r1cs_cross_term_cached_kernel"), count("r1cs_sat_kernel"),
            count("r1cs_sat_lds_kernel"), count("sparse_mle_kernel")) == (6, 3, 3, 9, 9, 3)
    # and nothing of these kernels escaped the table
    for unit in UNITS:
        for k in usage[unit]:
            if re.search(r"r1cs_multiply_vec_kernel|r1cs_cross_term|r1cs_sat_(lds_)?kernel|sparse_mle_kernel", k):
                assert k in seen, k
