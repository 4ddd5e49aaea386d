"""Folding on Grumpkin without a GPU: the shape constructor over a curve's scalar field is declared, bound and exported; the kernels
over the BN254 base field are instantiated in translation units of their own, once per form, within the budgets their Bn254Fr twins
keep in tests/test_r1cs_row_resources.py; and fold.hip / r1cs_sat.hip still hold no kernel over that field."""
import os
import re
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import kernel_resources as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lurk_hip_r1cs_create_for_curve"
FQ = "7Bn254Fq"
NEW_UNITS = ("fold_bn254fq.hip", "r1cs_sat_bn254fq.hip")
OLD_UNITS = ("fold.hip", "r1cs_sat.hip")
THIRD_WAVE = 168  # registers of three waves per SIMD (tests/test_r1cs_row_resources.py)
# (unit, pattern of the mangled name after the field, instantiations, register bound or None, scratch bound or None): scratch 0
# wherever the Bn254Fr twin has scratch 0; the six-gather cross term's twin spills 240 bytes, the folds have no twin in that table
KERNELS = [
    ("fold_bn254fq.hip", r"r1cs_multiply_vec_kernelINS_%sELb0E", 1, None, 0),
    ("fold_bn254fq.hip", r"r1cs_multiply_vec_kernelINS_%sELb1E", 1, None, 0),
    ("fold_bn254fq.hip", r"r1cs_cross_term_kernelINS_%sE", 1, None, None),
    ("fold_bn254fq.hip", r"r1cs_cross_term_cached_kernelINS_%sE", 1, THIRD_WAVE, 0),
    ("fold_bn254fq.hip", r"fold_vec_kernelINS_%sE", 1, None, None),
    ("fold_bn254fq.hip", r"fold_vecs_kernelINS_%sE", 1, None, None),
    ("r1cs_sat_bn254fq.hip", r"r1cs_sat_kernelINS_%sELi(4|8|16)E", 3, THIRD_WAVE, 0),
    ("r1cs_sat_bn254fq.hip", r"r1cs_sat_lds_kernelINS_%sELi(4|8|16)E", 3, None, 0),
]


def test_the_constructor_is_declared_bound_and_exported():
    from lurk_beta_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lurk_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^;]*)\);" % NAME, header)
    assert m, "not declared in include/lurk_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14 and params[1] == "int curve"  # lurk_hip_r1cs_create's arguments with the curve in the field's place
    assert "#define LURK_HIP_ABI_VERSION 4" in header  # an addition under the unchanged revision
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == 14 and args == _lib.SIGNATURES["lurk_hip_r1cs_create"][1]
    rs = open(os.path.join(ROOT, "rust", "lurk-hip-sys", "src", "ffi.rs")).read()
    assert re.search(r"pub fn %s\(shape: \*mut \*mut lurk_hip_r1cs, curve: c_int, " % NAME, rs)
    assert NAME + "(" in open(os.path.join(ROOT, "rust", "lurk-hip-sys", "src", "lib.rs")).read()  # the wrapper beside R1csShape::new
    assert NAME + "(" in open(os.path.join(ROOT, "lurk_beta_amd", "host", "lurk_host.hpp")).read()
    lib = _lib.load()
    assert hasattr(lib, NAME) and lib.lurk_hip_abi_version() == 4
    from lurk_beta_amd import R1CSShape

    assert callable(R1CSShape.for_curve)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    d = str(tmp_path_factory.mktemp("grumpkin_fold_resources"))
    units = NEW_UNITS + OLD_UNITS
    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        return dict(zip(units, ex.map(lambda s: KR.usage(s, d), units)))


def test_fq_kernels_live_in_their_own_units_within_the_budgets(usage):
    seen = set()
    for unit, pattern, count, regs, scratch in KERNELS:
        hits = {k: v for k, v in usage[unit].items() if re.search(pattern % FQ, k)}
        assert len(hits) == count, (pattern % FQ, sorted(usage[unit]))
        for k, v in hits.items():
            print(k, v, "bounds", (regs, scratch))
            assert regs is None or v["vgprs"] + v["agprs"] <= regs, (k, v, regs)
            assert scratch is None or v["scratch"] <= scratch, (k, v, scratch)
            seen.add(k)
    # the new units hold kernels over the BN254 base field only, and none beyond the table
    for unit in NEW_UNITS:
        for k, v in usage[unit].items():
            if "vgprs" in v and re.search(r"_kernelINS_", k):
                assert k in seen, k
    # fold.hip and r1cs_sat.hip: no symbol over that field at all
    for unit in OLD_UNITS:
        assert usage[unit] and not [k for k in usage[unit] if FQ in k], unit
