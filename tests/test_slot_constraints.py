"""CPU-only: the slot gadgets' constraint rows the library emits (lurk_hip_slot_constraints, built from the product's own Poseidon
constants in csrc/slot_circuit.hpp) against the rows oracle/circuit_ref.py records for the same gadgets; the sizes call; refusals; and
that the satisfiability kernels compile without scratch."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import circuit_ref as CR
from oracle import coracle as C
from oracle import pyref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ((3, "commitment"), (4, "hash4"), (6, "hash6"), (8, "hash8"), (1, "bit_decomp"))
# rows, nnz A / B / C, longest row, distinct coefficients - pinned from the oracle's run (the same on the three fields for the hash slots)
HASH_PINS = {3: (265, 2287, 4303, 349, 60, 326), 4: (289, 2481, 4665, 380, 61, 396), 6: (337, 2911, 5473, 442, 63, 539), 8: (388, 3473, 6542, 508, 66, 696)}
BIT_PINS = {1: (298, 1019, 298, 43, 255, 256), 0: (301, 1019, 301, 46, 255, None), 2: (354, 1015, 354, 100, 254, None)}  # Pallas Fq / Fp / BN254


def _sizes(lib, f, st):
    v = [ctypes.c_size_t() for _ in range(4)]
    assert lib.lurk_hip_slot_constraints_size(f, st, *[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


@pytest.mark.parametrize("f", [0, 1, 2])
@pytest.mark.parametrize("st,name", SLOTS)
def test_rows_equal_the_oracles(f, st, name):
    from lurk_beta_amd import _lib, slot_constraints, slot_witness_size

    lib = _lib.load()
    p = R.modulus(f)
    mats = slot_constraints(f, st)
    n, *nnz = _sizes(lib, f, st)
    size = slot_witness_size(f, st)
    cs = CR.slot_witness(f, name, [R.uniform_fe(60, i, p) for i in range(1 if st == 1 else st)])[1]
    assert cs.unsatisfied() == [] and len(cs.aux) == size
    assert n == len(cs.constraints)
    coeffs, longest = set(), 0
    for w, (indptr, indices, data) in enumerate(mats):
        assert len(indptr) == n + 1 and int(indptr[0]) == 0 and int(indptr[-1]) == len(indices) == nnz[w] and data.shape == (nnz[w], 4)
        vals = C.limbs_to_ints(C.from_mont(f, data)) if nnz[w] else []
        assert all(0 < v < p for v in vals)  # no zero data, canonical
        coeffs |= set(vals)
        for r in range(n):
            lo, hi = int(indptr[r]), int(indptr[r + 1])
            cols = [int(c) for c in indices[lo:hi]]
            assert cols == sorted(set(cols)) and all(c <= size for c in cols)
            longest = max(longest, hi - lo)
            want = {(size if k == 0 else k - 1): v % p for k, v in cs.constraints[r][w].items() if v % p}
            assert dict(zip(cols, vals[lo:hi])) == want, (f, name, "ABC"[w], r)
    pins = HASH_PINS[st] if st != 1 else BIT_PINS[f]
    assert (n, *nnz, longest) == pins[:5]
    if pins[5] is not None and (st == 1 or f == 1):
        assert len(coeffs) == pins[5]


def test_one_frame_of_the_step_on_pallas_fq():
    from lurk_beta_amd import _lib

    lib = _lib.load()
    counts = {4: 14, 8: 6, 3: 1, 1: 3}
    rows = sum(c * _sizes(lib, 1, st)[0] for st, c in counts.items())
    nnz = sum(c * sum(_sizes(lib, 1, st)[1:]) for st, c in counts.items())
    assert (rows, nnz) == (7533, 179521)


def test_refusals():
    from lurk_beta_amd import LurkHipError, _lib, slot_constraints

    lib = _lib.load()
    v = [ctypes.c_size_t() for _ in range(4)]
    refs = [ctypes.byref(x) for x in v]
    for f, st in ((3, 4), (-1, 4), (1, 5), (1, 0), (1, 2)):
        assert lib.lurk_hip_slot_constraints_size(f, st, *refs) != 0
        assert b"unknown" in lib.lurk_hip_last_error()
        with pytest.raises(LurkHipError):
            slot_constraints(f, st)
    for k in range(4):
        args = list(refs)
        args[k] = None
        assert lib.lurk_hip_slot_constraints_size(1, 4, *args) != 0 and b"null" in lib.lurk_hip_last_error()
    n, na, nb, nc = _sizes(lib, 1, 4)
    bufs = [np.zeros(n + 1, np.uint64), np.zeros(na, np.uint64), np.zeros((na, 4), np.uint64), np.zeros(n + 1, np.uint64), np.zeros(nb, np.uint64),
            np.zeros((nb, 4), np.uint64), np.zeros(n + 1, np.uint64), np.zeros(nc, np.uint64), np.zeros((nc, 4), np.uint64)]
    for k in range(9):
        args = [_lib.ptr(b) for b in bufs]
        args[k] = None
        assert lib.lurk_hip_slot_constraints(1, 4, *args) != 0 and b"null" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_slot_constraints(1, 4, *[_lib.ptr(b) for b in bufs]) == 0 and lib.lurk_hip_last_error() == b""


def test_satisfiability_kernels_use_no_scratch(tmp_path):
    import shutil
    import subprocess

    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "lurk_beta_amd", "csrc")
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-variable",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "r1cs_sat.hip", "-o", str(tmp_path / "r1cs_sat.o")], cwd=csrc, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) >= 3 and any("r1cs_sat_kernel" in n for n in names)
    assert all(s == 0 for s in scratch), dict(zip(names, scratch))
