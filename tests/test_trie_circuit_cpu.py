"""CPU-only: the rows of the trie coprocessor's step circuits the library emits (lurk_hip_trie_circuit_constraints, csrc/trie_circuit.hpp)
against the Python restatement of Trie::synthesize_lookup / synthesize_insert (tests/trie_circuit_ref.py), entry for entry; the sizes
call against the closed forms; the structure at H = 85, where the restatement is too slow to run whole; refusals; the ABI and mirror
bookkeeping; and the new kernels' registers and scratch against the existing trace kernels'."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import trie_circuit_ref as TC
from tests import trie_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lurk_hip_trie_circuit_size", "lurk_hip_trie_circuit_constraints", "lurk_hip_trie_circuit_r1cs_create", "lurk_hip_trie_circuit_witness_dev")


def _library_rows(f, mats):
    """per row three lists of (column, canonical coefficient), as tests.trie_circuit_ref.rows gives them"""
    per = []
    for indptr, indices, data in mats:
        vals = C.limbs_to_ints(C.from_mont(f, data)) if len(indices) else []
        per.append([list(zip((int(c) for c in indices[int(indptr[r]):int(indptr[r + 1])]), vals[int(indptr[r]):int(indptr[r + 1])])) for r in range(len(indptr) - 1)])
    return [tuple(per[w][r] for w in range(3)) for r in range(len(per[0]))]


def _proof(f, height, seed):
    """a small populated trie, a key and a value -> (root, key, old path, new value, new root)"""
    p = R.modulus(f)
    trie = T.RefTrie(f, height)
    for i in range(5):
        trie.insert(R.uniform_fe(70 + seed, i, p), R.uniform_fe(71 + seed, i, p))
    key = R.uniform_fe(70 + seed, 2 if seed % 2 else 9, p)  # present / absent
    root = trie.root
    value = R.uniform_fe(72, seed, p)
    old, new, _ = trie.copy().prove_insert(key, value)
    t2 = trie.copy()
    t2.insert(key, value)
    return root, key, old, value, t2.root


@pytest.mark.parametrize("op", [TC.LOOKUP, TC.INSERT])
@pytest.mark.parametrize("height", [1, 2, 3])
@pytest.mark.parametrize("f", [0, 1, 2])
def test_rows_sizes_and_columns_equal_the_restatement(f, height, op):
    from lurk_beta_amd.trie_circuit import trie_circuit_constraints, trie_circuit_size

    root, key, old, value, new_root = _proof(f, height, 3 * f + height)
    cs, result, value_var = TC.trie_circuit(f, height, op, root, key, old, value)
    assert cs.unsatisfied() == []  # the restatement accepts the reference trie's proof
    if op == TC.INSERT:
        assert cs.aux[result - 1] == new_root  # the insert's last digest is the directly computed new root
    else:
        assert cs.aux[result - 1] == old[-1][T.path(f, key, height)[-1]]
    sz = trie_circuit_size(f, height, op)
    want = TC.rows(cs)
    assert (sz.size, sz.num_cons, sz.result_col, sz.value_col) == (len(cs.aux), len(want), result - 1, None if value_var is None else value_var - 1)
    assert (sz.size, sz.num_cons, sz.result_col, sz.value_col) == TC.closed_forms(f, height, op)
    mats = trie_circuit_constraints(f, height, op)
    assert [len(m[1]) for m in mats] == [sz.nnz_a, sz.nnz_b, sz.nnz_c] == [sum(len(r[w]) for r in want) for w in range(3)]
    got = _library_rows(f, mats)
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f, height, op, r)


def test_the_issues_counts_at_height_3_on_bn254():
    from lurk_beta_amd.trie_circuit import trie_circuit_size

    lk, ins = trie_circuit_size(2, 3, TC.LOOKUP), trie_circuit_size(2, 3, TC.INSERT)
    assert (lk.size, lk.num_cons, ins.size, ins.num_cons) == (1564, 1542, 2753, 2706)


@pytest.mark.parametrize("f", [0, 1, 2])
def test_height_85_closed_forms_level_shift_and_constant_false_picks(f):
    from lurk_beta_amd.trie_circuit import trie_circuit_constraints, trie_circuit_size

    H = 85
    b = TC.key_block_size(f)
    for op in (TC.LOOKUP, TC.INSERT):
        sz = trie_circuit_size(f, H, op)
        assert (sz.size, sz.num_cons, sz.result_col, sz.value_col) == TC.closed_forms(f, H, op)
    if f == 2:
        assert (trie_circuit_size(f, H, TC.LOOKUP).size, trie_circuit_size(f, H, TC.LOOKUP).num_cons) == (34610, 34014)
        # nnz C is 1 530 below the 89 265 counted from the restatement's dictionaries: those hold a zero coefficient for ONE in the nine
        # S-boxes of a hash's last round, which has no key (oracle/circuit_ref.py's sbox) - 9 per hash, 170 hashes - and rows carry none
        assert (sz.size, sz.num_cons, sz.nnz_a, sz.nnz_b, sz.nnz_c) == (68271, 66994, 592700, 1113170, 89265 - 9 * 2 * H)
    A, B, Cm = trie_circuit_constraints(f, H, TC.INSERT)
    assert max(int(x) for x in np.diff(A[0])) == (254 if f == 2 else 255)  # the longest row: the unpacking row of the key's bits
    size = sz.size
    sz_l = trie_circuit_size(f, H, TC.LOOKUP)
    # the lookup's rows open the insert's, with ONE moved from the lookup's size to the insert's
    for (ip, ix, dv), (lp, lx, lv) in zip((A, B, Cm), trie_circuit_constraints(f, H, TC.LOOKUP)):
        n = len(lx)
        assert np.array_equal(ip[:sz_l.num_cons + 1], lp) and np.array_equal(dv[:n], lv)
        assert np.array_equal(np.where(lx == sz_l.size, size, lx), ix[:n])

    def level_rows(m, i):
        ip, ix, dv = m
        r0 = b + 396 * i
        lo, hi = int(ip[r0]), int(ip[r0 + 396])
        return (ip[r0:r0 + 397] - ip[r0]).copy(), ix[lo:hi].astype(np.int64), dv[lo:hi]

    # level i's rows are level 0's shifted by 403 i columns, apart from `next` (C of row 388) and the condition columns (B of rows 389 .. 395)
    base = [level_rows(m, 0) for m in (A, B, Cm)]
    empty_b = []
    for i in range(H):
        for w, m in enumerate((A, B, Cm)):
            ip, ix, dv = level_rows(m, i)
            ip0, ix0, dv0 = base[w]
            if w == 1:  # B: the seven pick rows hold the condition (or nothing)
                cond = [int(ip[389 + k + 1] - ip[389 + k]) for k in range(7)]
                empty_b += [(i, k) for k in range(7) if cond[k] == 0]
                keep, keep0 = int(ip[389]), int(ip0[389])
                assert keep == keep0 and np.array_equal(ip[:390], ip0[:390])
                ix, dv, ix0, dv0 = ix[:keep], dv[:keep], ix0[:keep0], dv0[:keep0]
            elif w == 2:  # C: row 388 is `next`
                assert np.array_equal(ip, ip0)
                at = int(ip[388])
                assert int(ip[389]) - at == 1 and int(ix[at]) == (0 if i == 0 else 1 + b + 403 * (i - 1) + 402)
                ix, dv, ix0, dv0 = np.delete(ix, at), np.delete(dv, at, axis=0), np.delete(ix0, at), np.delete(dv0, at, axis=0)
            else:
                assert np.array_equal(ip, ip0)
            assert np.array_equal(dv, dv0), (i, w)
            assert np.array_equal(np.where(ix == size, size, ix - 403 * i), ix0), (i, w)
    # Boolean::Constant(false): bit 254 on BN254 only - the four round-0 picks of level 0
    assert empty_b == ([(0, 0), (0, 1), (0, 2), (0, 3)] if f == 2 else [])
    # the condition of pick round r of level i is key bit 3 (H - 1 - i) + 2 - r: the unpacking row lists the bits from the top down
    ipa, ixa, _ = A
    bits_be = ixa[int(ipa[b - 1]):int(ipa[b])]
    ipb, ixb, _ = B
    for i in (0, 1, 41, 84):
        for k, r in enumerate((0, 0, 0, 0, 1, 1, 2)):
            bit = 3 * (H - 1 - i) + 2 - r
            row = b + 396 * i + 389 + k
            if bit < len(bits_be):
                assert [int(x) for x in ixb[int(ipb[row]):int(ipb[row + 1])]] == [int(bits_be[len(bits_be) - 1 - bit])]


def test_refusals():
    from lurk_beta_amd import LurkHipError, _lib
    from lurk_beta_amd.trie_circuit import trie_circuit_constraints, trie_circuit_size

    lib = _lib.load()
    v = [ctypes.c_size_t() for _ in range(7)]
    refs = [ctypes.byref(x) for x in v]
    for f, h, op, word in ((3, 3, 0, b"field"), (-1, 3, 0, b"field"), (1, 0, 0, b"height"), (1, 86, 1, b"height"), (1, 3, 2, b"circuit"), (1, 3, -1, b"circuit")):
        assert lib.lurk_hip_trie_circuit_size(f, h, op, *refs) != 0 and word in lib.lurk_hip_last_error()
        with pytest.raises(LurkHipError):
            trie_circuit_constraints(f, h, op)
    for k in range(6):
        args = list(refs)
        args[k] = None
        assert lib.lurk_hip_trie_circuit_size(1, 2, 1, *args) != 0 and b"null" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_trie_circuit_size(1, 2, 0, *refs[:6], None) == 0  # value_col may be NULL for a lookup
    sz = trie_circuit_size(1, 1, 0)
    n = sz.num_cons
    bufs = [b for nz in (sz.nnz_a, sz.nnz_b, sz.nnz_c) for b in (np.zeros(n + 1, np.uint64), np.zeros(nz, np.uint64), np.zeros((nz, 4), np.uint64))]
    for k in range(9):
        args = [_lib.ptr(x) for x in bufs]
        args[k] = None
        assert lib.lurk_hip_trie_circuit_constraints(1, 1, 0, *args) != 0 and b"null" in lib.lurk_hip_last_error()
    # all null, all zero
    assert lib.lurk_hip_trie_circuit_size(0, 0, 0, *[None] * 7) != 0 and lib.lurk_hip_last_error() != b""
    assert lib.lurk_hip_trie_circuit_constraints(0, 0, 0, *[None] * 9) != 0 and lib.lurk_hip_last_error() != b""


def test_the_entry_points_are_declared_and_bound_under_abi_4():
    import subprocess
    import sys

    from lurk_beta_amd import _lib, trie_circuit

    hdr = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    assert re.search(r"^#define LURK_HIP_ABI_VERSION 4$", hdr, flags=re.M)  # additions only
    assert re.search(r"^#define LURK_TRIE_CIRCUIT_LOOKUP 0$", hdr, flags=re.M) and re.search(r"^#define LURK_TRIE_CIRCUIT_INSERT 1$", hdr, flags=re.M)
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    assert lib.lurk_hip_abi_version() == 4
    for name in NEW_SYMBOLS:
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, plain)
        assert decl, "include/lurk_hip.h does not declare " + name
        assert len(_lib.SIGNATURES[name][1]) == len(decl.group(1).split(",")) and hasattr(lib, name)
    assert (trie_circuit.LOOKUP, trie_circuit.INSERT) == (0, 1)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "rust", "gen_sys.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rs = open(os.path.join(ROOT, "rust", "lurk-hip-sys", "src", "ffi.rs")).read()
    assert all("pub fn %s(" % name in rs for name in NEW_SYMBOLS)
    assert "lurk_hip_trie_circuit_witness_dev" in open(os.path.join(ROOT, "rust", "lurk-hip-sys", "src", "trie.rs")).read()


# what the parent commit's poseidon.hip compiles to (VGPRs, scratch bytes per lane) at T = 9, the form the trie circuit's kernels share:
# the trace kernels moved into poseidon_trace.cuh as templates over the destination, and the existing instantiations may not pay for it
PARENT_T9 = {
    ("poseidon_trace_wide_kernel", "PallasFp"): (151, 0), ("poseidon_trace_wide_kernel", "PallasFq"): (151, 0), ("poseidon_trace_wide_kernel", "Bn254Fr"): (194, 0),
    ("poseidon_trace_batch_kernel", "PallasFp"): (234, 672), ("poseidon_trace_batch_kernel", "PallasFq"): (234, 672), ("poseidon_trace_batch_kernel", "Bn254Fr"): (240, 672),
    ("bit_decomp_trace_kernel", "PallasFp"): (49, 80), ("bit_decomp_trace_kernel", "PallasFq"): (49, 80), ("bit_decomp_trace_kernel", "Bn254Fr"): (49, 80),
}
# the other arities of the two trace kernels, (field, T) -> (VGPRs, scratch)
PARENT_WIDE = {("PallasFp", 4): (98, 0), ("PallasFp", 5): (105, 0), ("PallasFp", 7): (143, 0), ("PallasFq", 4): (98, 0), ("PallasFq", 5): (105, 0), ("PallasFq", 7): (143, 0),
               ("Bn254Fr", 4): (105, 0), ("Bn254Fr", 5): (113, 0), ("Bn254Fr", 7): (151, 0)}
PARENT_BATCH = {("PallasFp", 4): (144, 304), ("PallasFp", 5): (170, 384), ("PallasFp", 7): (200, 512), ("PallasFq", 4): (144, 304), ("PallasFq", 5): (170, 384),
                ("PallasFq", 7): (200, 512), ("Bn254Fr", 4): (152, 304), ("Bn254Fr", 5): (170, 384), ("Bn254Fr", 7): (192, 512)}
# registers the picks may add to a trace kernel: the digit, the entry's index, the eight loaded words and the nine limbs of its conversion
PICK_VGPRS = 24


def _find(usage, kernel, field, t=None):
    hits = [v for k, v in usage.items() if kernel in k and field in k and (t is None or "ELi%dE" % t in k)]
    assert len(hits) == 1, (kernel, field, t, len(hits))
    return hits[0]


def test_kernel_resources(tmp_path):
    import shutil
    from concurrent.futures import ThreadPoolExecutor

    from tests import kernel_resources as K

    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    with ThreadPoolExecutor(2) as ex:
        old, new = ex.map(lambda s: K.usage(s, str(tmp_path)), ["poseidon.hip", "trie_circuit.hip"])
    for field in ("PallasFp", "PallasFq", "Bn254Fr"):
        # the existing trace kernels compile to what the parent commit gives
        for (kernel, fld), (vgprs, scratch) in PARENT_T9.items():
            if fld == field:
                u = _find(old, kernel, field, None if kernel.startswith("bit") else 9)
                assert (u["vgprs"], u["agprs"], u["scratch"]) == (vgprs, 0, scratch), (kernel, field, u)
        for t in (4, 5, 7):
            for kernel, pins in (("poseidon_trace_wide_kernel", PARENT_WIDE), ("poseidon_trace_batch_kernel", PARENT_BATCH)):
                u = _find(old, kernel, field, t)
                assert (u["vgprs"], u["agprs"], u["scratch"]) == (*pins[(field, t)][:1], 0, pins[(field, t)][1]), (kernel, field, t, u)
        # the new ones: the scratch of the trace kernel of the same field and form compiled in this run, its registers plus the picks'
        for mine, theirs, t in (("poseidon_trace_wide_kernel", "poseidon_trace_wide_kernel", 9), ("poseidon_trace_batch_kernel", "poseidon_trace_batch_kernel", 9),
                                ("trie_circuit_head_kernel", "bit_decomp_trace_kernel", None)):  # trie_circuit.hip instantiates the two trace kernels on its own destination
            a, b = _find(new, mine, field), _find(old, theirs, field, t)
            assert "TrieCircuitJob" in next(k for k in new if mine in k and field in k)
            print(field, mine, a, "against", theirs, b)
            assert a["scratch"] <= b["scratch"], (mine, field, a, b)
            assert a["vgprs"] + a["agprs"] <= b["vgprs"] + b["agprs"] + PICK_VGPRS, (mine, field, a, b)
