"""The capped-grid passes of the field-vector kernels against Python integers.

The kernels behind the inner-product argument, the sum-check, the eq tables, HyperKZG and the Poseidon batches clamp their grid to
(CU count) x k workgroups and cover the rest by a grid-stride loop, a host-side sum of workgroup partials or a last-workgroup
reduction.  On a 256-CU device the second pass starts at 2^19 .. 2^21 elements, far beyond what an exact Python reference can
follow - so every case here runs twice: in this process with the device's own caps, and in one fresh interpreter per field with
LURK_GRID_CUS=1 (read once per process), where the caps are 4 .. 16 workgroups and the sizes below
reach a second pass.  lurk_hip_grid_cus reports the count in use: the child refuses to run unless it is 1, and every case computes
the number of passes it takes, ceil(work / (cus * workgroups per CU * 256)), from the launch code's constants and, in the child,
asserts >= 2 for the sizes meant to reach a second pass (STAR below) - nothing passes vacuously.

All comparisons are exact: Python integers modulo the field order."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import bn254_ref as BN
from tests import ipa_fast_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (0, 1, 2)
MOD = {0: R.PALLAS_P, 1: R.PALLAS_Q, 2: BN.BN254_R}
BLOCK = 256  # IPA_BLOCK = SC_BLOCK = HK_BLOCK = POSEIDON_BLOCK = FOLD_BLOCK

# workgroups per CU of each capped launch (ipa.hip, sumcheck.hip, verify.hip, poseidon.hip)
PER_CU_INNER_PRODUCT = 8   # inner_product, cross_products_kernel, fill_kernel
PER_CU_FOLD = 16           # fold_halves, ipa_round_scalars, ipa_coef_fold
PER_CU_SUMCHECK = 8        # sumcheck_round_kernel
PER_CU_EQ = 4              # eq_evals_kernel, per chunk of 2^EQ_LO_BITS outputs
EQ_LO_BITS = 10
PER_CU_S_VECTOR = 8        # ipa_s_vector_kernel
PER_CU_POSEIDON = 2        # poseidon_batch_kernel, poseidon_trace_batch_kernel
PER_CU_HK = 16             # hyperkzg.hip: hk_grid (hk_fold_pairs_kernel, hk_batch_kernel)
POSEIDON_WIDE_MAX = 8192   # up to here a batch runs the lane-cooperative kernel, whose grid is not capped


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def _lib():
    from lurk_beta_amd import _lib as L

    return L, L.load()


_cus = []


def grid_cus():
    """The CU count the caps are computed from, asked after a device call (before one the library assumes 256)."""
    if not _cus:
        import torch

        L, lib = _lib()
        out = np.zeros(4, dtype=np.uint64)
        L.check(lib.lurk_hip_inner_product_dev(1, None, None, 0, L.ptr(out), None))
        torch.cuda.synchronize()
        v = ctypes.c_int(-1)
        L.check(lib.lurk_hip_grid_cus(ctypes.byref(v)))
        _cus.append(v.value)
    return _cus[0]


def passes(work, per_cu, star=False, unit=BLOCK):
    """Passes of a launch capped at cus * per_cu workgroups of `unit` work items; a STAR size must take >= 2 of them under one CU."""
    n = max(1, -(-work // (grid_cus() * per_cu * unit)))
    if star and grid_cus() == 1:
        assert n >= 2, (work, per_cu, n)
    return n


def to_dev(p, ints):
    import torch

    if not ints:
        return torch.zeros((0, 4), dtype=torch.int64, device="cuda")
    return torch.from_numpy(ipa_fast_ref.limbs([(x << 256) % p for x in ints]).view(np.int64)).cuda()


def mont(p, x):
    return ipa_fast_ref.limbs([(x << 256) % p])


def to_host(p, t):
    return BN.from_mont(p, t.cpu().numpy().view(np.uint64))


def vector(p, n, seed, kind="mixed"):
    """0, 1 and p - 1 among seeded random values (as many of them as fit), or all p - 1"""
    if kind == "ones":
        return [p - 1] * n
    rng = random.Random(seed * 1000003 + n)
    v = [rng.getrandbits(256) % p for _ in range(n)]
    # the last element is the one a ragged tail or a skipped pass loses: it is never the 0 (whose loss no sum or product would show)
    for k, s in ((n // 2, 0), (n // 3, 0), (2 * n // 3, p - 1), (0, 1), (n - 1, p - 1)):
        if n >= 3 or (n >= 1 and k == n - 1):
            v[k] = s
    return v


# ---- the cases: each runs under whatever caps the process has ----------------------------------------------------------------------
STAR_IP = (2049, 4099, 6145)


def case_inner_product(f):
    L, lib = _lib()
    p = MOD[f]
    out = np.zeros(4, dtype=np.uint64)
    for n in (0, 1, 255, 256, 257, 2047, 2048, 2049, 4099, 6145):
        passes(n, PER_CU_INNER_PRODUCT, star=n in STAR_IP)
        for kind in ("mixed", "ones"):
            a, b = vector(p, n, 11 + f, kind), vector(p, n, 12 + f, kind)
            b = b[::-1] if kind == "mixed" else b   # (0 against 0 and p - 1 against p - 1 would leave no cross terms of the specials)
            da, db = to_dev(p, a), to_dev(p, b)
            out[:] = 0xDEADBEEF
            L.check(lib.lurk_hip_inner_product_dev(f, L.ptr(da) if n else None, L.ptr(db) if n else None, n, L.ptr(out), None))
            assert BN.from_mont(p, out) == [sum(x * y for x, y in zip(a, b)) % p], (f, n, kind)


STAR_FOLD = (8194, 24578)


def case_fold_halves(f):
    import torch

    L, lib = _lib()
    p = MOD[f]
    rng = random.Random(21 + f)
    x, y = rng.getrandbits(256) % p, rng.getrandbits(256) % p
    for n in (2, 4, 510, 512, 514, 8190, 8192, 8194, 24578):
        h = n // 2
        passes(h, PER_CU_FOLD, star=n in STAR_FOLD)
        for kind, pairs in (("mixed", ((0, x), (x, 0), (1, 1), (p - 1, x), (x, y))), ("ones", ((x, y),))):
            v = vector(p, n, 22 + f, kind)
            base = to_dev(p, v)
            for lo, hi in pairs:
                d = base.clone()
                lo_m, hi_m = mont(p, lo), mont(p, hi)
                L.check(lib.lurk_hip_fold_halves_dev(f, L.ptr(d), n, L.ptr(lo_m), L.ptr(hi_m), None))
                torch.cuda.synchronize()
                got = to_host(p, d)
                assert got[:h] == [(lo * v[i] + hi * v[h + i]) % p for i in range(h)], (f, n, kind, lo, hi)
                assert got[h:] == v[h:], (f, n, kind, "the upper half is not the fold's to write")


NM = ((8, 2), (8, 8), (4096, 4096), (8192, 2), (8192, 64), (8192, 8192), (12288, 4096))
STAR_N = (8192, 12288)


def _round_scalars_want(p, a, coef, n, m):
    """ipa.hip, the comment above ipa_round_scalars_kernel: v[i] = a[(i mod m) -+ m/2] coef[i]; L takes the upper halves"""
    h = m // 2
    v, hi = [], []
    for i in range(n):
        q = i & (m - 1)
        hi.append(q >= h)
        v.append(a[q - h if q >= h else q + h] * coef[i] % p)
    return v, hi


def case_round_scalars(f):
    import torch

    L, lib = _lib()
    p = MOD[f]
    for n, m in NM:
        passes(n, PER_CU_FOLD, star=n in STAR_N)
        for kind in ("mixed", "ones"):
            a, coef = vector(p, m, 31 + f, kind), vector(p, n, 32 + f, kind)[::-1]
            v, hi = _round_scalars_want(p, a, coef, n, m)
            da, dc = to_dev(p, a), to_dev(p, coef)
            canary = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
            ol, orr, om = canary.clone(), canary.clone(), canary.clone()
            L.check(lib.lurk_hip_ipa_round_scalars_dev(f, L.ptr(da), m, L.ptr(dc), n, L.ptr(ol), L.ptr(orr), None))
            L.check(lib.lurk_hip_ipa_round_scalars_dev(f, L.ptr(da), m, L.ptr(dc), n, L.ptr(om), None, None))  # the merged form
            torch.cuda.synchronize()
            assert to_host(p, ol) == [x if t else 0 for x, t in zip(v, hi)], (f, n, m, kind, "L")
            assert to_host(p, orr) == [0 if t else x for x, t in zip(v, hi)], (f, n, m, kind, "R")
            assert to_host(p, om) == v, (f, n, m, kind, "merged")
            assert to_host(p, da) == a and to_host(p, dc) == coef  # the inputs are read only


def case_coef_fold(f):
    import torch

    L, lib = _lib()
    p = MOD[f]
    rng = random.Random(41 + f)
    x, y = rng.getrandbits(256) % p, rng.getrandbits(256) % p
    for n, m in NM:
        passes(n, PER_CU_FOLD, star=n in STAR_N)
        for kind, pairs in (("mixed", ((x, y), (0, 1), (p - 1, x))), ("ones", ((x, y),))):
            coef = vector(p, n, 42 + f, kind)
            base = to_dev(p, coef)
            for lo, hi in pairs:
                d = base.clone()
                lo_m, hi_m = mont(p, lo), mont(p, hi)
                L.check(lib.lurk_hip_ipa_coef_fold_dev(f, L.ptr(d), n, m, L.ptr(lo_m), L.ptr(hi_m), None))
                torch.cuda.synchronize()
                # ipa.hip, the comment above ipa_coef_fold_kernel: coef[i] *= s_lo if (i mod m) < m/2 else s_hi
                assert to_host(p, d) == [c * (hi if (i & (m - 1)) >= m // 2 else lo) % p for i, c in enumerate(coef)], (f, n, m, kind, lo, hi)


def case_eq_evals(f):
    from lurk_beta_amd import sumcheck as S

    p = MOD[f]
    for ell in (10, 11, 12, 13):
        passes(1 << (ell - EQ_LO_BITS), PER_CU_EQ, star=ell == 13, unit=1)  # 2^(ell - 10) chunks, one per workgroup and pass
        rng = random.Random(51 + f + ell)
        plain = [rng.getrandbits(256) % p or 1 for _ in range(ell)]
        special = list(plain)  # p - 1 among the chunk's bits (every chunk keeps a non-zero factor), 0 and 1 among the low bits
        special[0], special[-1], special[-2] = p - 1, 0, 1
        for r in (plain, special):
            got = to_host(p, S.eq_evals(f, BN.to_mont(p, r)))
            assert got == R.eq_evals(p, r), (f, ell)


_SC_WANT = {}


def case_sumcheck(f):
    """S.prove with every round on the device: the first round of 2^13 takes two passes under one CU, the first BINDING round of 2^14
    two as well; the second proof on the same stream finds the ticket counter and the scratch as the first left them."""
    from lurk_beta_amd import sumcheck as S

    p = MOD[f]
    before = os.environ.get("LURK_SUMCHECK_HOST_TAIL_LOG")
    os.environ["LURK_SUMCHECK_HOST_TAIL_LOG"] = "0"  # read per call
    try:
        for ell in (13, 14):
            n = 1 << ell
            passes(n // 2, PER_CU_SUMCHECK, star=True)                # round 0: sums over the tables as they are
            passes(n // 4, PER_CU_SUMCHECK, star=ell == 14)           # round 1: bind, then sums
            for ntab in (4, 2):
                tabs = [vector(p, n, 61 + 10 * f + k + ntab) for k in range(ntab)]
                comb = (lambda a, b, c, d: a * (b * c - d)) if ntab == 4 else (lambda a, b: a * b)
                claim = sum(comb(*[t[i] for t in tabs]) for i in range(n)) % p
                rng = random.Random(62 + f + ell)
                chal = [rng.getrandbits(256) % p for _ in range(ell)]
                if (f, ell, ntab) not in _SC_WANT:
                    _SC_WANT[(f, ell, ntab)] = R.sumcheck_prove(p, claim, tabs, chal)
                want_polys, want_finals, want_claim = _SC_WANT[(f, ell, ntab)]
                for proof in ("first", "second"):
                    got_polys, got_finals, got_claim = S.prove(f, p, claim, [to_dev(p, t) for t in tabs], lambda j, poly: chal[j])
                    assert got_polys == want_polys, (f, ell, ntab, proof)
                    assert got_finals == want_finals and got_claim == want_claim, (f, ell, ntab, proof)
    finally:
        if before is None:
            del os.environ["LURK_SUMCHECK_HOST_TAIL_LOG"]
        else:
            os.environ["LURK_SUMCHECK_HOST_TAIL_LOG"] = before


def case_s_vector(f):
    """verify.hip: ipa_s_vector, s[i] = prod_j (bit_(ell-1-j)(i) ? r_j : r_j^-1)"""
    from lurk_beta_amd import ipa

    p = MOD[f]
    for ell in (11, 12, 13):
        passes(1 << ell, PER_CU_S_VECTOR, star=ell >= 12)
        rng = random.Random(71 + f + ell)
        r = [rng.getrandbits(256) % p or 1 for _ in range(ell)]
        r[0], r[-1] = p - 1, 1
        want = [1]
        for rj in r:
            ri = pow(rj, p - 2, p)
            want = [y for x in want for y in (x * ri % p, x * rj % p)]
        assert to_host(p, ipa.s_vector(f, r)) == want, (f, ell)


POSEIDON_ARITY = {0: 6, 1: 8, 2: 3}


def case_poseidon_batch(f):
    """the smallest batch that leaves the lane-cooperative kernel (test_gpu_poseidon.test_batch_matches_oracle's 1000 hashes never do):
    8193 hashes through poseidon_batch_kernel, 17 passes of 2 workgroups under one CU"""
    from lurk_beta_amd import poseidon_batch

    p = MOD[f]
    n, arity = POSEIDON_WIDE_MAX + 1, POSEIDON_ARITY[f]
    passes(n, PER_CU_POSEIDON, star=True)
    pre = C.synth_scalars(f, 80 + arity, 0, n * arity).reshape(n, arity, 4)
    pre[0] = 0
    pre[n - 1] = C.ints_to_limbs([p - 1] * arity)
    assert np.array_equal(poseidon_batch(f, arity, pre), C.poseidon_batch(f, arity, pre))


def _object_ints(a):
    """(n, 4) u64 limbs -> numpy object array of Python integers"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return sum(a[:, k].astype(object) << (64 * k) for k in range(4))


def case_block_sum_beyond_256_workgroups():
    """sc_block_sum's last workgroup adds every workgroup's partial sums, 256 lanes at a time (b += SC_BLOCK): 512 workgroups here, on
    the device's own caps (one lurk_hip_sumcheck_round_dev call each; the cached per-stream scratch and its ticket counter are shared by
    the two calls)."""
    import torch

    L, lib = _lib()
    f = 1
    p = MOD[f]
    if grid_cus() * PER_CU_SUMCHECK < 512:
        pytest.fail("the device's cap is below 512 workgroups: this case needs the default caps of a device with >= 64 CUs")
    rinv = pow(1 << 256, -1, p)

    def tables(k, n, stream):
        can = [C.synth_scalars(f, stream + i, i % 2, n) for i in range(k)]
        for t in can:
            t[0], t[1], t[n - 1] = C.ints_to_limbs([0, 1, p - 1])
        return [_object_ints(t) for t in can], [torch.from_numpy(C.to_mont(f, t).view(np.int64)).cuda() for t in can]

    def evals(dev, n, r_mont, nv):
        ptrs = (ctypes.c_void_p * len(dev))(*[L.ptr(t) for t in dev])
        ev = np.zeros((3, 4), dtype=np.uint64)
        L.check(lib.lurk_hip_sumcheck_round_dev(f, 3 if len(dev) == 4 else 2, ptrs, n, L.ptr(r_mont) if r_mont is not None else None, L.ptr(ev), None))
        return BN.from_mont(p, ev[:nv])

    # cubic, no bind, 2^18: work = 2^17 pairs = 512 workgroups
    n = 1 << 18
    h = n // 2
    assert h // BLOCK == 512
    ints, dev = tables(4, n, 90)
    lo, hi = [t[:h] for t in ints], [t[h:] for t in ints]
    comb = lambda a, b, c, d: int((a * (b * c - d)).sum() % p)
    want = [comb(*lo), comb(*[2 * y - x for x, y in zip(lo, hi)]), comb(*[3 * y - 2 * x for x, y in zip(lo, hi)])]
    assert evals(dev, n, None, 3) == want
    for t, d in zip(ints, dev):  # nothing is bound: the tables are as they were
        assert (_object_ints(d.cpu().numpy().view(np.uint64)) * rinv % p == t).all()

    # quadratic, with bind, 2^19: the bound tables have 2^18 elements, work = 2^17 pairs = 512 workgroups
    n = 1 << 19
    m = n // 2
    q = m // 2
    assert q // BLOCK == 512
    ints, dev = tables(2, n, 95)
    r = random.Random(96).getrandbits(256) % p
    bound = [(t[:m] + r * (t[m:] - t[:m])) % p for t in ints]
    lo, hi = [t[:q] for t in bound], [t[q:] for t in bound]
    want = [int((lo[0] * lo[1]).sum() % p), int(((2 * hi[0] - lo[0]) * (2 * hi[1] - lo[1])).sum() % p)]
    assert evals(dev, n, mont(p, r), 2) == want
    torch.cuda.synchronize()
    for t, b, d in zip(ints, bound, dev):
        got = _object_ints(d.cpu().numpy().view(np.uint64)) * rinv % p
        assert (got[:m] == b).all() and (got[m:] == t[m:]).all()


_IPA_WANT = {}


def case_ipa_prover():
    """lurk_hip_ipa_prove_dev on Pallas at 2^13: round 0 has h = 4096, two passes of cross_products_kernel under one CU (8 workgroups),
    and fill_kernel takes four; the key is never folded (LURK_IPA_FOLD_MIN_LOG=0), under a resident plain key (two commitments per
    round) and a resident window-table key (the merged pair form).  Every L, R, a_hat and ck_hat against tests/ipa_fast_ref.py."""
    from lurk_beta_amd import CommitmentKey, ipa, point_to_affine

    c, sf, bf, log_n = 0, 1, 0, 13
    q = MOD[sf]
    n = 1 << log_n
    passes(n // 2, PER_CU_INNER_PRODUCT, star=True)  # cross_products_kernel, round 0
    passes(n, PER_CU_INNER_PRODUCT, star=True)       # fill_kernel
    B = C.synth_bases(c, n + 1)
    a, b = vector(q, n, 101), vector(q, n, 102)[::-1]
    rng = random.Random(103)
    r0 = rng.getrandbits(256) % q or 1
    chal = [rng.getrandbits(256) % q or 1 for _ in range(log_n)]
    if "want" not in _IPA_WANT:
        _IPA_WANT["want"] = ipa_fast_ref.ipa_prove(c, B, a, b, r0, chal)
    want_L, want_R, want_a, want_ck = _IPA_WANT["want"]
    ck_c_jac = np.concatenate([B[n], C.to_mont(bf, C.ints_to_limbs([1])).reshape(4)])
    aff = lambda jac: (lambda xy: None if xy == (0, 0) else xy)(point_to_affine(c, jac))
    before = os.environ.get("LURK_IPA_FOLD_MIN_LOG")
    os.environ["LURK_IPA_FOLD_MIN_LOG"] = "0"  # read per call
    try:
        for form, kw in (("resident_plain_key", dict(precompute=False)), ("resident_window_table_key", dict(precompute=True, window_bits=16))):
            key = CommitmentKey(c, B, **kw)
            try:
                got_L, got_R, got_a, got_ck = ipa.prove(c, q, None, ck_c_jac, to_dev(q, a), to_dev(q, b), r0, lambda j, l, r: chal[j], key=key)
            finally:
                key.close()
            assert len(got_L) == log_n and len(got_R) == log_n
            for j in range(log_n):
                assert aff(got_L[j]) == want_L[j], (form, "L", j)
                assert aff(got_R[j]) == want_R[j], (form, "R", j)
            assert got_a == want_a, form
            assert tuple(C.limbs_to_ints(C.from_mont(bf, got_ck.reshape(2, 4)))) == want_ck, form
    finally:
        if before is None:
            del os.environ["LURK_IPA_FOLD_MIN_LOG"]
        else:
            os.environ["LURK_IPA_FOLD_MIN_LOG"] = before


FIELD_CASES = (case_inner_product, case_fold_halves, case_round_scalars, case_coef_fold, case_eq_evals, case_sumcheck, case_s_vector, case_poseidon_batch)


# ---- this process: the device's own caps ------------------------------------------------------------------------------------------
def test_default_caps_come_from_the_device(hip):
    import torch

    assert "LURK_GRID_CUS" not in os.environ, "the suite runs with the device's own caps"
    assert grid_cus() == torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("f", FIELDS)
@pytest.mark.parametrize("case", FIELD_CASES, ids=lambda c: c.__name__[5:])
def test_default_caps(hip, case, f):
    case(f)


def test_block_sum_beyond_256_workgroups(hip):
    case_block_sum_beyond_256_workgroups()


def test_ipa_prover_at_2_13(hip):
    case_ipa_prover()


# ---- one CU: a fresh interpreter per field ---------------------------------------------------------------------------------------
def child_main(f):
    """Runs in the child (LURK_GRID_CUS=1).  HyperKZG: test_gpu_hyperkzg's fold lengths 8191, 8193 and 65537 straddle the cap of 16
    workgroups (4096 pairs: 1, 2 and 9 passes) and its 2^16 prover takes hk_batch_kernel through 16; Poseidon:
    test_batch_matches_oracle stays in the lane-cooperative kernel (uncapped) - case_poseidon_batch above is the capped one - and the
    slot-witness test's 12 600 hash4 slots take poseidon_trace_batch_kernel through 25 passes."""
    from tests import test_gpu_hyperkzg as HKT
    from tests import test_gpu_poseidon as PT
    from tests import test_gpu_witness as WT

    L, lib = _lib()
    assert os.environ.get("LURK_GRID_CUS") == "1"
    assert grid_cus() == 1, "LURK_GRID_CUS=1 did not take effect: every case below would pass vacuously"
    for case in FIELD_CASES:
        case(f)
        print("ok", case.__name__, flush=True)
    passes((8193 + 1) // 2, PER_CU_HK, star=True)
    passes((65537 + 1) // 2, PER_CU_HK, star=True)
    HKT.test_fold_pairs_matches_python_integers(f)
    print("ok hyperkzg fold_pairs", flush=True)
    PT.test_batch_matches_oracle(lib, f, POSEIDON_ARITY[f])
    print("ok poseidon batch (wide)", flush=True)
    if f == 1:  # Pallas' scalar field: the opening argument; the slot-witness test is written for this field
        passes(12600, PER_CU_POSEIDON, star=True)
        WT.test_large_batch_takes_the_lane_per_hash_kernel(lib)
        print("ok poseidon trace", flush=True)
        case_ipa_prover()
        print("ok ipa prover", flush=True)
    if f == 2:  # BN254's scalar field: the HyperKZG prover
        HKT.test_prover_matches_the_trapdoor_reference(16)
        print("ok hyperkzg prover", flush=True)


CHILD = r'''
import sys
sys.path.insert(0, %r)
import torch
from tests import test_gpu_grid_caps as T
T.child_main(%d)
print("child ok")
'''


@pytest.mark.parametrize("f", FIELDS)
def test_one_cu_caps(hip, f):
    e = dict(os.environ, LURK_GRID_CUS="1")
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, f)], env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-600:] + p.stderr[-3000:]
    assert "child ok" in p.stdout
