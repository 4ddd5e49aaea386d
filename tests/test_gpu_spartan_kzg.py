"""GPU: the compressing SNARK on BN254 G1 (lurk_hip_spartan_kzg_*) against the Python-integer reference of tests/spartan_kzg_ref.py -
the prover element for element, the verifier's verdict, failed check and pairing inputs - and lurk_hip_fold_padded_dev against Python
integers.  Everything is exact: every comparison is equality."""
import copy
import ctypes
import random

import numpy as np
import pytest

from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK
from tests import spartan_kzg_ref as K

pytestmark = pytest.mark.gpu

PALLAS_P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
MOD = {0: PALLAS_P, 2: BN.BN254_R}
Q = BN.BN254_R
TAU = 0x2B0F3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % Q
SHAPES = [(2, 2, 1), (8, 16, 2), (16, 8, 2), (16, 16, 2)]
BATCHES = {"three": [(16, 64), (64, 32), (8, 16)], "one": [(8, 16)]}


def dev(p, ints):
    import torch

    return torch.from_numpy(BN.to_mont(p, ints).view(np.int64).reshape(-1, 4)).cuda()


def host(p, t):
    return BN.from_mont(p, t.cpu().numpy().view(np.uint64))


def mats_mont(mats):
    return [(np.array(ip, dtype=np.uint64), np.array(ix, dtype=np.uint64), BN.to_mont(Q, d) if len(d) else np.zeros((0, 4), dtype=np.uint64)) for ip, ix, d in mats]


def aff(jac):
    from lurk_beta_amd import point_to_affine

    return BN.from_xy(point_to_affine(BN.CURVE_BN254, jac))


@pytest.fixture(scope="module")
def key():
    from lurk_beta_amd import hyperkzg

    k = hyperkzg.trapdoor_key(TAU, 64)
    yield k
    k.close()


_ref = {}


def reference(nc, nv, nio, folded):
    """the instance, the reference's proof and its verdict: computed once, shared, never modified"""
    k = (nc, nv, nio, folded)
    if k not in _ref:
        it = K.make_instance(TAU, nc, nv, nio, 11 + nc + nv, folded)
        pf = K.prove(TAU, it["mats"], nc, nv, it["X"], it["comm_W"], it["comm_E"], it["u"], it["W"], it["E"])
        _ref[k] = (it, pf, K.verify(it["mats"], nc, nv, it["X"], it["comm_W"], it["comm_E"], it["u"], pf))
    return _ref[k]


def reference_batch(name):
    if name not in _ref:
        insts = [K.make_instance(TAU, nc, nv, 2, 23 + i, i % 2 == 1) for i, (nc, nv) in enumerate(BATCHES[name])]
        pf = K.prove_batched(TAU, insts)
        _ref[name] = (insts, pf, K.verify_batched(insts, pf))
    return _ref[name]


def device_instance(it, key):
    d_W, d_E = dev(Q, it["W"]), dev(Q, it["E"])
    cw = key.commit_device(d_W, it["num_vars"], is_mont=True)
    ce = key.commit_device(d_E, it["num_cons"], is_mont=True)
    assert aff(cw) == it["comm_W"] and aff(ce) == it["comm_E"]
    return dict(X=it["X"], u=it["u"], d_W=d_W, d_E=d_E, comm_W=cw, comm_E=ce)


# ---- lurk_hip_fold_padded_dev ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 2])
def test_fold_padded_matches_python_integers(f):
    """counts 1, 2, 5; lengths below, at and across the kernel's 1024-element tile; a zero-length vector passed as NULL; n_out above every
    length; coefficients 0, 1, p - 1 and random.  Under 10^4 elements in all."""
    from lurk_beta_amd.fold import fold_padded

    p = MOD[f]
    rng = random.Random(5 + f)
    rnd = lambda n: [rng.getrandbits(256) % p for _ in range(n)]
    cases = [((1, 5), 5), ((1, 5), 9), ((5, 1), 8), ((257, 64, 0), 300), ((1030, 1030), 1030), ((1030, 1030), 1100), ((7,), 7), ((7,), 33),
             ((3, 1025, 2, 64, 0), 1025), ((3, 1025, 2, 64, 0), 1500)]
    for lens, n_out in cases:
        vecs = [rnd(n) for n in lens]
        for v in vecs:
            for k, s in ((0, p - 1), (1, 0), (len(v) - 1, p - 1)):
                if 0 <= k < len(v):
                    v[k] = s
        d_vecs = [dev(p, v) if v else None for v in vecs]
        for coeffs in ([0, 1, p - 1, rng.getrandbits(256) % p, 1][:len(lens)], rnd(len(lens)), [p - 1] * len(lens)):
            got = host(p, fold_padded(f, d_vecs, BN.to_mont(p, coeffs), n_out))
            want = [sum(c * (v[j] if j < len(v) else 0) for c, v in zip(coeffs, vecs)) % p for j in range(n_out)]
            assert got == want, (f, lens, n_out)


@pytest.mark.parametrize("f", [0, 2])
def test_fold_padded_refusals(f):
    import torch

    from lurk_beta_amd import LurkHipError
    from lurk_beta_amd.fold import fold_padded

    p = MOD[f]
    a, b = dev(p, [1, 2, 3, 4, 5]), dev(p, [6])
    one = BN.to_mont(p, [1, 1])
    out = torch.empty((8, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(LurkHipError, match="count must be at least 1"):
        fold_padded(f, [], one, 8, out=out)
    with pytest.raises(LurkHipError, match="a null vector with a non-zero length"):
        fold_padded(f, [a, None], one, 8, out=out, lens=[5, 1])
    with pytest.raises(LurkHipError, match="a vector is longer than n_out"):
        fold_padded(f, [a, b], one, 4, out=out)
    whole = torch.empty((16, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(LurkHipError, match="the output may not overlap an input"):
        fold_padded(f, [whole[4:9], b], one, 8, out=whole[:8])
    assert host(p, fold_padded(f, [a, b], one, 8, out=out)) == [7, 2, 3, 4, 5, 0, 0, 0]  # the call still works after the refusals


# ---- single instance -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("folded", [False, True], ids=["strict", "relaxed"])
@pytest.mark.parametrize("nc,nv,nio", SHAPES)
def test_prover_equals_reference_and_verifier_accepts(nc, nv, nio, folded, key):
    from lurk_beta_amd import SpartanKzgProver, SpartanKzgVerifier

    it, ref_pf, (ref_L, ref_R, ref_ok, ref_code) = reference(nc, nv, nio, folded)
    assert ref_ok and ref_code == K.ACCEPTED and HK.trapdoor_holds(TAU, ref_L, ref_R)
    pr = SpartanKzgProver(mats_mont(it["mats"]), nc, nv, nio)
    di = device_instance(it, key)
    pf = pr.prove(di["X"], di["u"], di["d_W"], di["d_E"], di["comm_W"], di["comm_E"], key)
    assert set(pf) == set(ref_pf)
    for k in ref_pf:
        assert pf[k] == ref_pf[k], k
    ver = SpartanKzgVerifier.from_shape(pr.shape)
    ok, L, R = ver.verify(it["X"], it["u"], it["comm_W"], it["comm_E"], pf)
    assert ok and ver.last_failed_check == K.ACCEPTED
    assert aff(L) == ref_L and aff(R) == ref_R and HK.trapdoor_holds(TAU, aff(L), aff(R))
    pr.close()


def other_point(pt):
    return BN.BN254.add(pt, BN.BN254.gen)


def tamperings(pf, batched):
    """(name, tampered proof): one element changed in each field of the proof"""
    bump = lambda v: (v + 1) % Q
    eE, eW = ("evals_E", "evals_W") if batched else ("eval_E", "eval_W")
    out = []
    for name in ("polys_outer", "polys_inner", "polys_batch"):
        bad = copy.deepcopy(pf)
        bad[name][-1][1] = bump(bad[name][-1][1])
        out.append((name, bad))
    bad = copy.deepcopy(pf)
    if batched:
        bad["claims_outer"][0][2] = bump(bad["claims_outer"][0][2])
    else:
        bad["claims_outer"][2] = bump(bad["claims_outer"][2])
    out.append(("claims_outer", bad))
    for name in (eE, eW):
        bad = copy.deepcopy(pf)
        if batched:
            bad[name][0] = bump(bad[name][0])
        else:
            bad[name] = bump(bad[name])
        out.append((name, bad))
    for name, idx in (("evals_batch", 1), ("kzg_v", 0)):
        bad = copy.deepcopy(pf)
        bad[name][idx] = bump(bad[name][idx])
        out.append((name, bad))
    # kzg_com is absorbed before r is squeezed: another point there moves r away from the one the v were evaluated at, and the scalar
    # checks (each linear in r) fail - the reference says OPENING, not "accepted so far" (tests/test_spartan_kzg_cpu.py)
    bad = copy.deepcopy(pf)
    bad["kzg_com"][0] = other_point(bad["kzg_com"][0])
    out.append(("kzg_com", bad))
    return out


def check_tampering(ref_verify, dev_verify, last_failed, pf, batched):
    for name, bad in tamperings(pf, batched):
        _, _, ref_ok, ref_code = ref_verify(bad)
        ok, L, R = dev_verify(bad)
        assert not ref_ok and not ok, name
        assert last_failed() == ref_code, (name, ref_code)
        assert not L.any() and not R.any(), name
    # a quotient commitment replaced by another curve point (only d depends on it): accepted so far, the pairing decides
    for name, idx in (("kzg_w", 1),):
        bad = copy.deepcopy(pf)
        bad[name][idx] = other_point(bad[name][idx])
        ref_L, ref_R, ref_ok, _ = ref_verify(bad)
        ok, L, R = dev_verify(bad)
        assert ref_ok and ok, name
        assert aff(L) == ref_L and aff(R) == ref_R and not HK.trapdoor_holds(TAU, aff(L), aff(R)), name
    # malformed: an unreduced scalar, a point off the curve
    bad = copy.deepcopy(pf)
    bad["kzg_v"][1] += Q
    assert ref_verify(bad)[3] == K.MALFORMED
    assert not dev_verify(bad)[0] and last_failed() == K.MALFORMED
    bad = copy.deepcopy(pf)
    bad["polys_inner"][0][0] += Q
    assert not dev_verify(bad)[0] and last_failed() == K.MALFORMED
    bad = copy.deepcopy(pf)
    x, y = bad["kzg_w"][2]
    bad["kzg_w"][2] = (x, (y + 1) % BN.BN254_P)
    assert ref_verify(bad)[3] == K.MALFORMED
    assert not dev_verify(bad)[0] and last_failed() == K.MALFORMED


def test_verifier_rejects_tampering_where_the_reference_does(key):
    from lurk_beta_amd import SpartanKzgVerifier

    nc, nv, nio = 8, 16, 2  # ell = 4: kzg_com has entries
    it, pf, _ = reference(nc, nv, nio, True)
    ver = SpartanKzgVerifier(mats_mont(it["mats"]), nc, nv, nio)
    check_tampering(lambda p: K.verify(it["mats"], nc, nv, it["X"], it["comm_W"], it["comm_E"], it["u"], p),
                    lambda p: ver.verify(it["X"], it["u"], it["comm_W"], it["comm_E"], p), lambda: ver.last_failed_check, pf, False)
    # a wrong statement
    ok, _, _ = ver.verify(it["X"], (it["u"] + 1) % Q, it["comm_W"], it["comm_E"], pf)
    assert not ok and ver.last_failed_check == K.verify(it["mats"], nc, nv, it["X"], it["comm_W"], it["comm_E"], (it["u"] + 1) % Q, pf)[3]
    ver.close()


# ---- batched -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BATCHES))
def test_batched_prover_verifier_and_tampering(name, key):
    from lurk_beta_amd import BatchedSpartanKzgProver, BatchedSpartanKzgVerifier, SpartanKzgProver, SpartanKzgVerifier

    insts, ref_pf, (ref_L, ref_R, ref_ok, ref_code) = reference_batch(name)
    assert ref_ok and ref_code == K.ACCEPTED and HK.trapdoor_holds(TAU, ref_L, ref_R)
    provers = [SpartanKzgProver(mats_mont(it["mats"]), it["num_cons"], it["num_vars"], 2) for it in insts]
    pf = BatchedSpartanKzgProver(provers).prove([device_instance(it, key) for it in insts], key)
    assert set(pf) == set(ref_pf)
    for k in ref_pf:
        assert pf[k] == ref_pf[k], k
    ver = BatchedSpartanKzgVerifier([SpartanKzgVerifier.from_shape(p.shape) for p in provers])
    ok, L, R = ver.verify(insts, pf)
    assert ok and ver.last_failed_check == K.ACCEPTED
    assert aff(L) == ref_L and aff(R) == ref_R and HK.trapdoor_holds(TAU, aff(L), aff(R))
    check_tampering(lambda p: K.verify_batched(insts, p), lambda p: ver.verify(insts, p), lambda: ver.last_failed_check, pf, True)
    for p in provers:
        p.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_key_usable(key):
    import torch

    import lurk_beta_amd as L
    from lurk_beta_amd import LurkHipError, SpartanKzgProver, _lib, synth

    nc, nv, nio = 8, 16, 2
    it, ref_pf, _ = reference(nc, nv, nio, False)
    pr = SpartanKzgProver(mats_mont(it["mats"]), nc, nv, nio)
    di = device_instance(it, key)
    args = (di["X"], di["u"], di["d_W"], di["d_E"], di["comm_W"], di["comm_E"])
    for curve, name in ((0, "Pallas"), (3, "Grumpkin")):
        other = L.CommitmentKey(curve, synth.bases(curve, 16), n=16, device=True)
        with pytest.raises(LurkHipError, match=f"lurk_hip_spartan_kzg_prove_dev needs a key on BN254 G1: this key is on {name}"):
            pr.prove(*args, other)
        other.close()
    # a shape over field 0 (the matrices' values are only bytes to the constructor)
    pr0 = SpartanKzgProver(mats_mont(it["mats"]), nc, nv, nio, field_id=0)
    with pytest.raises(LurkHipError, match="the shapes are not over LURK_FIELD_BN254_FR"):
        pr0.prove(*args, key)
    pr0.close()
    from lurk_beta_amd import hyperkzg

    short = hyperkzg.trapdoor_key(TAU, 8)
    with pytest.raises(LurkHipError, match="the key has fewer points than the padded polynomials have elements"):
        pr.prove(*args, short)
    short.close()
    # N = 1, at the C ABI (no shape has one row): refused by name before the shapes are looked at
    out = _lib.SpartanKzgProofStruct()
    dummy = np.zeros(12, dtype=np.uint64)
    rc = _lib.load().lurk_hip_spartan_kzg_prove_dev(pr.shape._h, pr.shape_t._h, 1, 1, 0, key._ctx, None, _lib.ptr(dummy), _lib.ptr(di["d_W"]), _lib.ptr(di["d_E"]),
                                                    _lib.ptr(dummy), _lib.ptr(dummy), b"", 0, ctypes.byref(out), None)
    assert rc != 0 and "N = max(num_cons, num_vars) = 1" in _lib.load().lurk_hip_last_error().decode()
    # one proof after all the refusals: the key still proves
    pf = pr.prove(*args, key)
    for k in ref_pf:
        assert pf[k] == ref_pf[k], k
    pr.close()
    torch.cuda.synchronize()


# ---- one medium case ---------------------------------------------------------------------------------------------------------------------------
def test_medium_instance_2_12():
    """2^12 x 2^12: the sum-check tables no longer fit one workgroup's pass and HyperKZG's commitments cycle through several of the key's
    slots.  The device proof is checked by the device verifier and the trapdoor identity, not by the Python prover (minutes at this size)."""
    import torch

    from lurk_beta_amd import SpartanKzgProver, SpartanKzgVerifier, hyperkzg, synth

    n = 1 << 12
    # A z o B z = C z row by row: row i is (w_i) * (w_{i+1 mod n/2 ...}) = w_{n/2 + i} on the first half, 0 * 0 = 0 after it
    half = n // 2
    rng = random.Random(12)
    free = [rng.getrandbits(256) % Q for _ in range(half)]
    W = free + [free[i] * free[(i + 1) % half] % Q for i in range(half)]
    ip = np.array([min(i, half) for i in range(n + 1)], dtype=np.uint64)
    one = BN.to_mont(Q, [1] * half)
    A = (ip, np.arange(half, dtype=np.uint64), one)
    B = (ip, np.array([(i + 1) % half for i in range(half)], dtype=np.uint64), one)
    Cm = (ip, np.arange(half, n, dtype=np.uint64), one)
    X = [5, 7]
    key = hyperkzg.trapdoor_key(TAU, n)
    d_W = dev(Q, W)
    d_E = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    cw, ce = key.commit_device(d_W, n, is_mont=True), key.commit_device(d_E, n, is_mont=True)
    pr = SpartanKzgProver((A, B, Cm), n, n, 2)
    pf = pr.prove(X, 1, d_W, d_E, cw, ce, key)
    ver = SpartanKzgVerifier.from_shape(pr.shape)
    ok, L, R = ver.verify(X, 1, aff(cw), aff(ce), pf)
    assert ok and ver.last_failed_check == K.ACCEPTED
    assert aff(R) is not None and HK.trapdoor_holds(TAU, aff(L), aff(R))
    bad = copy.deepcopy(pf)
    bad["eval_W"] = (bad["eval_W"] + 1) % Q
    assert not ver.verify(X, 1, aff(cw), aff(ce), bad)[0] and ver.last_failed_check == K.INNER
    pr.close()
    key.close()
