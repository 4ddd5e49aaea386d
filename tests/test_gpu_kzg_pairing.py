"""GPU: the KZG verifiers that DECIDE (include/lurk_hip.h: lurk_hip_hyperkzg_verify, lurk_hip_spartan_kzg_verify_pairing_dev /
_batch_dev) on proofs of the device provers under a trapdoor key and the verifier key [tau]H, and lurk_hip_kzg_key_check_dev on honest
and damaged resident keys in every form.  The pairing itself is compared with a reference in tests/test_bn254_pairing_cpu.py; here the
decisions are checked against what the trapdoor says (L == [tau]R) and against the codes the up-to-the-pairing calls report."""
import copy
import random

import numpy as np
import pytest

from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK
from tests import spartan_kzg_ref as K

pytestmark = pytest.mark.gpu

Q = BN.BN254_R
TAU = 0x2B0F3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % Q
TAU_OTHER = (TAU * 3 + 1) % Q
PAIRING, VERIFY_PAIRING = 3, 6  # LURK_HYPERKZG_PAIRING, LURK_VERIFY_PAIRING
SHAPES = [(2, 2, 1), (8, 4, 1)]  # N = 2 (kzg_com is NULL) and 8 x 4
FORMS = {"plain": dict(), "table": dict(precompute=True, window_bits=16), "small": dict(precompute=True, small_form=True)}

jac = lambda P: BN.jacobian(BN.BN254, P)


def dev(p, ints):
    import torch

    return torch.from_numpy(BN.to_mont(p, ints).view(np.int64).reshape(-1, 4)).cuda()


def aff(j):
    from lurk_beta_amd import point_to_affine

    return BN.from_xy(point_to_affine(BN.CURVE_BN254, j))


_vk = {}


def vk(tau):
    from lurk_beta_amd import hyperkzg

    if tau not in _vk:
        _vk[tau] = hyperkzg.trapdoor_vk(tau)
    return _vk[tau]


def malformed_keys():
    from lurk_beta_amd import pairing

    h = pairing.g2_to_ints(pairing.g2_generator())
    off = (h[0], ((h[1][0] + 1) % BN.BN254_P, h[1][1]))
    return [pairing.g2_from_ints(off), np.zeros(16, dtype=np.uint64)]  # off the twist, the identity


# ---- HyperKZG ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", (1, 2, 5))
def test_hyperkzg_device_proofs_are_decided(ell):
    """ell = 1 has no com, ell = 2 has one.  The device prover under the trapdoor key; the verifier with [tau]H accepts, one replaced W_t
    or the verifier key of another tau fails the pairing and nothing else."""
    from lurk_beta_amd import hyperkzg

    rng = random.Random(50 * ell)
    n = 1 << ell
    p0 = [rng.getrandbits(256) % Q for _ in range(n)]
    p0[0], p0[-1] = Q - 1, 1
    x = [rng.getrandbits(256) % Q for _ in range(ell)]
    ck = hyperkzg.trapdoor_key(TAU, n)
    tr, seen = HK.Transcript(), {}

    def challenge(stage, data):
        seen[stage] = tr(stage, [aff(j) for j in data] if stage == 0 else data)
        return seen[stage]

    pf = hyperkzg.prove(ck, dev(Q, p0), x, challenge)
    c = jac(HK.commit_trapdoor(TAU, p0))
    at_w = tr._h.copy()  # the transcript before W is absorbed: a verifier given another W squeezes another d from here
    d = tr(2, [aff(j) for j in pf["w"]])
    args = (ell, c, x, pf["y"], pf["com"], pf["v"])
    assert hyperkzg.verify(*args, pf["w"], seen[0], seen[1], d, vk(TAU)) == (True, hyperkzg.ACCEPTED)
    L, R, ok, _ = hyperkzg.pairing_inputs(*args, pf["w"], seen[0], seen[1], d)
    assert ok and HK.trapdoor_holds(TAU, aff(L), aff(R))
    assert hyperkzg.verify(*args, pf["w"], seen[0], seen[1], d, vk(TAU_OTHER)) == (False, PAIRING) == (False, hyperkzg.PAIRING)
    for t in range(3):
        w = pf["w"].copy()
        w[t] = jac(BN.BN254.add(aff(w[t]), BN.BN254.gen))
        fork = HK.Transcript()
        fork._h = at_w.copy()
        d_bad = fork(2, [aff(j) for j in w])  # (the verifier's own d follows the W it was given; either d fails)
        for dd in (d, d_bad):
            L, R, ok, _ = hyperkzg.pairing_inputs(*args, w, seen[0], seen[1], dd)
            assert ok and not HK.trapdoor_holds(TAU, aff(L), aff(R))
            assert hyperkzg.verify(*args, w, seen[0], seen[1], dd, vk(TAU)) == (False, PAIRING), t
    for bad in malformed_keys():
        assert hyperkzg.verify(*args, pf["w"], seen[0], seen[1], d, bad) == (False, hyperkzg.MALFORMED)
    assert hyperkzg.verify(*args, pf["w"], seen[0], seen[1], d, vk(TAU)) == (True, hyperkzg.ACCEPTED)
    ck.close()


# ---- Spartan-KZG ---------------------------------------------------------------------------------------------------------------------------
def mats_mont(mats):
    return [(np.array(ip, dtype=np.uint64), np.array(ix, dtype=np.uint64), BN.to_mont(Q, d) if len(d) else np.zeros((0, 4), dtype=np.uint64)) for ip, ix, d in mats]


@pytest.fixture(scope="module")
def key():
    from lurk_beta_amd import hyperkzg

    k = hyperkzg.trapdoor_key(TAU, 8)
    yield k
    k.close()


_inst = {}


def instance(nc, nv, nio):
    if (nc, nv, nio) not in _inst:
        _inst[(nc, nv, nio)] = K.make_instance(TAU, nc, nv, nio, 31 + nc + nv, True)
    return _inst[(nc, nv, nio)]


def device_instance(it, key):
    d_W, d_E = dev(Q, it["W"]), dev(Q, it["E"])
    cw, ce = key.commit_device(d_W, it["num_vars"], is_mont=True), key.commit_device(d_E, it["num_cons"], is_mont=True)
    assert aff(cw) == it["comm_W"] and aff(ce) == it["comm_E"]
    return dict(X=it["X"], u=it["u"], d_W=d_W, d_E=d_E, comm_W=cw, comm_E=ce)


def check_decisions(pf, ref_verify, up_to, up_to_code, decide, decide_code, batched):
    """up_to(proof) -> (ok, L, R) is the existing call, decide(proof, tau_h) -> bool the new one"""
    ref_L, ref_R, ref_ok, _ = ref_verify(pf)
    assert ref_ok and HK.trapdoor_holds(TAU, ref_L, ref_R)
    ok, L, R = up_to(pf)
    assert ok and (aff(L), aff(R)) == (ref_L, ref_R)  # the up-to-the-pairing call is what it was
    assert decide(pf, vk(TAU)) is True and decide_code() == K.ACCEPTED
    assert decide(pf, vk(TAU_OTHER)) is False and decide_code() == VERIFY_PAIRING
    # a quotient commitment replaced by another curve point: every check of today passes, only the pairing can tell
    bad = copy.deepcopy(pf)
    bad["kzg_w"][1] = BN.BN254.add(bad["kzg_w"][1], BN.BN254.gen)
    ok, L, R = up_to(bad)
    assert ok and not HK.trapdoor_holds(TAU, aff(L), aff(R))
    assert decide(bad, vk(TAU)) is False and decide_code() == VERIFY_PAIRING
    # a changed sum-check coefficient keeps the code it has today
    for name in ("polys_outer", "polys_inner", "polys_batch"):
        bad = copy.deepcopy(pf)
        bad[name][-1][1] = (bad[name][-1][1] + 1) % Q
        ok, _, _ = up_to(bad)
        today = up_to_code()
        assert not ok and today == ref_verify(bad)[3] and today not in (K.ACCEPTED, VERIFY_PAIRING), name
        assert decide(bad, vk(TAU)) is False and decide_code() == today, name
    for mal in malformed_keys():
        assert decide(pf, mal) is False and decide_code() == K.MALFORMED
    ok, L, R = up_to(pf)
    assert ok and (aff(L), aff(R)) == (ref_L, ref_R)
    assert decide(pf, vk(TAU)) is True and decide_code() == K.ACCEPTED


@pytest.mark.parametrize("nc,nv,nio", SHAPES)
def test_spartan_kzg_single_proofs_are_decided(nc, nv, nio, key):
    from lurk_beta_amd import SpartanKzgProver, SpartanKzgVerifier

    it = instance(nc, nv, nio)
    pr = SpartanKzgProver(mats_mont(it["mats"]), nc, nv, nio)
    di = device_instance(it, key)
    pf = pr.prove(di["X"], di["u"], di["d_W"], di["d_E"], di["comm_W"], di["comm_E"], key)
    ver = SpartanKzgVerifier.from_shape(pr.shape)
    st = (it["X"], it["u"], it["comm_W"], it["comm_E"])
    check_decisions(pf, lambda p: K.verify(it["mats"], nc, nv, it["X"], it["comm_W"], it["comm_E"], it["u"], p), lambda p: ver.verify(*st, p),
                    lambda: ver.last_failed_check, lambda p, t: ver.verify_pairing(*st, p, t), lambda: ver.last_failed_check, False)
    pr.close()


def test_spartan_kzg_batched_proofs_are_decided(key):
    from lurk_beta_amd import BatchedSpartanKzgProver, BatchedSpartanKzgVerifier, SpartanKzgProver, SpartanKzgVerifier

    insts = [instance(*s) for s in SHAPES]
    provers = [SpartanKzgProver(mats_mont(it["mats"]), it["num_cons"], it["num_vars"], len(it["X"])) for it in insts]
    pf = BatchedSpartanKzgProver(provers).prove([device_instance(it, key) for it in insts], key)
    ver = BatchedSpartanKzgVerifier([SpartanKzgVerifier.from_shape(p.shape) for p in provers])
    check_decisions(pf, lambda p: K.verify_batched(insts, p), lambda p: ver.verify(insts, p), lambda: ver.last_failed_check,
                    lambda p, t: ver.verify_pairing(insts, p, t), lambda: ver.last_failed_check, True)
    for p in provers:
        p.close()


# ---- the key check -------------------------------------------------------------------------------------------------------------------------
def tau_key(bases, n, form):
    from lurk_beta_amd import CommitmentKey

    return CommitmentKey(BN.CURVE_BN254, bases, n=n, device=True, **FORMS[form])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", (1, 2, 5, 1025))
def test_key_check_on_honest_and_damaged_keys(n, form):
    import torch

    from lurk_beta_amd import hyperkzg

    seeds = (7, 0xDEADBEEF12345)
    bases = hyperkzg.kzg_bases(TAU, n)
    torch.cuda.synchronize()
    ck = tau_key(bases, n, form)
    assert ck.info()["form"] == form
    for seed in seeds:
        assert hyperkzg.key_check(ck, vk(TAU), seed) is True
        assert hyperkzg.key_check(ck, vk(TAU_OTHER), seed) is (n == 1)  # (one point says nothing about tau: ck[0] == G is all there is)
    # afterwards the key commits as before: sum_i s_i [tau^i]G = [s(tau)]G
    rng = random.Random(n)
    s = [rng.getrandbits(256) % Q for _ in range(n)]
    assert aff(ck.commit_device(dev(Q, s), n, is_mont=True)) == HK.commit_trapdoor(TAU, s)
    ck.close()
    # point j replaced by another curve point
    other = torch.from_numpy(BN.affine_bases(BN.BN254, [BN.BN254.mul(0xABCDEF, BN.BN254.gen)]).view(np.int64)).cuda()
    for j in sorted({0, n // 2, n - 1}):
        damaged = bases.clone()
        damaged[j] = other[0]
        torch.cuda.synchronize()
        bad = tau_key(damaged, n, form)
        for seed in seeds:
            assert hyperkzg.key_check(bad, vk(TAU), seed) is False, j
        bad.close()


def test_key_check_refusals_and_a_key_that_is_no_powers_of_tau_key():
    import torch

    from lurk_beta_amd import CommitmentKey, LurkHipError, hyperkzg, synth

    n = 64
    gr = CommitmentKey(BN.CURVE_GRUMPKIN, synth.bases(BN.CURVE_GRUMPKIN, n), n=n, device=True)
    with pytest.raises(LurkHipError, match="lurk_hip_kzg_key_check_dev needs a key on BN254 G1: this key is on Grumpkin"):
        hyperkzg.key_check(gr, vk(TAU), 1)
    gr.close()
    pa = CommitmentKey(0, synth.bases(0, n), n=n, device=True)
    with pytest.raises(LurkHipError, match="this key is on Pallas"):
        hyperkzg.key_check(pa, vk(TAU), 1)
    pa.close()
    # the synthetic BN254 key (P_i = [k_i]G, no structure): not consistent with any verifier key, and still the key it was
    ck = CommitmentKey(BN.CURVE_BN254, synth.bases(BN.CURVE_BN254, n), n=n, device=True)
    for bad in malformed_keys():
        with pytest.raises(LurkHipError, match="the verifier key is"):
            hyperkzg.key_check(ck, bad, 1)
    assert hyperkzg.key_check(ck, vk(TAU), 1) is False
    s = synth.scalars(BN.FIELD_BN254_FR, 5, 0, n)
    torch.cuda.synchronize()
    assert aff(ck.commit_device(s, n)) == BN.dlog_checksum_np(BN.BN254, s.cpu().numpy().view(np.uint64))
    ck.close()
