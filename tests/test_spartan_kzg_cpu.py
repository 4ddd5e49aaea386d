"""CPU: the Python-integer reference of the compressing SNARK on BN254 G1 (tests/spartan_kzg_ref.py) proves and verifies, reports
tampering at the right check, and the header declares the new entry points under the unchanged ABI revision."""
import copy
import os
import re

import pytest

from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK
from tests import spartan_kzg_ref as K

Q = K.Q
TAU = 0x2B0F3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % Q
SHAPES = [(2, 2, 1), (8, 16, 2), (16, 8, 2), (16, 16, 2)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_ref = {}


def reference(nc, nv, nio, folded):
    k = (nc, nv, nio, folded)
    if k not in _ref:
        it = K.make_instance(TAU, nc, nv, nio, 11 + nc + nv, folded)
        _ref[k] = (it, K.prove(TAU, it["mats"], nc, nv, it["X"], it["comm_W"], it["comm_E"], it["u"], it["W"], it["E"]))
    return _ref[k]


def verify(it, pf, **over):
    a = dict(it, **over)
    return K.verify(a["mats"], a["num_cons"], a["num_vars"], a["X"], a["comm_W"], a["comm_E"], a["u"], pf)


@pytest.mark.parametrize("folded", [False, True], ids=["strict", "relaxed"])
@pytest.mark.parametrize("nc,nv,nio", SHAPES)
def test_reference_proves_and_verifies(nc, nv, nio, folded):
    it, pf = reference(nc, nv, nio, folded)
    assert K.is_sat(it["mats"], it["X"], it["u"], it["W"], it["E"])
    assert (it["u"] == 1 and not any(it["E"])) if not folded else (it["u"] != 1 and any(it["E"]))
    ell = max(nc, nv).bit_length() - 1
    assert len(pf["kzg_com"]) == ell - 1 and len(pf["kzg_v"]) == 3 * ell and len(pf["kzg_w"]) == 3
    L, R, ok, code = verify(it, pf)
    assert ok and code == K.ACCEPTED and R is not None and HK.trapdoor_holds(TAU, L, R)
    # a wrong statement is rejected
    assert not verify(it, pf, u=(it["u"] + 1) % Q)[2]
    assert not verify(it, pf, X=[(it["X"][0] + 1) % Q] + it["X"][1:])[2]


def test_tampering_is_reported_at_the_right_check():
    it, pf = reference(8, 16, 2, True)
    bump = lambda v: (v + 1) % Q

    def code(mutate):
        bad = copy.deepcopy(pf)
        mutate(bad)
        L, R, ok, c = verify(it, bad)
        assert not ok and L is None and R is None
        return c

    def at(name, *idx):
        def m(bad):
            tgt = bad
            for i in (name,) + idx[:-1]:
                tgt = tgt[i]
            tgt[idx[-1]] = bump(tgt[idx[-1]])
        return m if idx else (lambda bad: bad.__setitem__(name, bump(bad[name])))

    assert code(at("polys_outer", 1, 2)) == K.OUTER
    assert code(at("claims_outer", 0)) == K.OUTER
    assert code(at("eval_E")) == K.OUTER
    assert code(at("polys_inner", 0, 1)) == K.INNER
    assert code(at("eval_W")) == K.INNER
    assert code(at("polys_batch", 2, 0)) == K.BATCH
    assert code(at("evals_batch", 1)) == K.BATCH
    assert code(at("kzg_v", 0)) == K.OPENING
    # an unreduced scalar, a point off the curve
    assert code(lambda bad: bad["kzg_v"].__setitem__(1, bad["kzg_v"][1] + Q)) == K.MALFORMED
    assert code(lambda bad: bad["kzg_w"].__setitem__(2, (bad["kzg_w"][2][0], (bad["kzg_w"][2][1] + 1) % BN.BN254_P))) == K.MALFORMED


def test_a_replaced_commitment_of_the_opening():
    """kzg_w[1] replaced by another curve point: only d depends on the W_t, every scalar check still holds - accepted so far, and the
    pairing (here the trapdoor identity) rejects.  kzg_com[0] replaced: com is absorbed BEFORE r is squeezed, so r moves away from the
    point the v were evaluated at and the scalar checks - each one linear in r with a non-zero slope - fail: OPENING.  (With a
    caller-supplied r, as in tests/test_gpu_hyperkzg.py, a replaced com is accepted so far; bound to the transcript it cannot be.)"""
    it, pf = reference(8, 16, 2, True)
    other = lambda pt: BN.BN254.add(pt, BN.BN254.gen)
    bad = copy.deepcopy(pf)
    bad["kzg_w"][1] = other(bad["kzg_w"][1])
    L, R, ok, code = verify(it, bad)
    assert ok and code == K.ACCEPTED and not HK.trapdoor_holds(TAU, L, R)
    bad = copy.deepcopy(pf)
    bad["kzg_com"][0] = other(bad["kzg_com"][0])
    assert verify(it, bad)[2:] == (False, K.OPENING)
    # v[2][0] = P_0(r^2) enters no scalar check, only b_2 and through it L: accepted so far, the pairing rejects
    bad = copy.deepcopy(pf)
    ell = 4
    bad["kzg_v"][2 * ell] = (bad["kzg_v"][2 * ell] + 1) % Q
    L, R, ok, code = verify(it, bad)
    assert ok and not HK.trapdoor_holds(TAU, L, R)


@pytest.mark.parametrize("sizes", [[(16, 64), (64, 32), (8, 16)], [(8, 16)]], ids=["three", "one"])
def test_batched_reference(sizes):
    insts = [K.make_instance(TAU, nc, nv, 2, 23 + i, i % 2 == 1) for i, (nc, nv) in enumerate(sizes)]
    pf = K.prove_batched(TAU, insts)
    L, R, ok, code = K.verify_batched(insts, pf)
    assert ok and code == K.ACCEPTED and HK.trapdoor_holds(TAU, L, R)
    for name, want in (("evals_E", K.OUTER), ("evals_W", K.INNER), ("evals_batch", K.BATCH), ("kzg_v", K.OPENING)):
        bad = copy.deepcopy(pf)
        bad[name][0] = (bad[name][0] + 1) % Q
        assert K.verify_batched(insts, bad)[2:] == (False, want), name
    swapped = copy.deepcopy(insts)
    swapped[0]["u"] = (swapped[0]["u"] + 1) % Q
    assert not K.verify_batched(swapped, pf)[2]


def test_header_declares_the_new_entry_points_under_abi_4():
    with open(os.path.join(ROOT, "include", "lurk_hip.h")) as f:
        h = f.read()
    for sym in ("lurk_hip_fold_padded_dev", "lurk_hip_spartan_kzg_prove_dev", "lurk_hip_spartan_kzg_prove_batch_dev", "lurk_hip_spartan_kzg_verify_dev",
                "lurk_hip_spartan_kzg_verify_batch_dev"):
        assert re.search(r"^int " + sym + r"\(", h, re.M), sym
    for struct in ("lurk_hip_spartan_kzg_proof", "lurk_hip_spartan_kzg_batch_proof"):
        assert re.search(r"\}\s*" + struct + ";", h), struct
    assert re.search(r"^#define LURK_HIP_ABI_VERSION 4$", h, re.M)
