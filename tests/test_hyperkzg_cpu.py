"""CPU-only: the HyperKZG reference (tests/hyperkzg_ref.py) proves and verifies, the library's host-only verifier up to the pairing
(lurk_hip_hyperkzg_pairing_inputs) computes the same L, R and flag as the reference, the trapdoor identity L == [tau]R holds for honest
proofs and every class of tampering is caught - by a scalar check with its own code, or by L != [tau]R."""
import copy
import os
import random
import re

import numpy as np
import pytest

from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = HK.Q
TAU = 0x1F2E3D4C5B6A79881122334455667788990AABBCCDDEEFF00112233445566778 % Q
ELLS = (1, 2, 3, 7)


def _instance(ell, seed=0):
    """an honest reference proof: everything pairing_inputs takes, as Python values"""
    rng = random.Random(1000 * ell + seed)
    n = 1 << ell
    p0 = [rng.randrange(Q) for _ in range(n)]
    p0[0], p0[-1] = Q - 1, 1
    x = [rng.randrange(Q) for _ in range(ell)]
    tr = HK.Transcript()
    pf = HK.prove(TAU, p0, x, tr)
    c = HK.commit_trapdoor(TAU, p0)
    d = tr(2, pf["w"])
    return {"ell": ell, "c": c, "x": x, "y": pf["y"], "com": pf["com"], "v": pf["v"], "w": pf["w"], "r": pf["r"], "q": pf["q"], "d": d}


_cache = {}


def instance(ell):
    if ell not in _cache:
        _cache[ell] = _instance(ell)
    return copy.deepcopy(_cache[ell])


def ref_verify(a):
    return HK.pairing_inputs(a["ell"], a["c"], a["x"], a["y"], a["com"], a["v"], a["w"], a["r"], a["q"], a["d"])


def lib_verify(a):
    from lurk_beta_amd import hyperkzg, point_to_affine

    jac = lambda P: BN.jacobian(BN.BN254, P)
    com = np.stack([jac(P) for P in a["com"]]) if a["com"] else np.zeros((0, 12), dtype=np.uint64)
    L, R, ok, code = hyperkzg.pairing_inputs(a["ell"], jac(a["c"]), a["x"], a["y"], com, a["v"], np.stack([jac(P) for P in a["w"]]), a["r"], a["q"], a["d"])
    return BN.from_xy(point_to_affine(BN.CURVE_BN254, L)), BN.from_xy(point_to_affine(BN.CURVE_BN254, R)), ok, code


@pytest.mark.parametrize("ell", ELLS)
def test_reference_proof_is_accepted_and_the_library_agrees(ell):
    a = instance(ell)
    # the evaluation the proof claims is the multilinear extension at x (x_0 <-> the most significant index bit)
    rng = random.Random(1000 * ell)
    p0 = [rng.randrange(Q) for _ in range(1 << ell)]
    p0[0], p0[-1] = Q - 1, 1
    want = 0
    for idx, val in enumerate(p0):
        w = val
        for j in range(ell):
            bit = (idx >> (ell - 1 - j)) & 1
            w = w * (a["x"][j] if bit else 1 - a["x"][j]) % Q
        want = (want + w) % Q
    assert a["y"] == want
    L, R, ok, code = ref_verify(a)
    assert ok and code == HK.ACCEPTED and HK.trapdoor_holds(TAU, L, R)
    assert R is not None
    gL, gR, gok, gcode = lib_verify(a)
    assert (gL, gR, gok, gcode) == (L, R, True, HK.ACCEPTED)
    assert HK.trapdoor_holds(TAU, gL, gR)


def _tamper_cases(ell):
    bump = lambda v: (v + 1) % Q
    other = BN.BN254.mul(12345, BN.BN254.gen)
    cases = []
    for t in range(3):
        def f(a, t=t):
            a["v"][t][ell - 1] = bump(a["v"][t][ell - 1])
        cases.append((f"v[{t}]", f))
    cases.append(("y", lambda a: a.__setitem__("y", bump(a["y"]))))
    if ell > 1:
        cases.append(("com", lambda a: a["com"].__setitem__(0, BN.BN254.add(a["com"][0], other))))
    cases.append(("C", lambda a: a.__setitem__("c", BN.BN254.add(a["c"], other))))
    for t in range(3):
        def g(a, t=t):
            a["w"][t] = BN.BN254.add(a["w"][t], other)
        cases.append((f"W[{t}]", g))
    cases.append(("x", lambda a: a["x"].__setitem__(0, bump(a["x"][0]))))
    cases.append(("r", lambda a: a.__setitem__("r", bump(a["r"]))))
    if ell > 1:  # (with a single polynomial q multiplies nothing: B = P_0 whatever q is)
        cases.append(("q", lambda a: a.__setitem__("q", bump(a["q"]))))
    return cases


@pytest.mark.parametrize("ell", (1, 3))
def test_every_class_of_tampering_is_caught(ell):
    for name, f in _tamper_cases(ell):
        a = instance(ell)
        f(a)
        L, R, ok, code = ref_verify(a)
        gL, gR, gok, gcode = lib_verify(a)
        assert (gok, gcode) == (ok, code), name
        if ok:
            assert code == HK.ACCEPTED and (gL, gR) == (L, R), name
            assert not HK.trapdoor_holds(TAU, gL, gR), f"{name}: a tampered proof passed the trapdoor identity"
        else:  # the flag is never "accepted" on a failed scalar check, and nothing is handed to the pairing
            assert code == HK.FOLD and (gL, gR) == (None, None), name
    # which classes the scalar checks alone catch: the evaluations, y, x and r enter them; com, C, W, q and d only the group equation
    caught = {name for name, f in _tamper_cases(ell) for a in [instance(ell)] if (f(a), ref_verify(a))[1][3] == HK.FOLD}
    assert {"v[0]", "v[1]", "y", "x", "r"} <= caught
    assert not caught & {"C", "W[0]", "W[1]", "W[2]", "q", "com"}


@pytest.mark.parametrize("ell", (1, 3))
def test_the_batching_challenge_d_binds_the_three_openings(ell):
    """d only batches three equations that an honest proof satisfies one by one, so changing d ALONE cannot break L == [tau]R (it moves L and
    R, which the library must follow).  What d is for: a forgery whose errors in W_0 and W_1 cancel under one d - built here with the
    trapdoor, (u_0 - tau) a + d (u_1 - tau) b = 0 - passes under that d and is caught under any other."""
    a = instance(ell)
    L0, R0, ok, _ = ref_verify(a)
    moved = copy.deepcopy(a)
    moved["d"] = (a["d"] + 1) % Q
    L1, R1, ok1, _ = ref_verify(moved)
    assert ok and ok1 and (L1, R1) != (L0, R0) and HK.trapdoor_holds(TAU, L1, R1)
    assert lib_verify(moved) == (L1, R1, True, HK.ACCEPTED)
    u0, u1, d = a["r"], (-a["r"]) % Q, a["d"]
    ea = 0x1234567
    eb = (-(u0 - TAU) * ea * pow(d * (u1 - TAU), -1, Q)) % Q
    forged = copy.deepcopy(a)
    forged["w"][0] = BN.BN254.add(a["w"][0], BN.BN254.mul(ea, BN.BN254.gen))
    forged["w"][1] = BN.BN254.add(a["w"][1], BN.BN254.mul(eb, BN.BN254.gen))
    gL, gR, gok, _ = lib_verify(forged)
    assert gok and HK.trapdoor_holds(TAU, gL, gR)  # tuned to this d ...
    forged["d"] = (d + 1) % Q
    gL, gR, gok, _ = lib_verify(forged)
    assert gok and not HK.trapdoor_holds(TAU, gL, gR)  # ... and caught under another


def test_malformed_input_is_rejected_before_any_arithmetic():
    for name, f in (("y", lambda a: a.__setitem__("y", Q)), ("r", lambda a: a.__setitem__("r", 0)), ("v", lambda a: a["v"][1].__setitem__(0, Q + 5)),
                    ("W", lambda a: a["w"].__setitem__(2, (1, 3))), ("com", lambda a: a["com"].__setitem__(0, (5, 7))), ("d", lambda a: a.__setitem__("d", (1 << 256) - 1))):
        a = instance(2)
        f(a)
        assert ref_verify(a)[2:] == (False, HK.MALFORMED), name
        assert lib_verify(a) == (None, None, False, HK.MALFORMED), name


def test_other_curves_are_refused_by_name():
    from lurk_beta_amd import LurkHipError, hyperkzg

    z12, z4 = np.zeros(12, dtype=np.uint64), [0]
    for curve, name in ((0, "Pallas"), (1, "Vesta"), (3, "Grumpkin")):
        with pytest.raises(LurkHipError, match=name):
            hyperkzg.pairing_inputs(1, z12, z4, 0, np.zeros((0, 12), dtype=np.uint64), [z4, z4, z4], np.zeros((3, 12), dtype=np.uint64), 1, 0, 0, curve=curve)


def test_reference_primitives_are_consistent():
    rng = random.Random(5)
    for n in (1, 2, 5, 16):
        c = [rng.randrange(Q) for _ in range(n)]
        u = rng.randrange(Q)
        h, rem = HK.div_linear(c, u)
        assert rem == HK.poly_eval(c, u) and len(h) == n - 1
        back = [0] * n
        for j, a in enumerate(h):  # h (X - u) + rem
            back[j + 1] = (back[j + 1] + a) % Q
            back[j] = (back[j] - u * a) % Q
        back[0] = (back[0] + rem) % Q
        assert back == c
    assert HK.fold_pairs([1, 2, 3], 5) == [(1 + 5 * 1) % Q, (3 - 15) % Q]


def test_header_constants_and_symbols_are_present_and_bound():
    from lurk_beta_amd import _lib, hyperkzg

    hdr = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    consts = dict(re.findall(r"^#define\s+(LURK_HYPERKZG_[A-Z_]+)\s+(\d+)\s*$", hdr, flags=re.M))
    assert consts == {"LURK_HYPERKZG_ACCEPTED": "0", "LURK_HYPERKZG_MALFORMED": "1", "LURK_HYPERKZG_FOLD": "2"}
    assert (hyperkzg.ACCEPTED, hyperkzg.MALFORMED, hyperkzg.FOLD) == (HK.ACCEPTED, HK.MALFORMED, HK.FOLD) == (0, 1, 2)
    assert re.search(r"^#define LURK_HIP_ABI_VERSION 4$", hdr, flags=re.M)  # additions only
    lib = _lib.load()
    for name in ("lurk_hip_mle_fold_pairs_dev", "lurk_hip_poly_eval_dev", "lurk_hip_poly_div_linear_dev", "lurk_hip_synth_kzg_bases_dev",
                 "lurk_hip_hyperkzg_prove_dev", "lurk_hip_hyperkzg_pairing_inputs"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "lurk_hip_hyperkzg_challenge_fn" in hdr
    for fn in ("prove", "pairing_inputs", "trapdoor_key"):
        assert callable(getattr(hyperkzg, fn))
