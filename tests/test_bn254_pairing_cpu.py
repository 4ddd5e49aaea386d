"""CPU-only: the BN254 pairing check behind the KZG verifiers (include/lurk_hip.h, "the BN254 pairing check").  The library's host-only
entry points load without a GPU.  Every decision is compared with tests/bn254_pairing_ref.py, a Python-integer pairing built another way
(a flat Fp[w]/(w^12 - 18 w^6 + 82), the plain ate loop, one pow for the final exponentiation); lurk_hip_hyperkzg_verify is compared with
the trapdoor identity L == [tau]R of tests/hyperkzg_ref.py on honest and tampered reference proofs.  About thirty reference pairings of
~0.4 s each is the budget of this file."""
import copy
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bn254_pairing_ref as PR
from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = BN.BN254_R
G, H = BN.BN254.gen, PR.G2_GEN
TAU = 0x1F2E3D4C5B6A79881122334455667788990AABBCCDDEEFF00112233445566778 % Q
TAU_OTHER = (TAU + 1) % Q
ELLS = (1, 2, 3, 7)
RNG = random.Random(20254)
SCALARS = [RNG.randrange(1, Q) for _ in range(3)]

jac = lambda P: BN.jacobian(BN.BN254, P)
g1 = lambda k: BN.BN254.mul(k % Q, G)
g2 = lambda k: PR.g2_mul(k % Q, H)


def lib_check(pairs):
    """the library's decision on [(G1 point, G2 point)] given as the reference's Python values"""
    from lurk_beta_amd import pairing

    if not pairs:
        return pairing.pairing_check(np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 16), dtype=np.uint64))
    return pairing.pairing_check(np.stack([jac(p) for p, _ in pairs]), np.stack([pairing.g2_from_ints(q) for _, q in pairs]))


# ---- constants ---------------------------------------------------------------------------------------------------------------------------
def test_constants_follow_from_the_bn_parameter():
    from lurk_beta_amd import pairing

    assert PR.X == 0x44E992B44A6909F1
    assert (PR.P, PR.R) == (BN.BN254_P, BN.BN254_R) == (pairing.BN254_P, pairing.BN254_R)
    assert (PR.P**4 - PR.P**2 + 1) % PR.R == 0
    assert PR.B_TWIST == (0x2B149D40CEB8AAAE81BE18991BE06AC3B5B4C5E559DBEFA33267E6DC24A138E5, 0x009713B03AF0FED4CD2CAFADEED8FDF4A74FA084E52D1852E4A2BD0685C315D2)
    assert PR.g2_on_twist(H) and PR.g2_mul(PR.R, H) is None
    # the literals of the product's header: the loop count, the hard exponent, the generator
    hpp = open(os.path.join(ROOT, "lurk_beta_amd", "csrc", "bn254_pairing.hpp")).read()
    assert int(re.search(r"BN_X = (0x[0-9A-Fa-f]+)ull", hpp).group(1), 16) == PR.X
    assert (1 << 64) | int(re.search(r"ATE_LOOP_LOW = (0x[0-9A-Fa-f]+)ull", hpp).group(1), 16) == 6 * PR.X + 2
    hard = "".join(re.findall(r'"([0-9a-f]+)"', hpp[hpp.index("HARD_EXPONENT_HEX"):hpp.index("HARD_EXPONENT_LIMBS")]))
    assert int(hard, 16) == PR.HARD_EXPONENT and PR.HARD_EXPONENT.bit_length() == 761
    assert PR.HARD_EXPONENT.bit_length() <= 32 * int(re.search(r"HARD_EXPONENT_LIMBS = (\d+);", hpp).group(1))
    gen = [int(re.search(r'G2_GEN_%s_HEX = "([0-9a-f]{64})"' % c, hpp).group(1), 16) for c in ("X0", "X1", "Y0", "Y1")]
    assert ((gen[0], gen[1]), (gen[2], gen[3])) == H
    # ... and what the library computes from them
    assert pairing.g2_to_ints(pairing.g2_generator()) == H
    assert pairing.g2_to_ints(pairing.g2_mul(None, PR.R - 1)) == PR.g2_neg(H)


def test_header_constants_and_symbols_are_present_and_bound():
    from lurk_beta_amd import _lib, hyperkzg, pairing, spartan_kzg

    hdr = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    assert re.search(r"^#define LURK_HIP_ABI_VERSION 4$", hdr, flags=re.M)  # additions only
    assert re.search(r"^#define LURK_HYPERKZG_PAIRING 3\b", hdr, flags=re.M) and hyperkzg.PAIRING == 3
    assert re.search(r"^#define LURK_VERIFY_PAIRING \(6\)", hdr, flags=re.M) and spartan_kzg.VERIFY_PAIRING == 6
    lib = _lib.load()
    for name in ("lurk_hip_bn254_g2_mul", "lurk_hip_bn254_pairing_check", "lurk_hip_hyperkzg_verify", "lurk_hip_spartan_kzg_verify_pairing_dev",
                 "lurk_hip_spartan_kzg_verify_pairing_batch_dev", "lurk_hip_kzg_key_check_dev"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
    for mod, fns in ((pairing, ("g2_generator", "g2_mul", "pairing_check")), (hyperkzg, ("verify", "key_check", "trapdoor_vk"))):
        for fn in fns:
            assert callable(getattr(mod, fn)), fn
    assert callable(spartan_kzg.SpartanKzgVerifier.verify_pairing) and callable(spartan_kzg.BatchedSpartanKzgVerifier.verify_pairing)


# ---- G2 multiples ------------------------------------------------------------------------------------------------------------------------
def test_g2_mul_equals_the_reference():
    from lurk_beta_amd import pairing

    base_k = SCALARS[0]
    other = PR.g2_mul(base_k, H)
    for k in [0, 1, 2, PR.R - 1] + SCALARS:
        assert pairing.g2_to_ints(pairing.g2_mul(None, k)) == PR.g2_mul(k, H), k
        assert pairing.g2_to_ints(pairing.g2_mul(pairing.g2_from_ints(other), k)) == PR.g2_mul(k, other), k
    assert pairing.g2_to_ints(pairing.g2_mul(np.zeros(16, dtype=np.uint64), 5)) is None  # the identity stays the identity


# ---- decisions ---------------------------------------------------------------------------------------------------------------------------
def _decision_cases():
    a, b, c = SCALARS
    ab = a * b % Q
    cases = [
        ("scalar on G1 and G2", [(g1(a), g2(b)), (BN.BN254.neg(g1(ab)), H)], True),
        ("scalar on G1 and G2, off by one", [(g1(a), g2(b)), (BN.BN254.neg(g1(ab + 1)), H)], False),
        ("scalar moved to G2", [(g1(a), g2(b)), (BN.BN254.neg(G), g2(ab))], True),
        ("scalar moved to G2, off by one", [(g1(a), g2(b)), (BN.BN254.neg(G), g2(ab + 1))], False),
        ("three pairs", [(g1(a), g2(b)), (g1(c), g2(a)), (g1(-(ab + c * a)), H)], True),
        ("three pairs, off by one", [(g1(a), g2(b)), (g1(c), g2(a)), (g1(-(ab + c * a) + 1), H)], False),
        ("four pairs", [(g1(a), g2(b)), (g1(c), g2(a)), (g1(b), g2(c)), (G, g2(-(ab + c * a + b * c)))], True),
        ("four pairs, off by one", [(g1(a), g2(b)), (g1(c), g2(a)), (g1(b), g2(c)), (G, g2(-(ab + c * a + b * c) + 1))], False),
        ("identities on either side", [(None, g2(a)), (g1(b), None), (None, None)], True),
        ("identities beside a balanced product", [(None, g2(a)), (g1(a), g2(b)), (g1(b), None), (BN.BN254.neg(g1(ab)), H)], True),
        ("one non-trivial pair alone", [(g1(a), g2(b))], False),
        ("no pairs", [], True),
    ]
    return cases


@pytest.mark.parametrize("name,pairs,want", _decision_cases(), ids=[c[0] for c in _decision_cases()])
def test_the_library_and_the_reference_decide_alike(name, pairs, want):
    assert PR.pairing_product_is_one(pairs) is want
    assert lib_check(pairs) is want


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_a_valid_call_works_afterwards():
    import ctypes

    from lurk_beta_amd import LurkHipError, _lib, pairing

    a, b, _ = SCALARS
    good = [(g1(a), g2(b)), (BN.BN254.neg(g1(a * b)), H)]
    g1s = np.stack([jac(p) for p, _ in good])
    g2s = np.stack([pairing.g2_from_ints(q) for _, q in good])

    def works():
        assert pairing.pairing_check(g1s, g2s) is True

    # a G1 point off the curve (index 1)
    bad = g1s.copy()
    bad[1] = jac((1, 3))
    with pytest.raises(LurkHipError, match=r"G1 point 1 is neither the identity nor on the curve"):
        pairing.pairing_check(bad, g2s)
    works()
    # a G2 point off the twist (index 0)
    off = (H[0], PR.f2_add(H[1], (1, 0)))
    assert not PR.g2_on_twist(off)
    bad2 = g2s.copy()
    bad2[0] = pairing.g2_from_ints(off)
    with pytest.raises(LurkHipError, match=r"G2 point 0 is off the twist"):
        pairing.pairing_check(g1s, bad2)
    with pytest.raises(LurkHipError, match=r"off the twist"):
        pairing.g2_mul(pairing.g2_from_ints(off), 2)
    works()
    # a twist point outside the order-r subgroup (index 1): multiplied as it is, refused by the pairing check
    outside = PR.g2_outside_subgroup()
    assert PR.g2_on_twist(outside) and not PR.g2_in_subgroup(outside)
    assert pairing.g2_to_ints(pairing.g2_mul(pairing.g2_from_ints(outside), 3)) == PR.g2_mul(3, outside)
    bad2 = g2s.copy()
    bad2[1] = pairing.g2_from_ints(outside)
    with pytest.raises(LurkHipError, match=r"G2 point 1 is on the twist but outside the order-r subgroup"):
        pairing.pairing_check(g1s, bad2)
    works()
    # a coordinate that is not reduced
    bad2 = g2s.copy()
    bad2[0, :4] = np.uint64(0xFFFFFFFFFFFFFFFF)
    with pytest.raises(LurkHipError, match=r"G2 point 0 is off the twist"):
        pairing.pairing_check(g1s, bad2)
    # a scalar that is not below r
    for k in (PR.R, PR.R + 5, (1 << 256) - 1):
        with pytest.raises(LurkHipError, match=r"not reduced"):
            pairing.g2_mul(None, k)
    # NULLs
    lib, out, flag = _lib.load(), np.zeros(16, dtype=np.uint64), ctypes.c_int(7)
    k = np.array([1, 0, 0, 0], dtype=np.uint64)
    assert lib.lurk_hip_bn254_g2_mul(None, None, _lib.ptr(k)) != 0 and b"null" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_bn254_g2_mul(_lib.ptr(out), None, None) != 0 and b"null" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_bn254_pairing_check(2, _lib.ptr(g1s), _lib.ptr(g2s), None) != 0 and b"null" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_bn254_pairing_check(2, None, _lib.ptr(g2s), ctypes.byref(flag)) != 0 and b"null" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_bn254_pairing_check(2, _lib.ptr(g1s), None, ctypes.byref(flag)) != 0 and b"null" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_bn254_pairing_check(0, None, None, ctypes.byref(flag)) == 0 and flag.value == 1  # n = 0 needs no arrays
    works()


# ---- lurk_hip_hyperkzg_verify on reference proofs -----------------------------------------------------------------------------------------
def _instance(ell):
    """an honest reference proof, as tests/test_hyperkzg_cpu.py builds them"""
    rng = random.Random(1000 * ell)
    p0 = [rng.randrange(Q) for _ in range(1 << ell)]
    p0[0], p0[-1] = Q - 1, 1
    x = [rng.randrange(Q) for _ in range(ell)]
    tr = HK.Transcript()
    pf = HK.prove(TAU, p0, x, tr)
    return {"ell": ell, "c": HK.commit_trapdoor(TAU, p0), "x": x, "y": pf["y"], "com": pf["com"], "v": pf["v"], "w": pf["w"], "r": pf["r"], "q": pf["q"],
            "d": tr(2, pf["w"])}


_cache = {}


def instance(ell):
    if ell not in _cache:
        _cache[ell] = _instance(ell)
    return copy.deepcopy(_cache[ell])


def vk(tau):
    if ("vk", tau) not in _cache:
        from lurk_beta_amd import hyperkzg

        _cache[("vk", tau)] = hyperkzg.trapdoor_vk(tau)
    return _cache[("vk", tau)]


def lib_verify(a, tau_h):
    from lurk_beta_amd import hyperkzg

    com = np.stack([jac(P) for P in a["com"]]) if a["com"] else np.zeros((0, 12), dtype=np.uint64)
    return hyperkzg.verify(a["ell"], jac(a["c"]), a["x"], a["y"], com, a["v"], np.stack([jac(P) for P in a["w"]]), a["r"], a["q"], a["d"], tau_h)


def ref_decision(a, tau=TAU):
    """(accepted, code) as the header states it, the pairing replaced by the trapdoor identity"""
    L, R, ok, code = HK.pairing_inputs(a["ell"], a["c"], a["x"], a["y"], a["com"], a["v"], a["w"], a["r"], a["q"], a["d"])
    if not ok:
        return False, code
    return (True, HK.ACCEPTED) if HK.trapdoor_holds(tau, L, R) else (False, 3)


def test_trapdoor_vk_is_tau_times_the_generator():
    from lurk_beta_amd import pairing

    assert pairing.g2_to_ints(vk(TAU)) == PR.g2_mul(TAU, H)


@pytest.mark.parametrize("ell", ELLS)
def test_honest_reference_proofs_are_accepted(ell):
    a = instance(ell)
    assert ref_decision(a) == (True, HK.ACCEPTED)
    assert lib_verify(a, vk(TAU)) == (True, HK.ACCEPTED)
    # the verifier key of another tau: only the pairing equation can tell
    assert ref_decision(a, TAU_OTHER) == (False, 3)
    assert lib_verify(a, vk(TAU_OTHER)) == (False, 3)


def _tamper_cases(ell):
    bump = lambda v: (v + 1) % Q
    other = BN.BN254.mul(12345, G)
    cases = []
    for t in range(3):
        cases.append((f"v[{t}]", lambda a, t=t: a["v"][t].__setitem__(ell - 1, bump(a["v"][t][ell - 1]))))
    cases.append(("y", lambda a: a.__setitem__("y", bump(a["y"]))))
    cases.append(("x", lambda a: a["x"].__setitem__(0, bump(a["x"][0]))))
    cases.append(("r", lambda a: a.__setitem__("r", bump(a["r"]))))
    if ell > 1:  # (with a single polynomial there is no com, and q multiplies nothing)
        cases.append(("com", lambda a: a["com"].__setitem__(0, BN.BN254.add(a["com"][0], other))))
        cases.append(("q", lambda a: a.__setitem__("q", bump(a["q"]))))
    cases.append(("C", lambda a: a.__setitem__("c", BN.BN254.add(a["c"], other))))
    for t in range(3):
        cases.append((f"W[{t}]", lambda a, t=t: a["w"].__setitem__(t, BN.BN254.add(a["w"][t], other))))
    return cases


@pytest.mark.parametrize("ell", ELLS)
def test_every_tampering_keeps_its_code_or_fails_the_pairing(ell):
    """The library's (accepted, code) is the reference's for every class of tampering: what a scalar check catches today keeps
    LURK_HYPERKZG_FOLD, what only L != [tau]R catches is LURK_HYPERKZG_PAIRING, nothing is accepted."""
    from lurk_beta_amd import hyperkzg

    assert (hyperkzg.ACCEPTED, hyperkzg.MALFORMED, hyperkzg.FOLD, hyperkzg.PAIRING) == (HK.ACCEPTED, HK.MALFORMED, HK.FOLD, 3)
    codes = {}
    for name, f in _tamper_cases(ell):
        a = instance(ell)
        f(a)
        want = ref_decision(a)
        assert want[0] is False, name
        assert lib_verify(a, vk(TAU)) == want, name
        codes[name] = want[1]
    assert all(codes[k] == HK.FOLD for k in ("v[0]", "v[1]", "y", "x", "r")), codes
    assert all(codes[k] == hyperkzg.PAIRING for k in codes if k in ("C", "W[0]", "W[1]", "W[2]", "com", "q")), codes
    assert codes["v[2]"] in (HK.FOLD, hyperkzg.PAIRING)  # (v[2][ell-1] enters a scalar check only when ell > 1)


@pytest.mark.parametrize("ell", (1, 3))
def test_a_changed_d_is_caught_by_the_pairing_where_d_matters(ell):
    """d batches three equations an honest proof satisfies one by one: on an HONEST proof another d moves L and R and the proof stays
    valid.  Where d matters is a forgery whose errors in W_0 and W_1 cancel under one d - built with the trapdoor,
    (u_0 - tau) a + d (u_1 - tau) b = 0: it verifies under that d and fails the pairing under any other."""
    a = instance(ell)
    moved = copy.deepcopy(a)
    moved["d"] = (a["d"] + 1) % Q
    assert ref_decision(moved) == (True, HK.ACCEPTED) and lib_verify(moved, vk(TAU)) == (True, HK.ACCEPTED)
    u0, u1, d = a["r"], (-a["r"]) % Q, a["d"]
    ea = 0x1234567
    eb = (-(u0 - TAU) * ea * pow(d * (u1 - TAU), -1, Q)) % Q
    forged = copy.deepcopy(a)
    forged["w"][0] = BN.BN254.add(a["w"][0], g1(ea))
    forged["w"][1] = BN.BN254.add(a["w"][1], g1(eb))
    assert ref_decision(forged) == (True, HK.ACCEPTED) and lib_verify(forged, vk(TAU)) == (True, HK.ACCEPTED)
    forged["d"] = (d + 1) % Q
    assert ref_decision(forged) == (False, 3) and lib_verify(forged, vk(TAU)) == (False, 3)


def test_malformed_input_and_malformed_verifier_keys():
    from lurk_beta_amd import LurkHipError, hyperkzg, pairing

    for name, f in (("y", lambda a: a.__setitem__("y", Q)), ("r", lambda a: a.__setitem__("r", 0)), ("W", lambda a: a["w"].__setitem__(2, (1, 3))),
                    ("com", lambda a: a["com"].__setitem__(0, (5, 7)))):
        a = instance(2)
        f(a)
        assert ref_decision(a) == (False, HK.MALFORMED), name
        assert lib_verify(a, vk(TAU)) == (False, HK.MALFORMED), name
    a = instance(2)
    outside = PR.g2_outside_subgroup()
    off = (H[0], PR.f2_add(H[1], (1, 0)))
    for name, key in (("off the twist", pairing.g2_from_ints(off)), ("outside the subgroup", pairing.g2_from_ints(outside)), ("the identity", np.zeros(16, dtype=np.uint64))):
        assert lib_verify(a, key) == (False, HK.MALFORMED), name
    # ... whatever the proof: a failed scalar check under a malformed key is malformed input too
    a["y"] = (a["y"] + 1) % Q
    assert lib_verify(a, np.zeros(16, dtype=np.uint64)) == (False, HK.MALFORMED)
    assert lib_verify(instance(2), vk(TAU)) == (True, HK.ACCEPTED)
    # other curves are refused by name
    z12, z4 = np.zeros(12, dtype=np.uint64), [0]
    for curve, cname in ((0, "Pallas"), (1, "Vesta"), (3, "Grumpkin")):
        with pytest.raises(LurkHipError, match="lurk_hip_hyperkzg_verify.*" + cname):
            hyperkzg.verify(1, z12, z4, 0, np.zeros((0, 12), dtype=np.uint64), [z4, z4, z4], np.zeros((3, 12), dtype=np.uint64), 1, 0, 0, vk(TAU), curve=curve)


# ---- the header under the sanitizers, as a program of its own ----------------------------------------------------------------------------------
def test_host_program_passes_under_address_and_undefined_sanitizers(tmp_path):
    """tests/host_pairing/main.cpp: bn254_pairing.hpp compiled by plain g++ with -fsanitize=address,undefined into an executable of its
    own with the sanitizer runtimes linked in (it needs nothing from the environment it is started in), running a fixed list of tower, group-law, bilinearity and rejection checks."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "host_pairing")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        os.path.join(ROOT, "tests", "host_pairing", "main.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert re.search(r"host_pairing: \d+ checks passed", r.stdout), r.stdout[-500:]
