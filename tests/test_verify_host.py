"""CPU-only: the host half of the verifiers.  lurk_hip_sumcheck_verify (SumcheckProof::verify) against oracle/spartan_ref.py: _sc_verify
without a device; the device verifiers fail loudly without one (no CPU fallback); the failed-check codes of the header and of the Python
wrapper are the same numbers."""
import os
import random
import re

import numpy as np
import pytest

from oracle import pyref as R
from oracle import spartan_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _poly_for(rng, q, degree, claim):
    """A round polynomial with p(0) + p(1) == claim."""
    co = [rng.randrange(q) for _ in range(degree + 1)]
    co[1] = (claim - 2 * co[0] - sum(co[2:])) % q
    return co


@pytest.mark.parametrize("field_id", [0, 1, 2])
@pytest.mark.parametrize("degree,rounds", [(2, 0), (2, 1), (3, 1), (2, 7), (3, 12)])
def test_sumcheck_verify_matches_the_oracle_without_a_device(field_id, degree, rounds):
    from lurk_beta_amd import sumcheck

    q = R.modulus(field_id)
    rng = random.Random(100 * field_id + 10 * degree + rounds)
    claim0 = rng.randrange(q)
    polys, rs, claim = [], [], claim0
    for _ in range(rounds):
        polys.append(_poly_for(rng, q, degree, claim))
        rs.append(rng.randrange(q))
        claim = R.unipoly_eval(q, polys[-1], rs[-1])
    want = S._sc_verify(q, claim0, polys, rs)
    assert want is not None and want == claim
    assert sumcheck.verify(field_id, degree, claim0, polys, rs) == want
    # every single coefficient changed: the round it belongs to fails (as in the oracle), except that the LAST round's polynomial is only
    # bound by p(0) + p(1) - the oracle decides, the library must agree
    for j in range(rounds):
        for k in range(degree + 1):
            bad = [list(p) for p in polys]
            bad[j][k] = (bad[j][k] + 1) % q
            o = S._sc_verify(q, claim0, bad, rs)
            assert sumcheck.verify(field_id, degree, claim0, bad, rs) == o
            if not (j == rounds - 1 and k >= 2):
                assert o is None
    if rounds:
        assert sumcheck.verify(field_id, degree, (claim0 + 1) % q, polys, rs) is None
        # not reduced: refused (ok = 0), whatever the oracle's reduction would make of it
        bad = [list(p) for p in polys]
        bad[0][0] += q
        assert bad[0][0] < 1 << 256 and sumcheck.verify(field_id, degree, claim0, bad, rs) is None
        assert sumcheck.verify(field_id, degree, claim0, polys, [rs[0] + q] + rs[1:]) is None
        assert sumcheck.verify(field_id, degree, claim0, polys[:-1], rs) is None  # (the wrapper: one challenge per polynomial)


def test_sumcheck_verify_refuses_bad_arguments():
    import ctypes

    from lurk_beta_amd import LurkHipError, _lib

    lib = _lib.load()
    z = np.zeros(4, dtype=np.uint64)
    ok = ctypes.c_int(7)
    for field_id, degree in ((3, 2), (0, 1), (0, 4)):
        assert lib.lurk_hip_sumcheck_verify(field_id, degree, 0, _lib.ptr(z), None, None, _lib.ptr(z), ctypes.byref(ok)) != 0
    with pytest.raises(LurkHipError):
        _lib.check(lib.lurk_hip_sumcheck_verify(0, 2, 1, _lib.ptr(z), None, None, _lib.ptr(z), ctypes.byref(ok)))
    assert lib.lurk_hip_sumcheck_verify(0, 2, 0, _lib.ptr(z), None, None, _lib.ptr(z), ctypes.byref(ok)) == 0 and ok.value == 1


def test_device_verifiers_fail_loudly_without_a_device():
    import ctypes

    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from lurk_beta_amd import LurkHipError, _lib

    lib = _lib.load()
    buf = np.zeros(64, dtype=np.uint64)
    acc, failed = ctypes.c_int(0), ctypes.c_int(0)
    p = _lib.ptr(buf)
    pf = _lib.SpartanProofStruct(*[buf.ctypes.data] * 10)
    bpf = _lib.SpartanBatchProofStruct(*[buf.ctypes.data] * 10)
    inst = (_lib.SpartanInstanceStruct * 1)()
    calls = [
        lambda: lib.lurk_hip_r1cs_sparse_mle_dev(p, p, 1, p, 1, p, None),
        lambda: lib.lurk_hip_ipa_s_vector_dev(1, p, 1, p, None),
        lambda: lib.lurk_hip_ipa_verify_dev(p, 2, p, p, None, p, p, p, p, ctypes.cast(lib.lurk_hip_keccak_ipa_challenge, ctypes.c_void_p), None, ctypes.byref(acc),
                                            ctypes.byref(failed), None),
        lambda: lib.lurk_hip_spartan_verify_dev(p, 2, 2, 0, p, p, p, p, p, p, b"x", 1, ctypes.byref(pf), ctypes.byref(acc), ctypes.byref(failed), None),
        lambda: lib.lurk_hip_spartan_verify_batch_dev(ctypes.cast(inst, ctypes.c_void_p), 1, p, p, b"x", 1, ctypes.byref(bpf), ctypes.byref(acc), ctypes.byref(failed), None),
    ]
    for call in calls:
        with pytest.raises(LurkHipError, match="no CPU fallback"):
            _lib.check(call())
        assert acc.value == 0


def test_failed_check_codes_are_the_headers():
    from lurk_beta_amd import spartan

    src = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+LURK_VERIFY_([A-Z]+)\s+(\d+)", src, flags=re.M)}
    assert codes == {"ACCEPTED": 0, "MALFORMED": 1, "OUTER": 2, "INNER": 3, "BATCH": 4, "OPENING": 5}
    for name, value in codes.items():
        assert getattr(spartan, "VERIFY_" + name) == value
    assert int(re.search(r"^#define\s+LURK_HIP_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1)) == 4
    from lurk_beta_amd import _lib

    assert _lib.load().lurk_hip_abi_version() == 4


def test_the_wrapper_rejects_what_it_cannot_marshal():
    """Wrong list lengths and values that do not fit 32 bytes never reach the library: False, failed check 1."""
    from lurk_beta_amd import spartan

    q = R.modulus(1)
    v = spartan.SpartanVerifier.__new__(spartan.SpartanVerifier)
    v.curve, v.q, v.sf, v.num_cons, v.num_vars, v.num_io, v.shape, v.last_failed_check = 0, q, 1, 4, 4, 1, None, None
    ck_c = np.zeros(8, dtype=np.uint64)
    good = dict(polys_outer=[[0] * 4] * 2, claims_outer=[0] * 3, eval_E=0, polys_inner=[[0] * 3] * 3, eval_W=0, polys_batch=[[0] * 3] * 2, evals_batch=[0, 0],
                ipa_L=[None, None], ipa_R=[None, None], ipa_a=0)
    cases = [dict(good, polys_outer=[[0] * 4]), dict(good, polys_inner=[[0] * 3] * 2), dict(good, polys_batch=[[0] * 2] * 2), dict(good, claims_outer=[0] * 2),
             dict(good, ipa_L=[None]), dict(good, ipa_R=[None] * 3), dict(good, evals_batch=[0]), dict(good, ipa_a=1 << 256), dict(good, eval_W=-1),
             dict(good, ipa_L=[(1, 1 << 255), None]), {k: w for k, w in good.items() if k != "eval_E"}]
    for proof in cases:
        v.last_failed_check = None
        assert v.verify([0], 1, np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64), proof, key=None, ck_c=ck_c) is False
        assert v.last_failed_check == spartan.VERIFY_MALFORMED
    assert v.verify([0, 0], 1, np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64), good, key=None, ck_c=ck_c) is False  # two X for num_io = 1
