"""The library's verifiers (lurk_hip_spartan_verify_dev / _verify_batch_dev and their building blocks) against the CPU oracle
(oracle/spartan_fast.py: verify / verify_batched, oracle/oracle.c): same decision on the oracle prover's proofs and on the library
prover's, on every single-element change of proof and statement - at the stage the oracle's own control flow returns from - and on
malformed input, which the oracle has no notion of.  Reference: CompressedSNARK::verify, /root/reference/src/proof/nova.rs:358-373,
supernova.rs:304-316; the protocol is the repository's own (oracle/spartan_ref.py)."""
import ctypes
import inspect
import re
import threading

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from oracle import spartan_fast as SF
from oracle import spartan_ref as S
from tests.test_oracle_spartan import _to_arrays, product_instance

pytestmark = pytest.mark.gpu

CURVES = [("pallas", 0), ("vesta", 1)]


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _staged(fn, returns):
    """A copy of an oracle verifier whose `return False` statements return the number of the check they belong to (in source order) and
    whose final comparison returns 0 / 5; `_label_suffix` (a global of the copy) is appended to the transcript's label."""
    src = inspect.getsource(fn)
    assert src.count("return False") == len(returns), "the oracle's control flow changed: re-derive the stages"
    it = iter(returns)
    src = re.sub(r"return False", lambda m: f"return {next(it)}", src)
    src, n = re.subn(r"return (P == [^\n]+)", r"return 0 if (\1) else 5", src)
    assert n == 1
    src, n = re.subn(r"tr = Transcript\(([^\n]+)\)\n", r"tr = Transcript(\1 + _label_suffix)\n", src, count=1)
    assert n == 1
    ns = dict(vars(SF))
    ns["_label_suffix"] = b""
    exec(compile(src, "<staged oracle>", "exec"), ns)
    return ns


# verify: round counts (1), outer (2), inner (3), batching (4), the number of opening rounds (1);  verify_batched: two length checks first
_SV = _staged(SF.verify, [1, 2, 3, 4, 1])
_SVB = _staged(SF.verify_batched, [1, 1, 2, 3, 4, 1])


def staged_verify(*a, label_suffix=b""):
    _SV["_label_suffix"] = label_suffix
    try:
        return _SV["verify"](*a)
    finally:
        _SV["_label_suffix"] = b""


def staged_verify_batched(*a):
    return _SVB["verify_batched"](*a)


def _instance(cn, c, nc, nv, folded, seed=9, nio=2):
    sf = 1 - c
    mats, X, u, W, E = product_instance(cn, nc, nv, nio, seed, folded)
    m_arr, W_arr, E_arr = _to_arrays(mats, X, W, E)
    N = max(nc, nv)
    B = C.synth_bases(c, N + 1)
    comm_W, comm_E = SF._aff(c, SF._commit(c, B, W_arr)), SF._aff(c, SF._commit(c, B, E_arr))
    return dict(c=c, sf=sf, q=R.CURVES[cn]["order"], mats=m_arr, nc=nc, nv=nv, N=N, X=X, u=u, W=W_arr, E=E_arr, B=B, comm_W=comm_W, comm_E=comm_E)


def _mont_mats(sf, mats):
    return [(M[0], M[1], C.to_mont(sf, M[2])) for M in mats]


def _oracle_args(I, **over):
    a = dict(I, **over)
    return (a["c"], a["mats"], a["nc"], a["nv"], a["X"], a["B"], a["comm_W"], a["comm_E"], a["u"])


# ---- 1. accepts what the oracle accepts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn,c", CURVES)
@pytest.mark.parametrize("nc,nv,folded", [(8, 16, False), (32, 64, True), (64, 128, True)])
def test_accepts_the_oracles_and_the_librarys_proofs(hip, cn, c, nc, nv, folded):
    """A relaxed instance (folded: u != 1, E != 0) and a strict one (comm_E = the identity); plain and table key."""
    from lurk_beta_amd import CommitmentKey
    from lurk_beta_amd.spartan import SpartanProver, SpartanVerifier

    I = _instance(cn, c, nc, nv, folded)
    if not folded:
        assert I["comm_E"] is None and I["u"] == 1
    else:
        assert I["comm_E"] is not None and I["u"] != 1
    N, B, q = I["N"], I["B"], I["q"]
    want = SF.prove(c, I["mats"], nc, nv, I["X"], B, I["comm_W"], I["comm_E"], I["u"], I["W"], I["E"])
    assert SF.verify(*_oracle_args(I), want)
    prover = SpartanProver(c, q, _mont_mats(I["sf"], I["mats"]), nc, nv, len(I["X"]))
    verifier = SpartanVerifier.from_shape(prover.shape, c, q)
    own = SpartanVerifier(c, q, _mont_mats(I["sf"], I["mats"]), nc, nv, len(I["X"]))
    for key in (CommitmentKey(c, B[:N]), CommitmentKey(c, B[:N], precompute=True)):
        cw, ce = key.commit(I["W"]), key.commit(I["E"])
        got = prover.prove(I["X"], I["u"], _dev(C.to_mont(I["sf"], I["W"])), _dev(C.to_mont(I["sf"], I["E"])), _dev(B), cw, ce, key=key, in_library=True)
        assert got == want
        for v in (verifier, own):
            for proof in (want, got):
                assert v.verify(I["X"], I["u"], cw, ce, proof, key, d_ck=_dev(B)) is True and v.last_failed_check == 0
                assert v.verify(I["X"], I["u"], I["comm_W"], I["comm_E"], proof, key, d_ck=B) is True  # commitments as the oracle carries them
        bad_x = [(I["X"][0] + 1) % q] + I["X"][1:]
        assert verifier.verify(bad_x, I["u"], cw, ce, got, key, d_ck=B) is False and not SF.verify(*_oracle_args(I, X=bad_x), got)
        assert verifier.last_failed_check == staged_verify(*_oracle_args(I, X=bad_x), got)
        key.close()
    own.close()
    prover.close()


@pytest.mark.parametrize("cn,c,log_n", [("pallas", 0, 14), ("vesta", 1, 14), ("pallas", 0, 16)])
def test_accepts_at_2_14_and_2_16(hip, cn, c, log_n):
    from lurk_beta_amd import CommitmentKey
    from lurk_beta_amd.spartan import SpartanProver, SpartanVerifier

    sf, q = 1 - c, R.CURVES[cn]["order"]
    nc = nv = 1 << log_n
    A, Bm, Cm, W, X = SF.synth_product_instance(sf, nc, nv, 2, seed=log_n + c)
    E = np.zeros((nc, 4), dtype=np.uint64)
    B = C.synth_bases(c, nc + 1)
    comm_W = SF._aff(c, SF._commit(c, B, W))
    want = SF.prove(c, (A, Bm, Cm), nc, nv, X, B, comm_W, None, 1, W, E)
    prover = SpartanProver(c, q, _mont_mats(sf, (A, Bm, Cm)), nc, nv, len(X))
    verifier = SpartanVerifier.from_shape(prover.shape, c, q)
    bad_x = [(X[0] + 1) % q] + X[1:]
    stages = []
    for key in (CommitmentKey(c, B[:nc]), CommitmentKey(c, B[:nc], precompute=True)):
        cw, ce = key.commit(W), key.commit(E)
        got = prover.prove(X, 1, _dev(C.to_mont(sf, W)), _dev(E), _dev(B), cw, ce, key=key, in_library=True)
        for proof in (want, got):
            assert verifier.verify(X, 1, cw, ce, proof, key, d_ck=B) is True and verifier.last_failed_check == 0
        assert verifier.verify(bad_x, 1, cw, ce, got, key, d_ck=B) is False
        stages.append(verifier.last_failed_check)
        key.close()
    assert SF.verify(c, (A, Bm, Cm), nc, nv, X, B, comm_W, None, 1, want)
    o = staged_verify(c, (A, Bm, Cm), nc, nv, bad_x, B, comm_W, None, 1, want)
    assert o != 0 and stages == [o, o]
    prover.close()


# ---- 2. rejects what the oracle rejects, at the same stage -----------------------------------------------------------------------------
def _proof_changes(I, proof):
    """(name, changed proof, the stage the changed element first enters) for every single element of the proof."""
    q, c = I["q"], I["c"]
    other = lambda pt: SF._aff(c, C.jac_add(c, _jac(c, pt), _jac(c, C.affine_to_ints(c, I["B"][3:4])[0])))  # the point plus a key point
    out = []

    def put(path, stage):
        p = {k: ([list(x) if isinstance(x, list) else x for x in v] if isinstance(v, list) else v) for k, v in proof.items()}
        tgt, key = p, path[0]
        for k in path[1:]:
            tgt, key = tgt[key], k
        tgt[key] = other(tgt[key]) if path[0] in ("ipa_L", "ipa_R") else (tgt[key] + 1) % q
        out.append(("/".join(map(str, path)), p, stage))

    for name, stage in (("polys_outer", 2), ("polys_inner", 3), ("polys_batch", 4)):
        for j, poly in enumerate(proof[name]):
            for k in range(len(poly)):
                put((name, j, k), stage)
    for k in range(3):
        put(("claims_outer", k), 2)
    put(("eval_E",), 2)
    put(("eval_W",), 3)
    for k in range(2):
        put(("evals_batch", k), 4)
    for name in ("ipa_L", "ipa_R"):
        for j in range(len(proof[name])):
            put((name, j), 5)
    put(("ipa_a",), 5)
    return out


def _jac(c, aff):
    """affine integers / None -> Jacobian Montgomery limbs (the oracle's layout)"""
    if aff is None:
        return np.zeros(12, dtype=np.uint64)
    p = R.modulus(c)  # the base field of curve c has the id c
    Rm = (1 << 256) % p
    return C.ints_to_limbs([aff[0] * Rm % p, aff[1] * Rm % p, Rm]).reshape(12)


@pytest.mark.parametrize("cn,c", CURVES)
def test_rejects_every_single_element_change_at_the_oracles_stage(hip, cn, c):
    from lurk_beta_amd import CommitmentKey
    from lurk_beta_amd.spartan import SpartanVerifier

    nc, nv = 32, 64
    I = _instance(cn, c, nc, nv, True)
    q, sf, N, B = I["q"], I["sf"], I["N"], I["B"]
    proof = SF.prove(c, I["mats"], nc, nv, I["X"], B, I["comm_W"], I["comm_E"], I["u"], I["W"], I["E"])
    key = CommitmentKey(c, B[:N])
    v = SpartanVerifier(c, q, _mont_mats(sf, I["mats"]), nc, nv, len(I["X"]))
    lib = lambda Iv, pf, vv=v, kk=key, **kw: (vv.verify(Iv["X"], Iv["u"], Iv["comm_W"], Iv["comm_E"], pf, kk, d_ck=Iv["B"], **kw), vv.last_failed_check)
    assert lib(I, proof) == (True, 0) and staged_verify(*_oracle_args(I), proof) == 0
    ran = 0
    # -- the proof
    changes = _proof_changes(I, proof)
    assert len(changes) >= 55
    for name, bad, stage in changes:
        o = staged_verify(*_oracle_args(I), bad)
        assert o != 0 and not SF.verify(*_oracle_args(I), bad), name
        assert lib(I, bad) == (False, o), name
        assert o == stage, (name, o, stage)
        ran += 1
    # -- the statement: the stage is whichever check the oracle's own control flow returns from
    key_pt = C.affine_to_ints(c, B[5:6])[0]
    moved = lambda pt: SF._aff(c, C.jac_add(c, _jac(c, pt), _jac(c, key_pt)))
    stmt = [("X%d" % i, dict(X=[(x + 1) % q if k == i else x for k, x in enumerate(I["X"])])) for i in range(len(I["X"]))]
    stmt += [("u", dict(u=(I["u"] + 1) % q)), ("comm_W", dict(comm_W=moved(I["comm_W"]))), ("comm_E", dict(comm_E=moved(I["comm_E"])))]
    for name, over in stmt:
        Iv = dict(I, **over)
        o = staged_verify(*_oracle_args(Iv), proof)
        assert o != 0 and not SF.verify(*_oracle_args(Iv), proof), name
        assert lib(Iv, proof) == (False, o), name
        ran += 1
    # -- the shape: one coefficient, one column index
    for name, which in (("coefficient", 2), ("column", 1)):
        mats = [tuple(np.array(a, copy=True) for a in M) for M in I["mats"]]
        if which == 2:
            mats[0][2][7] = C.ints_to_limbs([(C.limbs_to_ints(mats[0][2][7:8])[0] + 1) % q])[0]
        else:
            mats[1][1][11] = (int(mats[1][1][11]) + 1) if int(mats[1][1][11]) + 1 < nv - nc else 0  # another free variable
        Iv = dict(I, mats=mats)
        o = staged_verify(*_oracle_args(Iv), proof)
        assert o != 0 and not SF.verify(*_oracle_args(Iv), proof), name
        v2 = SpartanVerifier(c, q, _mont_mats(sf, mats), nc, nv, len(I["X"]))
        assert lib(Iv, proof, vv=v2) == (False, o), name
        v2.close()
        ran += 1
    # -- the key: the inner-product base, one key point
    for name, idx in (("ck_c", N), ("key point", 3)):
        B2 = B.copy()
        B2[idx] = C.synth_bases(c, 1, first=N + 7)[0]
        Iv = dict(I, B=B2)
        o = staged_verify(*_oracle_args(Iv), proof)
        assert o == 5 and not SF.verify(*_oracle_args(Iv), proof), name
        k2 = CommitmentKey(c, B2[:N])
        assert lib(Iv, proof, kk=k2) == (False, 5), name
        k2.close()
        ran += 1
    # -- the label
    o = staged_verify(*_oracle_args(I), proof, label_suffix=b"!")
    assert o != 0
    assert lib(I, proof, label=b"lurk-hip spartan v2" + cn.encode() + b"!") == (False, o)
    ran += 1
    assert ran >= 55 + 9 and ran == len(changes) + len(stmt) + 5  # nothing was skipped
    key.close()
    v.close()


# ---- 3. malformed input -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn,c", CURVES)
def test_malformed_input_is_rejected_before_any_arithmetic(hip, cn, c):
    from lurk_beta_amd import CommitmentKey, LurkHipError, _lib, ipa
    from lurk_beta_amd.spartan import SpartanVerifier

    nc, nv = 8, 16
    I = _instance(cn, c, nc, nv, True)
    q, sf, N, B = I["q"], I["sf"], I["N"], I["B"]
    p = R.modulus(c)
    proof = SF.prove(c, I["mats"], nc, nv, I["X"], B, I["comm_W"], I["comm_E"], I["u"], I["W"], I["E"])
    key = CommitmentKey(c, B[:N])
    v = SpartanVerifier(c, q, _mont_mats(sf, I["mats"]), nc, nv, len(I["X"]))
    run = lambda pf, **over: (v.verify(over.get("X", I["X"]), over.get("u", I["u"]), over.get("comm_W", I["comm_W"]), over.get("comm_E", I["comm_E"]), pf, key, d_ck=B),
                              v.last_failed_check)
    assert run(proof) == (True, 0)
    for big in (q, (1 << 256) - 1):
        for field in ("eval_E", "eval_W", "ipa_a"):
            assert run(dict(proof, **{field: big})) == (False, 1), field
        assert run(dict(proof, claims_outer=[proof["claims_outer"][0], big, proof["claims_outer"][2]])) == (False, 1)
        assert run(dict(proof, polys_inner=[[big] + proof["polys_inner"][0][1:]] + proof["polys_inner"][1:])) == (False, 1)
        assert run(proof, X=[I["X"][0], big]) == (False, 1)
        assert run(proof, u=big) == (False, 1)
    # a value + q is the same residue: the oracle (which reduces) would accept it, the library refuses the encoding
    assert run(dict(proof, eval_W=proof["eval_W"] + q)) == (False, 1)
    # points off the curve
    off = lambda pt: (pt[0], (pt[1] + 1) % p)
    assert run(dict(proof, ipa_L=[off(proof["ipa_L"][0])] + proof["ipa_L"][1:])) == (False, 1)
    assert run(dict(proof, ipa_R=proof["ipa_R"][:-1] + [off(proof["ipa_R"][-1])])) == (False, 1)
    assert run(proof, comm_W=off(I["comm_W"])) == (False, 1)
    assert run(proof, comm_E=off(I["comm_E"])) == (False, 1)
    # a zero a_hat is well-formed: a failed opening
    assert run(dict(proof, ipa_a=0)) == (False, 5)
    assert not SF.verify(*_oracle_args(I), dict(proof, ipa_a=0))
    # wrong list lengths: the wrapper's answer
    assert run(dict(proof, polys_outer=proof["polys_outer"][:-1])) == (False, 1)
    assert run(dict(proof, ipa_L=proof["ipa_L"] + [None])) == (False, 1)
    assert run(dict(proof, evals_batch=proof["evals_batch"][:1])) == (False, 1)
    # the opening argument alone: n not a power of two is a call error, a zero challenge is malformed
    ck_c = np.concatenate([B[N], C.ints_to_limbs([(1 << 256) % p])[0]])
    P = np.zeros(12, dtype=np.uint64)
    with pytest.raises(LurkHipError):
        ipa.verify(key, 12, P, ck_c, [P] * 3, [P] * 3, 1, lambda j, L, Rr: 5, eq_point=[1, 2, 3])
    with pytest.raises(LurkHipError):
        ipa.verify(key, 2 * N, P, ck_c, [P] * (N.bit_length()), [P] * (N.bit_length()), 1, lambda j, L, Rr: 5, eq_point=[1] * N.bit_length())  # more than the key holds
    assert ipa.verify(key, 8, P, ck_c, [P] * 3, [P] * 3, 1, lambda j, L, Rr: 0 if j == 1 else 5, eq_point=[1, 2, 3]) == (False, 1)
    assert ipa.verify(key, 8, P, ck_c, [P] * 3, [P] * 3, 1, lambda j, L, Rr: q, eq_point=[1, 2, 3]) == (False, 1)
    # ... and a well-formed one that does not open: check 5; the all-identity statement with a_hat = 0 does open (0 == 0)
    assert ipa.verify(key, 8, P, ck_c, [P] * 3, [P] * 3, 1, lambda j, L, Rr: 5 + j, eq_point=[1, 2, 3]) == (False, 5)
    assert ipa.verify(key, 8, P, ck_c, [P] * 3, [P] * 3, 0, lambda j, L, Rr: 5 + j, eq_point=[1, 2, 3]) == (True, 0)
    # the general-b form agrees with the closed form of b = eq(point)
    from lurk_beta_amd import sumcheck

    Rq = (1 << 256) % q
    d_b = sumcheck.eq_evals(sf, sumcheck._limbs([z * Rq % q for z in (1, 2, 3)]))
    assert ipa.verify(key, 8, P, ck_c, [P] * 3, [P] * 3, 0, lambda j, L, Rr: 5 + j, d_b=d_b) == (True, 0)
    assert ipa.verify(key, 8, P, ck_c, [P] * 3, [P] * 3, 3, lambda j, L, Rr: 5 + j, d_b=d_b) == (False, 5)
    key.close()
    v.close()


# ---- 4. batched -------------------------------------------------------------------------------------------------------------------------
def _batch(cn, c, dims):
    from lurk_beta_amd import CommitmentKey
    from lurk_beta_amd.spartan import SpartanProver

    sf, q = 1 - c, R.CURVES[cn]["order"]
    N = max(max(nc, nv) for nc, nv, _, _ in dims)
    B = C.synth_bases(c, N + 1)
    key = CommitmentKey(c, B[:N])
    insts, provers, dev_insts = [], [], []
    for nc, nv, folded, seed in dims:
        mats, X, u, W, E = product_instance(cn, nc, nv, 2, seed, folded)
        m_arr, W_arr, E_arr = _to_arrays(mats, X, W, E)
        cw, ce = key.commit(W_arr), key.commit(E_arr)
        insts.append(dict(mats=m_arr, num_cons=nc, num_vars=nv, X=X, u=u, W=W_arr, E=E_arr, comm_W=SF._aff(c, cw), comm_E=SF._aff(c, ce)))
        provers.append(SpartanProver(c, q, _mont_mats(sf, m_arr), nc, nv, len(X)))
        dev_insts.append(dict(X=X, u=u, d_W=_dev(C.to_mont(sf, W_arr)), d_E=_dev(C.to_mont(sf, E_arr)), comm_W=cw, comm_E=ce))
    return q, B, key, insts, provers, dev_insts


def _check_batch(c, q, B, key, insts, provers, dev_insts, oracle_proof):
    from lurk_beta_amd.spartan import BatchedSpartanProver, BatchedSpartanVerifier, SpartanVerifier

    got = BatchedSpartanProver(provers).prove(dev_insts, _dev(B), key=key, in_library=True)
    pub = [{k: v for k, v in it.items() if k not in ("W", "E")} for it in insts]
    bv = BatchedSpartanVerifier([SpartanVerifier.from_shape(p.shape, c, q) for p in provers])
    run = lambda pubs, pf, vv=bv: (vv.verify(pubs, pf, key, d_ck=B), vv.last_failed_check)
    for proof in ([got, oracle_proof] if oracle_proof is not None else [got]):
        assert run(pub, proof) == (True, 0) and run(dev_insts, proof) == (True, 0)
        assert staged_verify_batched(c, pub, B, proof) == 0 and SF.verify_batched(c, pub, B, proof)
    for i in (0, len(pub) - 1):
        bad = [dict(it) for it in pub]
        bad[i]["X"] = [(bad[i]["X"][0] + 1) % q] + bad[i]["X"][1:]
        o = staged_verify_batched(c, bad, B, got)
        assert o != 0 and not SF.verify_batched(c, bad, B, got)
        assert run(bad, got) == (False, o)
    if len(pub) > 1:  # the proof of the batch in another instance order
        order = list(range(1, len(pub))) + [0]
        re_pub = [pub[i] for i in order]
        bv2 = BatchedSpartanVerifier([SpartanVerifier.from_shape(provers[i].shape, c, q) for i in order])
        o = staged_verify_batched(c, re_pub, B, got)
        assert o != 0 and not SF.verify_batched(c, re_pub, B, got)
        assert run(re_pub, got, vv=bv2) == (False, o)
    # malformed: an evaluation that is not reduced; wrong counts
    assert run(pub, dict(got, evals_W=[got["evals_W"][0] + q] + got["evals_W"][1:])) == (False, 1)
    assert run(pub, dict(got, evals_E=got["evals_E"] + [0])) == (False, 1)
    assert run(pub[:-1] if len(pub) > 1 else pub + pub, got) == (False, 1)
    assert run(pub, dict(got, ipa_a=(got["ipa_a"] + 1) % q)) == (False, 5)
    return got


@pytest.mark.parametrize("cn,c,dims", [("pallas", 0, [(16, 64, True, 11), (64, 128, False, 12), (8, 16, True, 13)]),
                                       ("vesta", 1, [(32, 64, True, 21), (8, 32, False, 22)])])
def test_batched_verifier_decides_as_the_oracle(hip, cn, c, dims):
    q, B, key, insts, provers, dev_insts = _batch(cn, c, dims)
    want = SF.prove_batched(c, insts, B)
    assert _check_batch(c, q, B, key, insts, provers, dev_insts, want) == want
    key.close()
    for p in provers:
        p.close()


def test_batched_verifier_at_2_12_and_2_14(hip):
    from lurk_beta_amd import CommitmentKey
    from lurk_beta_amd.spartan import SpartanProver

    c, sf, q = 0, 1, R.CURVES["pallas"]["order"]
    sizes = [1 << 12, 1 << 14]
    N = max(sizes)
    B = C.synth_bases(c, N + 1)
    key = CommitmentKey(c, B[:N], precompute=True)
    insts, provers, dev_insts = [], [], []
    for k, n in enumerate(sizes):
        A, Bm, Cm, W, X = SF.synth_product_instance(sf, n, n, 2, seed=30 + k)
        E = np.zeros((n, 4), dtype=np.uint64)
        cw = key.commit(W)
        insts.append(dict(mats=(A, Bm, Cm), num_cons=n, num_vars=n, X=X, u=1, W=W, E=E, comm_W=SF._aff(c, cw), comm_E=None))
        provers.append(SpartanProver(c, q, _mont_mats(sf, (A, Bm, Cm)), n, n, len(X)))
        dev_insts.append(dict(X=X, u=1, d_W=_dev(C.to_mont(sf, W)), d_E=_dev(E), comm_W=cw, comm_E=np.zeros(12, dtype=np.uint64)))
    _check_batch(c, q, B, key, insts, provers, dev_insts, None)
    key.close()
    for p in provers:
        p.close()


# ---- 5. at the benchmark's size ----------------------------------------------------------------------------------------------------------
def test_verifies_the_2_20_compress_instance_as_the_oracle_does(hip):
    """The 2^20 x 2^20 instance of bench_workloads/compress.py (six public inputs, table key): the library prover's proof is accepted,
    rejected for X[0] + 1, and the oracle's verifier (2-4 s per call on the CPU: this test's duration) decides the same."""
    import torch

    from lurk_beta_amd import CommitmentKey
    from lurk_beta_amd.spartan import SpartanProver, SpartanVerifier

    c, sf, q = 0, 1, R.CURVES["pallas"]["order"]
    nc = nv = 1 << 20
    A, Bm, Cm, W, X = SF.synth_product_instance(sf, nc, nv, 6, seed=11)
    B = C.synth_bases(c, nc + 1)
    prover = SpartanProver(c, q, _mont_mats(sf, (A, Bm, Cm)), nc, nv, len(X))
    verifier = SpartanVerifier.from_shape(prover.shape, c, q)
    d_W, d_E, d_B = _dev(C.to_mont(sf, W)), torch.zeros((nc, 4), dtype=torch.int64, device="cuda"), _dev(B)
    key = CommitmentKey(c, d_B, n=nc, device=True, precompute=True)
    cw, ce = key.commit_device(d_W, nv, is_mont=True), key.commit_device(d_E, nc, is_mont=True)
    proof = prover.prove(X, 1, d_W, d_E, d_B, cw, ce, key=key, in_library=True)
    bad_x = [(X[0] + 1) % q] + X[1:]
    assert verifier.verify(X, 1, cw, ce, proof, key, d_ck=d_B) is True and verifier.last_failed_check == 0
    # (X is absorbed before the first challenge: another X is another tau, and the outer sum-check's final claim misses - the stage the
    # instrumented oracle returns from at every smaller size above)
    assert verifier.verify(bad_x, 1, cw, ce, proof, key, d_ck=d_B) is False and verifier.last_failed_check == 2
    aff = lambda J: SF._aff(c, np.ascontiguousarray(J, dtype=np.uint64))
    assert SF.verify(c, (A, Bm, Cm), nc, nv, X, B, aff(cw), aff(ce), 1, proof)
    assert not SF.verify(c, (A, Bm, Cm), nc, nv, bad_x, B, aff(cw), aff(ce), 1, proof)
    key.close()
    prover.close()


# ---- 6. the building blocks against oracle.c ---------------------------------------------------------------------------------------------
def _mle_check(f, mats, rows, cols_needed, shape, n_x=None, n_y=None, seeds=(1, 2), extreme=True):
    """sparse_mle_dev == SF.sparse_mle for A, B, C with random and all-(q - 1) tables of n_x / n_y elements."""
    q = R.modulus(f)
    n_x, n_y = n_x or rows, n_y or cols_needed
    tables = [(C.synth_scalars(f, 40 + seeds[0], 0, n_x), C.synth_scalars(f, 40 + seeds[1], 0, n_y))]
    if extreme:
        tables.append((np.tile(C.ints_to_limbs([q - 1]), (n_x, 1)), np.tile(C.ints_to_limbs([q - 1]), (n_y, 1))))
    for ex, ey in tables:
        got = C.limbs_to_ints(C.from_mont(f, shape.sparse_mle(_dev(C.to_mont(f, ex)), _dev(C.to_mont(f, ey)))))
        # the oracle reads eq_rx[row] for row < rows and eq_ry[col]: truncated tables are simply shorter arrays
        want = [SF.sparse_mle(f, M, np.ascontiguousarray(ex), np.ascontiguousarray(ey)) for M in mats]
        assert got == want


@pytest.mark.parametrize("log_n", [10, 16])
def test_sparse_mle_on_the_synthetic_product_shape(hip, log_n):
    from lurk_beta_amd import LurkHipError, R1CSShape

    f, n = 1, 1 << log_n
    A, Bm, Cm, _, X = SF.synth_product_instance(f, n, n, 2, seed=log_n)
    shape = R1CSShape(f, n, n, len(X), *_mont_mats(f, (A, Bm, Cm)))
    _mle_check(f, (A, Bm, Cm), n, 2 * n, shape)
    _mle_check(f, (A, Bm, Cm), n, n + 1 + len(X), shape, n_x=n + 5, extreme=False)  # truncated / longer tables
    ex, ey = _dev(np.zeros((n, 4), dtype=np.uint64)), _dev(np.zeros((2 * n, 4), dtype=np.uint64))
    with pytest.raises(LurkHipError):
        shape.sparse_mle(ex[: n - 1].contiguous(), ey)
    max_col = int(max(M[1].max() for M in (A, Bm, Cm)))
    with pytest.raises(LurkHipError):
        shape.sparse_mle(ex, ey[:max_col].contiguous())
    assert shape.sparse_mle(ex, ey[: max_col + 1].contiguous()).any() == False  # noqa: E712 - zero tables, the shortest legal eq_y
    shape.close()


@pytest.mark.parametrize("f", [0, 1, 2])
def test_sparse_mle_on_the_slot_rows(hip, f):
    """A shape from lurk_hip_frames_r1cs_create with all five slot types: rows of up to 66 terms, the 1 405-coefficient dictionary."""
    from lurk_beta_amd import R1CSShape, slot_constraints, slot_witness_size

    counts, types = [2, 1, 1, 1, 2], [4, 6, 8, 3, 1]  # (hash4, hash6, hash8, commitment, bit_decomp): LURK_SLOT_*
    shape_len = sum(n * slot_witness_size(f, t) for n, t in zip(counts, types))
    num_frames, first = 2, 3
    nv, nio = first + num_frames * shape_len + 4, 2
    shape = R1CSShape.for_frames(f, num_frames, counts, first, shape_len, nv, nio)
    # the same rows as host CSR for the oracle
    mats = [([0], [], []) for _ in range(3)]
    base = first
    for _ in range(num_frames):
        for n, t in zip(counts, types):
            size = slot_witness_size(f, t)
            cons = slot_constraints(f, t)
            for _k in range(n):
                for w in range(3):
                    ip, ix, dv = cons[w]
                    at = len(mats[w][1])
                    mats[w][1].extend(nv if int(col) == size else base + int(col) for col in ix)
                    mats[w][2].extend(C.limbs_to_ints(C.from_mont(f, np.ascontiguousarray(dv).reshape(-1, 4))) if len(ix) else [])
                    mats[w][0].extend(at + int(x) for x in ip[1:])
                base += size
    rows = len(mats[0][0]) - 1
    assert rows == shape.num_cons and max(np.diff(mats[0][0]).max(), np.diff(mats[1][0]).max()) >= 60
    assert shape.info()["distinct_coefficients"] >= 1000
    arr = [(np.array(ip, dtype=np.uint64), np.array(ix, dtype=np.uint64), C.ints_to_limbs(dv)) for ip, ix, dv in mats]
    _mle_check(f, arr, rows, nv + 1 + nio, shape)
    shape.close()


@pytest.mark.parametrize("f", [0, 1])
def test_sparse_mle_on_empty_rows_a_200_term_row_and_a_single_row(hip, f):
    from lurk_beta_amd import R1CSShape

    q = R.modulus(f)
    rng = np.random.default_rng(5 + f)
    nv, nio = 300, 1
    ncols = nv + 1 + nio

    def mat(lens):
        ip = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(np.array(lens, dtype=np.uint64), out=ip[1:])
        nnz = int(ip[-1])
        return ip, rng.integers(0, ncols, nnz).astype(np.uint64), C.synth_scalars(f, 60 + len(lens), 0, max(nnz, 1))[:nnz]

    # rows: empty, 3 terms, empty, 200 terms in A only (crosses RowAcc's 64-term fold; 16 lanes), 300 terms (beyond 256: the partial sums
    # re-enter one by one), 20 terms (4 lanes), empty
    lens_a, lens_b, lens_c = [0, 3, 0, 200, 300, 20, 0], [0, 1, 0, 0, 2, 70, 0], [0, 0, 0, 1, 0, 0, 0]
    mats = (mat(lens_a), mat(lens_b), mat(lens_c))
    shape = R1CSShape(f, 7, nv, nio, *_mont_mats(f, mats))
    _mle_check(f, mats, 7, ncols, shape)
    _mle_check(f, mats, 7, ncols, shape, n_x=8, n_y=512, extreme=False)
    shape.close()
    one = (mat([5]), mat([1]), mat([0]))
    shape = R1CSShape(f, 1, nv, nio, *_mont_mats(f, one))
    _mle_check(f, one, 1, ncols, shape)
    shape.close()
    empty = (mat([0, 0]), mat([0, 0]), mat([0, 0]))
    shape = R1CSShape(f, 2, nv, nio, *_mont_mats(f, empty))
    assert not shape.sparse_mle(_dev(C.synth_scalars(f, 1, 0, 2)), _dev(C.synth_scalars(f, 2, 0, ncols))).any()
    shape.close()


def _oracle_s_vector(f, chal):
    ell = len(chal)
    out = np.empty((1 << ell, 4), dtype=np.uint64)
    ch = C.ints_to_limbs(chal) if ell else np.zeros((1, 4), dtype=np.uint64)
    C.lib().orc_ipa_s_vector(f, ch.ctypes.data_as(ctypes.c_void_p), ell, out.ctypes.data_as(ctypes.c_void_p))
    return out


@pytest.mark.parametrize("f", [0, 1])
def test_s_vector_matches_the_oracle(hip, f):
    from lurk_beta_amd import LurkHipError, ipa

    q = R.modulus(f)
    for ell in range(17):
        chal = [R.uniform_fe(90 + ell, j, q) or 1 for j in range(ell)]
        if ell >= 2:
            chal[1] = q - 1
        got = C.from_mont(f, ipa.s_vector(f, chal).cpu().numpy().view(np.uint64))
        assert np.array_equal(got, _oracle_s_vector(f, chal)), ell
    chal = [R.uniform_fe(77, j, q) or 1 for j in range(20)]
    got = C.from_mont(f, ipa.s_vector(f, chal).cpu().numpy().view(np.uint64))
    want = _oracle_s_vector(f, chal)
    pos = np.concatenate([[0, (1 << 20) - 1], np.random.default_rng(3).integers(0, 1 << 20, 1 << 12)])
    assert np.array_equal(got[pos], want[pos])
    for bad in ([3, 0, 5], [3, q, 5], [q + 1]):
        with pytest.raises(LurkHipError):
            ipa.s_vector(f, bad)


@pytest.mark.parametrize("cn,c", CURVES)
def test_sumcheck_verify_on_the_oracles_polynomials(hip, cn, c):
    from lurk_beta_amd import sumcheck

    I = _instance(cn, c, 32, 64, True)
    q, sf = I["q"], I["sf"]
    proof = SF.prove(c, I["mats"], 32, 64, I["X"], I["B"], I["comm_W"], I["comm_E"], I["u"], I["W"], I["E"])
    rng = np.random.default_rng(2)
    for name, degree, claim in (("polys_outer", 3, 0), ("polys_inner", 2, None), ("polys_batch", 2, None)):
        polys = proof[name]
        rs = [int.from_bytes(rng.bytes(31), "little") for _ in polys]
        if claim is None:
            claim = (2 * polys[0][0] + sum(polys[0][1:])) % q
        # (random challenges: only the first round is consistent - the oracle decides, the library agrees; then the consistent prefix)
        assert sumcheck.verify(sf, degree, claim, polys, rs) == S._sc_verify(q, claim, polys, rs)
        assert sumcheck.verify(sf, degree, claim, polys[:1], rs[:1]) == S._sc_verify(q, claim, polys[:1], rs[:1]) != None  # noqa: E711
        bad = [list(polys[0])]
        bad[0][2] = (bad[0][2] + 1) % q
        assert sumcheck.verify(sf, degree, claim, bad, rs[:1]) is None and S._sc_verify(q, claim, bad, rs[:1]) is None


# ---- 7. streams ------------------------------------------------------------------------------------------------------------------------------
def test_two_verifiers_on_two_streams_from_two_threads(hip):
    import torch

    from lurk_beta_amd import CommitmentKey
    from lurk_beta_amd.spartan import SpartanVerifier

    cn, c = "pallas", 0
    setups = []
    for nc, nv, seed in ((32, 64, 9), (64, 128, 10)):
        I = _instance(cn, c, nc, nv, True, seed=seed)
        proof = SF.prove(c, I["mats"], nc, nv, I["X"], I["B"], I["comm_W"], I["comm_E"], I["u"], I["W"], I["E"])
        setups.append((I, proof, CommitmentKey(c, I["B"][: I["N"]]), SpartanVerifier(c, I["q"], _mont_mats(I["sf"], I["mats"]), nc, nv, len(I["X"]))))
    results, errors = [[], []], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            I, proof, key, v = setups[t]
            stream = torch.cuda.Stream()
            X = I["X"] if t == 0 else [(I["X"][0] + 1) % I["q"]] + I["X"][1:]  # thread 0 accepts, thread 1 rejects
            for _ in range(8):
                ok = v.verify(X, I["u"], I["comm_W"], I["comm_E"], proof, key, d_ck=I["B"], stream=stream.cuda_stream)
                results[t].append((ok, v.last_failed_check))
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert results[0] == [(True, 0)] * 8
    assert results[1] == [(False, 2)] * 8  # (another X: another tau - the outer check, as the instrumented oracle says above)
    for _, _, key, v in setups:
        key.close()
        v.close()
