"""GPU: the three polynomial primitives of the HyperKZG argument against Python integers over fields 0, 1 and 2, the powers-of-tau key,
and the prover (lurk_hip_hyperkzg_prove_dev) against the trapdoor reference of tests/hyperkzg_ref.py element for element."""
import random

import numpy as np
import pytest

from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK

pytestmark = pytest.mark.gpu

PALLAS_P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001
PALLAS_Q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
MOD = {0: PALLAS_P, 1: PALLAS_Q, 2: BN.BN254_R}
FIELDS = (0, 1, 2)
SMALL = list(range(1, 131))
# lane / wave / workgroup / multi-chunk boundaries; 1023 .. 1025: the division's tile; 2^18: the last length whose tile carries fit one
# lane each (2^18 + 3 takes two per lane)
BIG = [1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193, 65537, (1 << 18), (1 << 18) + 3]
EVAL_LONG = (1 << 20) + 257  # past 256 segments of 4096 coefficients the evaluation lengthens its segments
TAU = 0x2B0F3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % HK.Q


def dev(p, ints):
    import torch

    return torch.from_numpy(BN.to_mont(p, ints).view(np.int64).reshape(-1, 4)).cuda()


def host(p, t):
    return BN.from_mont(p, t.cpu().numpy().view(np.uint64))


_vec = {}


def vector(f, n, kind="mixed"):
    """(ints, device tensor): 0, 1, p - 1 among random values, or all p - 1"""
    key = (f, n, kind)
    if key not in _vec:
        p = MOD[f]
        if kind == "ones":
            v = [p - 1] * n
        else:
            rng = random.Random(7 * n + f)
            v = [rng.getrandbits(256) % p for _ in range(n)]
            for k, s in ((0, p - 1), (1, 0), (2, 1), (n - 1, p - 1), (n // 2, 0)):
                if k < n:
                    v[k] = s
        _vec[key] = (v, dev(p, v))
        if len(_vec) > 64:  # (the three primitives' tests of a field share their vectors)
            _vec.pop(next(iter(_vec)))
    return _vec[key]


def points(f, k):
    p = MOD[f]
    rng = random.Random(99 + f)
    return ([p - 1, rng.getrandbits(256) % p, 1, 0][:k] if k != 1 else [rng.getrandbits(256) % p])


def base_vector(f):
    return vector(f, 130)


def cases(f):
    v, d = base_vector(f)
    for n in SMALL:
        yield n, v[:n], d[:n]
    for n in BIG:
        yield (n,) + vector(f, n)
    for n in (130, 4097, 65537):
        yield (n,) + vector(f, n, "ones")


@pytest.mark.parametrize("f", FIELDS)
def test_fold_pairs_matches_python_integers(f):
    from lurk_beta_amd import hyperkzg

    p = MOD[f]
    for x in (0, 1, p - 1, 0x123456789ABCDEF0123456789ABCDEF % p):
        xm = BN.to_mont(p, [x])
        for n, v, d in cases(f):
            if n > 130 and x in (0, 1, p - 1):
                continue
            got = host(p, hyperkzg.fold_pairs(f, d, xm))
            vv = v + [0] * (n & 1)
            want = [(vv[2 * j] + x * (vv[2 * j + 1] - vv[2 * j])) % p for j in range((n + 1) // 2)]
            assert got == want, (f, n, x)


@pytest.mark.parametrize("f", FIELDS)
def test_poly_eval_matches_python_integers(f):
    from lurk_beta_amd import hyperkzg

    p = MOD[f]
    for idx, (n, v, d) in enumerate(cases(f)):
        for k in ((1, 3, 4) if n <= 130 else ((1, 3, 4)[idx % 3],)):  # (a long vector takes one of the three counts, in turn)
            pts = points(f, k)
            got = BN.from_mont(p, hyperkzg.poly_eval(f, d, BN.to_mont(p, pts)))
            assert got == [HK.poly_eval(v, u, p) for u in pts], (f, n, k)
    v, d = vector(f, EVAL_LONG)
    u = points(f, 1)
    assert BN.from_mont(p, hyperkzg.poly_eval(f, d, BN.to_mont(p, u))) == [HK.poly_eval(v, u[0], p)]


@pytest.mark.parametrize("f", FIELDS)
def test_poly_div_linear_matches_python_integers(f):
    from lurk_beta_amd import hyperkzg

    p = MOD[f]
    rng = random.Random(31 + f)
    w = rng.getrandbits(256) % p
    for idx, (n, v, d) in enumerate(cases(f)):
        for roots in (([w], [p - 1, w, w], [0, 1, w]) if n <= 130 else (([w], [p - 1, w, w])[idx % 2],)):
            quot, rem = hyperkzg.poly_div_linear(f, d, BN.to_mont(p, roots))
            rem = BN.from_mont(p, rem)
            for k, u in enumerate(roots):
                h = host(p, quot[k]) if n > 1 else []
                assert len(h) == n - 1
                want_h, want_rem = HK.div_linear(v, u, p)
                assert rem[k] == want_rem, (f, n, roots, k)
                assert h == want_h, (f, n, roots, k)
                # quotient (X - u) + remainder == input, coefficient by coefficient
                back = [((h[j - 1] if j >= 1 else 0) - u * (h[j] if j < n - 1 else 0) + (rem[k] if j == 0 else 0)) % p for j in range(n)]
                assert back == v, (f, n, roots, k)


def test_primitives_refuse_bad_arguments():
    import torch

    from lurk_beta_amd import LurkHipError, _lib, hyperkzg

    v, d = vector(2, 8)
    one = BN.to_mont(MOD[2], [1])
    with pytest.raises(LurkHipError, match="alias"):
        _lib.check(_lib.load().lurk_hip_mle_fold_pairs_dev(2, _lib.ptr(d), 8, _lib.ptr(one), _lib.ptr(d), None))
    with pytest.raises(LurkHipError, match="field"):
        hyperkzg.fold_pairs(3, d, one)
    with pytest.raises(LurkHipError, match="points"):
        hyperkzg.poly_eval(2, d, BN.to_mont(MOD[2], [1, 2, 3, 4, 5]))
    with pytest.raises(LurkHipError, match="roots"):
        hyperkzg.poly_div_linear(2, d, BN.to_mont(MOD[2], [1, 2, 3, 4]))
    torch.cuda.synchronize()
    assert BN.from_mont(MOD[2], hyperkzg.poly_eval(2, d, one)) == [sum(v) % MOD[2]]


def test_powers_of_tau_key():
    from lurk_beta_amd import LurkHipError, hyperkzg

    G = BN.BN254.gen

    def check(first, n):
        got = hyperkzg.kzg_bases(TAU, n, first=first).cpu().numpy().view(np.uint64).reshape(-1, 4)
        xy = BN.from_mont(BN.BN254_P, got)
        for i in range(n):
            assert BN.from_xy((xy[2 * i], xy[2 * i + 1])) == BN.BN254.mul(pow(TAU, first + i, HK.Q), G), (first, i)

    check(0, 64)
    check(250, 12)            # straddles the first workgroup
    check((1 << 20) - 3, 6)   # and an index of more than 20 bits
    xy = BN.from_mont(BN.BN254_P, hyperkzg.kzg_bases(0, 3).cpu().numpy().view(np.uint64).reshape(-1, 4))
    assert [BN.from_xy((xy[2 * i], xy[2 * i + 1])) for i in range(3)] == [G, None, None]  # tau = 0: [1]G, then the identity
    for curve, name in ((0, "Pallas"), (1, "Vesta"), (3, "Grumpkin")):
        with pytest.raises(LurkHipError, match=name):
            hyperkzg.kzg_bases(TAU, 4, curve=curve)


# ---- the prover ----------------------------------------------------------------------------------------------------------------------
_keys = {}


def key(n, **kw):
    from lurk_beta_amd import hyperkzg

    k = (n, tuple(sorted(kw.items())))
    if k not in _keys:
        _keys[k] = hyperkzg.trapdoor_key(TAU, n, **kw)
    return _keys[k]


def affine(jac):
    from lurk_beta_amd import point_to_affine

    return BN.from_xy(point_to_affine(BN.CURVE_BN254, jac))


class DeviceTranscript:
    """tests/hyperkzg_ref.py's transcript behind the library's callback: Jacobians become affine tuples first"""

    def __init__(self):
        self.tr = HK.Transcript()
        self.out = {}

    def __call__(self, stage, data):
        c = self.tr(stage, [affine(j) for j in data] if stage == 0 else data)
        self.out[stage] = c
        return c


def prove_and_check(ck, p0, x, want=None):
    from lurk_beta_amd import hyperkzg

    ell = len(x)
    tr = DeviceTranscript()
    pf = hyperkzg.prove(ck, dev(HK.Q, p0), x, tr)
    ref = want if want is not None else HK.prove(TAU, p0, x, HK.Transcript())
    assert [affine(j) for j in pf["com"]] == ref["com"]
    assert (tr.out[0], tr.out[1]) == (ref["r"], ref["q"])
    assert pf["v"] == ref["v"]
    assert [affine(j) for j in pf["w"]] == ref["w"]
    assert pf["y"] == ref["y"]
    d = tr.tr(2, ref["w"])
    c = BN.jacobian(BN.BN254, HK.commit_trapdoor(TAU, p0))
    L, R, ok, code = hyperkzg.pairing_inputs(ell, c, x, pf["y"], pf["com"], pf["v"], pf["w"], tr.out[0], tr.out[1], d)
    assert ok and code == 0
    assert HK.trapdoor_holds(TAU, affine(L), affine(R))
    return pf, ref


def random_instance(ell, seed=0):
    rng = random.Random(50 * ell + seed)
    p0 = [rng.getrandbits(256) % HK.Q for _ in range(1 << ell)]
    p0[0], p0[-1] = HK.Q - 1, 1
    return p0, [rng.getrandbits(256) % HK.Q for _ in range(ell)]


@pytest.mark.parametrize("ell", (1, 2, 3, 5, 10, 16))
def test_prover_matches_the_trapdoor_reference(ell):
    p0, x = random_instance(ell)
    pf, _ = prove_and_check(key(1 << ell), p0, x)
    assert pf["com"].shape == (ell - 1, 12)


def test_prover_edge_inputs():
    ell, n = 5, 32
    ck = key(n)
    p0, x = random_instance(ell, seed=1)
    pf, _ = prove_and_check(ck, [0] * n, x)  # the zero polynomial: every commitment is the identity
    assert all(affine(j) is None for j in pf["com"]) and all(affine(j) is None for j in pf["w"]) and pf["y"] == 0
    prove_and_check(ck, [0] * (n - 1) + [HK.Q - 2], x)  # a single non-zero entry, at index n - 1
    _, ref0 = prove_and_check(ck, p0, [0] * ell)
    assert ref0["y"] == p0[0]
    _, ref1 = prove_and_check(ck, p0, [1] * ell)
    assert ref1["y"] == p0[-1]
    ref = HK.prove(TAU, p0, x, HK.Transcript())
    a, _ = prove_and_check(ck, p0, x, ref)
    b, _ = prove_and_check(ck, p0, x, ref)  # two proofs in a row under one key: identical output
    assert np.array_equal(a["com"], b["com"]) and np.array_equal(a["w"], b["w"]) and (a["v"], a["y"]) == (b["v"], b["y"])
    prove_and_check(key(64), p0, x, ref)  # a key longer than n
    table = key(n, precompute=True, window_bits=16)
    assert table.info()["form"] == "table"
    prove_and_check(table, p0, x, ref)
    assert ck.info()["form"] == "plain"


def test_prover_refusals_name_their_reason_and_leave_the_key_usable():
    from lurk_beta_amd import CommitmentKey, LurkHipError, hyperkzg, synth

    ell, n = 5, 32
    ck = key(n)
    p0, x = random_instance(ell, seed=2)
    ref = HK.prove(TAU, p0, x, HK.Transcript())
    d_p = dev(HK.Q, p0)
    never = lambda stage, data: pytest.fail("the transcript was asked although the call is refused")
    for curve, name in ((0, "Pallas"), (3, "Grumpkin")):
        other = CommitmentKey(curve, synth.bases(curve, n), n=n, device=True)
        with pytest.raises(LurkHipError, match=name):
            hyperkzg.prove(other, d_p, x, never)
        other.close()
    with pytest.raises(LurkHipError, match="power of two"):
        hyperkzg.prove(ck, d_p[:24], x[:4], never)
    with pytest.raises(LurkHipError, match="fewer points"):
        hyperkzg.prove(ck, dev(HK.Q, p0 + p0), x + [1], never)
    prove_and_check(ck, p0, x, ref)
    with pytest.raises(LurkHipError, match="zero challenge"):
        hyperkzg.prove(ck, d_p, x, lambda stage, data: 0)
    prove_and_check(ck, p0, x, ref)
    for bad_stage in (0, 1):
        with pytest.raises(LurkHipError, match="callback failed"):
            hyperkzg.prove(ck, d_p, x, lambda stage, data: None if stage == bad_stage else 5)
        prove_and_check(ck, p0, x, ref)
    with pytest.raises(LurkHipError, match="not reduced"):
        hyperkzg.prove(ck, d_p, x, lambda stage, data: HK.Q)
    prove_and_check(ck, p0, x, ref)
