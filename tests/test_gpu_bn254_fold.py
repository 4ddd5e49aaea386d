"""The folding context on the BN254 primary curve (shape over Fr, BN254 key), r supplied by the caller, against Python integers:
spmv / cross_term / axpy of oracle/pyref.py (generic over the modulus) and the commitments of tests/bn254_ref.py.  Needs an MI355X."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import bn254_ref as B

pytestmark = pytest.mark.gpu

C = B.BN254
P = C.order  # the circuit field: BN254 Fr
M, NV, NIO = 96, 80, 2


def _matrix(rng):
    """CSR over z = [W | u | X]: every third row long (the step's long-row path), the others 1-3 entries"""
    ncols = NV + 1 + NIO
    indptr, indices, data = [0], [], []
    for i in range(M):
        k = 40 if i % 3 == 0 else rng.randrange(1, 4)
        cols = sorted(rng.sample(range(ncols), k))
        indices += cols
        data += [rng.randrange(1, P) if rng.random() < 0.7 else rng.choice([1, P - 1, 2]) for _ in cols]
        indptr.append(len(indices))
    return indptr, indices, data


@pytest.fixture(scope="module")
def setup(hip):
    import lurk_beta_amd as L

    rng = random.Random("bn254-fold")
    mats = [_matrix(rng) for _ in range(3)]
    shape = L.R1CSShape(B.FIELD_BN254_FR, M, NV, NIO, *[(ip, ix, B.to_mont(P, d)) for ip, ix, d in mats])
    pts = C.synth_bases(max(M, NV))
    key = L.CommitmentKey(B.CURVE_BN254, B.affine_bases(C, pts))
    yield L, mats, shape, key, pts, rng
    key.close()
    shape.close()


def _affine(L, jac):
    return B.from_xy(L.point_to_affine(B.CURVE_BN254, jac))


def test_three_steps_and_a_staged_one(setup):
    L, mats, shape, key, pts, rng = setup
    ctx = L.FoldingContext(B.CURVE_BN254, shape, key)
    ctx2 = L.FoldingContext(B.CURVE_BN254, shape, key)  # the same steps, the last one staged
    z1, e1, u1 = [0] * (NV + 1 + NIO), [0] * M, 0
    cw1 = ce1 = None
    abc = lambda z: [R.spmv(P, *m, z) for m in mats]
    steps = []
    for step in range(3):
        w2 = [rng.randrange(P) for _ in range(NV)]
        x2 = [rng.randrange(P) for _ in range(NIO)]
        r = rng.randrange(1 << 128)
        steps.append((w2, x2, r))
        z2 = w2 + [1] + x2
        t = R.cross_term(P, *abc(z1), *abc(z2), u1, 1)
        cw, ct = ctx.begin(B.to_mont(P, w2), B.to_mont(P, x2))
        want_cw, want_ct = C.msm(w2, pts[:NV]), C.msm(t, pts[:M])
        assert _affine(L, cw) == want_cw and _affine(L, ct) == want_ct, step
        ctx.finish(B.to_mont(P, [r]))
        z1, e1, u1 = R.axpy(P, z1, z2, r), R.axpy(P, e1, t, r), (u1 + r) % P
        cw1, ce1 = C.add(cw1, C.mul(r, want_cw)), C.add(ce1, C.mul(r, want_ct))
        gz, ge = ctx.read()
        assert B.from_mont(P, gz) == z1 and B.from_mont(P, ge) == e1, step
        icw, ice, iu, ix = ctx.instance()
        assert _affine(L, icw) == cw1 and _affine(L, ice) == ce1, step
        assert B.from_mont(P, iu) == [u1] and B.from_mont(P, ix) == z1[NV + 1:], step
    # the second context: two plain steps, then the third staged ahead (prefetch + begin_prefetched with a late patch)
    for w2, x2, r in steps[:2]:
        ctx2.begin(B.to_mont(P, w2), B.to_mont(P, x2))
        ctx2.finish(B.to_mont(P, [r]))
    w2, x2, r = steps[2]
    late = 7  # the last 7 witness values arrive with the step
    ctx2.prefetch(B.to_mont(P, w2[:NV - late]), 0)
    cw, ct = ctx2.begin_prefetched(B.to_mont(P, x2), patches=[(NV - late, B.to_mont(P, w2[NV - late:]))])
    assert _affine(L, cw) == C.msm(w2, pts[:NV])
    ctx2.finish(B.to_mont(P, [r]))
    gz2, ge2 = ctx2.read()
    gz, ge = ctx.read()
    assert np.array_equal(gz, gz2) and np.array_equal(ge, ge2)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.instance(), ctx2.instance()))
    # set_running: a third context adopts the running pair and folds one more step like the first
    ctx3 = L.FoldingContext(B.CURVE_BN254, shape, key)
    ctx3.set_running(gz, ge, ctx.instance()[0], ctx.instance()[1])
    w2 = [rng.randrange(P) for _ in range(NV)]
    x2 = [rng.randrange(P) for _ in range(NIO)]
    outs = []
    for c in (ctx, ctx3):
        c.begin(B.to_mont(P, w2), B.to_mont(P, x2))
        c.finish(B.to_mont(P, [12345]))
        outs.append(c.read())
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    for c in (ctx, ctx2, ctx3):
        c.close()


def test_transcript_calls_and_grumpkin_are_refused_by_name(setup):
    L, mats, shape, key, pts, rng = setup
    ctx = L.FoldingContext(B.CURVE_BN254, shape, key)
    w2, x2 = B.to_mont(P, [1] * NV), B.to_mont(P, [2] * NIO)
    for call in (lambda: ctx.set_pp_digest(0xABCDEF), lambda: ctx.step(w2, x2, 0xABCDEF)):
        with pytest.raises(L.LurkHipError, match="BN254"):
            call()
    cw, ct = ctx.begin(w2, x2)
    with pytest.raises(L.LurkHipError, match="BN254"):
        ctx.challenge()
    ctx.finish(B.to_mont(P, [5]))  # a following valid call works: the step is still open and closes
    assert B.from_mont(P, ctx.read()[0])[:NV] == [5] * NV
    ctx.close()
    with pytest.raises(L.LurkHipError, match="Grumpkin"):
        L.FoldingContext(B.CURVE_GRUMPKIN, shape, key)
    gk = L.CommitmentKey(B.CURVE_GRUMPKIN, B.affine_bases(B.GRUMPKIN, B.GRUMPKIN.synth_bases(4)))
    with pytest.raises(L.LurkHipError, match="Grumpkin"):
        L.FoldingContext(B.CURVE_BN254, shape, gk)
    gk.close()
