"""Folding on Grumpkin, the secondary curve of the BN254 cycle: shapes over the BN254 base field (R1CSShape.for_curve) through the
shape-keyed kernels, and the folding context with the caller's r, bit for bit against Python integers - spmv / cross_term / axpy of
oracle/pyref.py (generic over the modulus), the curve and the commitment checks of tests/bn254_ref.py.  Needs an MI355X."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import bn254_ref as B

pytestmark = pytest.mark.gpu

C = B.GRUMPKIN
P = B.BN254_P  # the circuit field: Grumpkin's scalar field, the BN254 base field
assert C.order == P
M, NV, NIO = 96, 80, 2
NCOLS = NV + 1 + NIO
# row lengths at every class boundary of the kernels (FOLD_LONG = 32: 33 entries in A, B or C send a row to the 16-lane walk; the
# satisfiability classes end at 8 and 96 entries; a group adds partial sums limb-wise up to 256 entries); matrix w sees the table
# shifted by 11 w rows, so that a row is long in one matrix and short or empty in the others.  Row 0 is empty in all three.
SPECIAL = {3: 0, 7: 32, 8: 33, 9: 40, 20: 255, 31: 8, 32: 9, 40: 1, 41: 2, 42: 3}


def _dev(ints):
    import torch

    return torch.from_numpy(B.to_mont(P, ints).view(np.int64)).cuda()


def _host(t):
    return B.from_mont(P, t.cpu().numpy().view(np.uint64))


def _matrix(rng, w):
    indptr, indices, data = [0], [], []
    for i in range(M):
        k = 0 if i == 0 else SPECIAL.get((i + 11 * w) % M, rng.randrange(0, 4))
        cols = sorted(rng.randrange(NCOLS) for _ in range(k))  # more entries than columns: a column may repeat
        indices += cols
        if k == 255:  # the worst case of the lazy sums: the largest coefficient on the longest row
            data += [P - 1] * k
        else:
            data += [rng.choice([1, 2, P - 1, rng.randrange(1, P)]) for _ in cols]
        indptr.append(len(indices))
    return indptr, indices, data


@pytest.fixture(scope="module")
def setup(hip):
    import lurk_beta_amd as L

    rng = random.Random("grumpkin-fold")
    mats = [_matrix(rng, w) for w in range(3)]
    shape = L.R1CSShape.for_curve(B.CURVE_GRUMPKIN, M, NV, NIO, *[(ip, ix, B.to_mont(P, d)) for ip, ix, d in mats])
    pts = C.synth_bases(max(M, NV))
    yield L, mats, shape, pts, rng
    shape.close()


def test_shape_reports_the_fourth_field_and_reads_back(setup):
    L, mats, shape, pts, rng = setup
    assert shape.field_id == B.FIELD_BN254_FQ == 3 and (shape.num_cons, shape.num_vars, shape.num_io) == (M, NV, NIO)
    assert shape.info()["nnz"] == tuple(len(m[1]) for m in mats)
    for w, (ip, ix, d) in enumerate(mats):
        gip, gix, gd = shape.read(w)
        assert list(gip) == ip and list(gix) == ix and B.from_mont(P, gd) == d, w


def test_shape_kernels_against_python_integers(setup, hip):
    from lurk_beta_amd import _lib

    L, mats, shape, pts, rng = setup
    abc = lambda z: [R.spmv(P, *m, z) for m in mats]
    z_rand = [rng.randrange(P) for _ in range(NCOLS)]
    z_rand2 = [rng.randrange(P) for _ in range(NCOLS)]
    z_worst = [P - 1] * NCOLS  # with the coefficient p - 1 on the 255-entry row: every term of every lazy sum is (p - 1)^2
    want = {id(z): abc(z) for z in (z_rand, z_rand2, z_worst)}
    for z in (z_rand, z_worst):
        got = shape.multiply_vec(_dev(z))
        assert [_host(g) for g in got] == want[id(z)]
    # the host-pointer forms (the C++ mirror's calls)
    out = [np.zeros((M, 4), dtype=np.uint64) for _ in range(3)]
    zm = B.to_mont(P, z_worst)
    assert hip.lurk_hip_r1cs_multiply_vec(shape._h, _lib.ptr(zm), *[_lib.ptr(o) for o in out]) == 0
    assert [B.from_mont(P, o) for o in out] == want[id(z_worst)]
    for z1, z2 in ((z_rand, z_rand2), (z_worst, z_worst), (z_rand, z_worst)):
        t = R.cross_term(P, *want[id(z1)], *want[id(z2)], z1[NV], z2[NV])
        assert _host(shape.cross_term(_dev(z1), _dev(z2))) == t
        # the cached form: from (A z1, B z1, C z1) and z2 alone
        abc1 = [_dev(v) for v in want[id(z1)]]
        tc, abc2 = shape.cross_term_cached(_dev(z2), abc1, B.to_mont(P, [z1[NV]]))
        assert _host(tc) == t and [_host(v) for v in abc2] == want[id(z2)]
        # ... with the previous step's products folded into the cache by the same launch: cache <- cache + r prev
        r = rng.randrange(P)
        prev = [_dev(v) for v in want[id(z_rand2)]]
        folded = [R.axpy(P, a, b, r) for a, b in zip(want[id(z1)], want[id(z_rand2)])]
        u1 = rng.randrange(P)
        t_f = R.cross_term(P, *folded, *want[id(z2)], u1, z2[NV])
        tc, _ = shape.cross_term_cached(_dev(z2), abc1, B.to_mont(P, [u1]), prev=prev, r_prev_mont=B.to_mont(P, [r]))
        assert _host(tc) == t_f and [_host(v) for v in abc1] == folded
    t_host = np.zeros((M, 4), dtype=np.uint64)
    assert hip.lurk_hip_r1cs_cross_term(shape._h, _lib.ptr(B.to_mont(P, z_rand)), _lib.ptr(zm), _lib.ptr(t_host)) == 0
    assert B.from_mont(P, t_host) == R.cross_term(P, *want[id(z_rand)], *want[id(z_worst)], z_rand[NV], z_worst[NV])
    # is_sat: a relaxed pair that holds by construction, E = Az o Bz - u Cz; then one E entry changed
    for z in (z_rand, z_worst):
        az, bz, cz = want[id(z)]
        e = [(a * b - z[NV] * c) % P for a, b, c in zip(az, bz, cz)]
        assert shape.is_sat(_dev(z), _dev(e)) == (0, M)
        for row in (0, 8, 20, M - 1):  # an empty row, a long one, the 255-entry one, the last
            bad = list(e)
            bad[row] = (bad[row] + 1) % P
            assert shape.is_sat(_dev(z), _dev(bad)) == (1, row)
    assert shape.is_sat(_dev(z_rand))[0] > 0  # E = 0: a random z is no strict instance


def _model(mats, pts, rng):
    """three steps in Python integers: per step (w2, x2, r, comm_W2, comm_T) and the running pair / instance after it"""
    z1, e1, u1 = [0] * NCOLS, [0] * M, 0
    cw1 = ce1 = None
    abc = lambda z: [R.spmv(P, *m, z) for m in mats]
    steps = []
    for _ in range(3):
        w2 = [rng.randrange(P) for _ in range(NV)]
        x2 = [rng.randrange(P) for _ in range(NIO)]
        r = rng.randrange(1 << 128)
        z2 = w2 + [1] + x2
        t = R.cross_term(P, *abc(z1), *abc(z2), u1, 1)
        want_cw, want_ct = C.msm(w2, pts[:NV]), C.msm(t, pts[:M])
        z1, e1, u1 = R.axpy(P, z1, z2, r), R.axpy(P, e1, t, r), (u1 + r) % P
        cw1, ce1 = C.add(cw1, C.mul(r, want_cw)), C.add(ce1, C.mul(r, want_ct))
        steps.append(dict(w2=w2, x2=x2, r=r, cw=want_cw, ct=want_ct, z=z1, e=e1, u=u1, icw=cw1, ice=ce1))
    return steps


@pytest.fixture(scope="module")
def model(setup):
    L, mats, shape, pts, rng = setup
    return _model(mats, pts, random.Random("grumpkin-fold-steps"))


@pytest.mark.parametrize("table_key", [False, True], ids=["plain-key", "window-table-key"])
def test_three_steps_and_a_staged_one(setup, model, table_key, monkeypatch):
    L, mats, shape, pts, rng = setup
    kw = dict(precompute=True, window_bits=16) if table_key else {}
    key = L.CommitmentKey(B.CURVE_GRUMPKIN, B.affine_bases(C, pts), **kw)
    aff = lambda jac: B.from_xy(L.point_to_affine(B.CURVE_GRUMPKIN, jac))
    monkeypatch.setenv("LURK_FOLD_CACHED_PRODUCTS", "0")  # read when a context is created: the six-gather cross term
    ctx6 = L.FoldingContext(B.CURVE_GRUMPKIN, shape, key)
    monkeypatch.delenv("LURK_FOLD_CACHED_PRODUCTS")
    for k, s in enumerate(model):
        cw, ct = ctx6.begin(B.to_mont(P, s["w2"]), B.to_mont(P, s["x2"]))
        assert aff(cw) == s["cw"] and aff(ct) == s["ct"], k
        ctx6.finish(B.to_mont(P, [s["r"]]))
    gz6, ge6 = ctx6.read()
    assert B.from_mont(P, gz6) == model[-1]["z"] and B.from_mont(P, ge6) == model[-1]["e"]
    ctx6.close()
    ctx = L.FoldingContext(B.CURVE_GRUMPKIN, shape, key)  # the default: the running products cached
    ctx2 = L.FoldingContext(B.CURVE_GRUMPKIN, shape, key)  # the same steps, the last one staged
    for k, s in enumerate(model):
        cw, ct = ctx.begin(B.to_mont(P, s["w2"]), B.to_mont(P, s["x2"]))
        assert aff(cw) == s["cw"] and aff(ct) == s["ct"], k
        ctx.finish(B.to_mont(P, [s["r"]]))
        gz, ge = ctx.read()
        assert B.from_mont(P, gz) == s["z"] and B.from_mont(P, ge) == s["e"], k
        icw, ice, iu, ix = ctx.instance()
        assert aff(icw) == s["icw"] and aff(ice) == s["ice"], k
        assert B.from_mont(P, iu) == [s["u"]] and B.from_mont(P, ix) == s["z"][NV + 1:], k
    for s in model[:2]:
        ctx2.begin(B.to_mont(P, s["w2"]), B.to_mont(P, s["x2"]))
        ctx2.finish(B.to_mont(P, [s["r"]]))
    s = model[2]
    late = 7  # the last 7 witness values arrive with the step
    ctx2.prefetch(B.to_mont(P, s["w2"][:NV - late]), 0)
    cw, ct = ctx2.begin_prefetched(B.to_mont(P, s["x2"]), patches=[(NV - late, B.to_mont(P, s["w2"][NV - late:]))])
    assert aff(cw) == s["cw"] and aff(ct) == s["ct"]
    ctx2.finish(B.to_mont(P, [s["r"]]))
    gz2, ge2 = ctx2.read()
    gz, ge = ctx.read()
    assert np.array_equal(gz, gz2) and np.array_equal(ge, ge2)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.instance(), ctx2.instance()))
    # set_running: a third context adopts the running pair and folds one more step like the first
    ctx3 = L.FoldingContext(B.CURVE_GRUMPKIN, shape, key)
    ctx3.set_running(gz, ge, ctx.instance()[0], ctx.instance()[1])
    w2 = [(7 * i + 3) % P for i in range(NV)]
    x2 = [P - 1, 5]
    z2 = w2 + [1] + x2
    abc = lambda z: [R.spmv(P, *m, z) for m in mats]
    t = R.cross_term(P, *abc(s["z"]), *abc(z2), s["u"], 1)
    outs = []
    for c in (ctx, ctx3):
        c.begin(B.to_mont(P, w2), B.to_mont(P, x2))
        c.finish(B.to_mont(P, [12345]))
        outs.append(c.read())
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert B.from_mont(P, outs[1][0]) == R.axpy(P, s["z"], z2, 12345) and B.from_mont(P, outs[1][1]) == R.axpy(P, s["e"], t, 12345)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.instance(), ctx3.instance()))
    for c in (ctx, ctx2, ctx3):
        c.close()
    key.close()


# ---- the secondary circuit's own size ---------------------------------------------------------------------------------------------
BM, BNV, BNIO = 10240, 9000, 2
FREE, PROD = 2000, 7000  # free witness values; rows i < PROD define witness FREE + i as a product


def _secondary_shape(rng):
    """A satisfiable circuit of the secondary's size: row i < PROD is (A_i z)(B_i z) = w[FREE + i] over earlier columns (every 64th row
    long: 40 entries in A), the rest are linear rows (A_i z) u = u (A_i z) written with B = u's column and C = A."""
    u_col = BNV
    A, Bm, Cm = ([0], [], []), ([0], [], []), ([0], [], [])
    coeff = lambda: rng.choice([1, 1, 2, P - 1, rng.randrange(1, P)])

    def push(m, cols):
        m[1].extend(cols)
        m[2].extend(coeff() for _ in cols)
        m[0].append(len(m[1]))

    for i in range(BM):
        if i < PROD:
            known = FREE + i  # the columns whose values are known by now: the witness so far, then u and X
            pick = lambda k: sorted(c if c < known else u_col + c - known for c in rng.sample(range(known + 1 + BNIO), k))
            push(A, pick(40 if i % 64 == 0 else rng.randrange(1, 4)))
            push(Bm, pick(rng.randrange(1, 4)))
            Cm[1].append(FREE + i)
            Cm[2].append(1)
            Cm[0].append(len(Cm[1]))
        else:
            cols = sorted(rng.sample(range(BNV), 40 if i % 64 == 0 else rng.randrange(1, 4)))
            vals = [coeff() for _ in cols]
            for m in (A, Cm):
                m[1].extend(cols)
                m[2].extend(vals)
                m[0].append(len(m[1]))
            Bm[1].append(u_col)
            Bm[2].append(1)
            Bm[0].append(len(Bm[1]))
    return A, Bm, Cm


def _secondary_witness(mats, rng):
    A, Bm, Cm = mats
    x2 = [rng.randrange(P) for _ in range(BNIO)]
    z = [rng.randrange(P) for _ in range(FREE)] + [0] * (BNV - FREE) + [1] + x2
    row = lambda m, i: sum(m[2][k] * z[m[1][k]] for k in range(m[0][i], m[0][i + 1])) % P
    for i in range(PROD):
        z[FREE + i] = row(A, i) * row(Bm, i) % P
    return z[:BNV], x2


def test_two_steps_at_the_secondary_circuits_size(hip):
    import lurk_beta_amd as L
    from lurk_beta_amd import synth

    rng = random.Random("grumpkin-secondary")
    mats = _secondary_shape(rng)
    shape = L.R1CSShape.for_curve(B.CURVE_GRUMPKIN, BM, BNV, BNIO, *[(ip, ix, B.to_mont(P, d)) for ip, ix, d in mats])
    n = max(BM, BNV)
    key = L.CommitmentKey(B.CURVE_GRUMPKIN, synth.bases(B.CURVE_GRUMPKIN, n), n=n, device=True)
    aff = lambda jac: B.from_xy(L.point_to_affine(B.CURVE_GRUMPKIN, jac))
    ctx = L.FoldingContext(B.CURVE_GRUMPKIN, shape, key)
    abc = lambda z: [R.spmv(P, *m, z) for m in mats]
    z1, e1, u1 = [0] * (BNV + 1 + BNIO), [0] * BM, 0
    abc1 = abc(z1)
    for step in range(2):
        w2, x2 = _secondary_witness(mats, rng)
        z2 = w2 + [1] + x2
        abc2 = abc(z2)
        assert all(a * b % P == c for a, b, c in zip(*abc2))  # the fresh instance is a strict one
        r = rng.randrange(1 << 128)
        t = R.cross_term(P, *abc1, *abc2, u1, 1)
        cw, ct = ctx.begin(B.to_mont(P, w2), B.to_mont(P, x2))
        assert aff(cw) == B.dlog_checksum_np(C, B.ints_to_limbs(w2)), step
        assert aff(ct) == B.dlog_checksum_np(C, B.ints_to_limbs(t)), step
        ctx.finish(B.to_mont(P, [r]))
        z1, e1, u1 = R.axpy(P, z1, z2, r), R.axpy(P, e1, t, r), (u1 + r) % P
        abc1 = [R.axpy(P, a, b, r) for a, b in zip(abc1, abc2)]
    gz, ge = ctx.read()
    assert B.from_mont(P, gz) == z1 and B.from_mont(P, ge) == e1
    import torch

    d_z, d_e = torch.from_numpy(gz.view(np.int64)).cuda(), torch.from_numpy(ge.view(np.int64)).cuda()
    assert shape.is_sat(d_z, d_e) == (0, BM)  # the folded pair is a relaxed instance of the shape
    ge[BM - 1, 0] ^= np.uint64(1)
    assert shape.is_sat(d_z, torch.from_numpy(ge.view(np.int64)).cuda()) == (1, BM - 1)
    ctx.close()
    key.close()
    shape.close()


def test_refusals_name_the_curve_or_the_field_and_leave_everything_usable(setup, hip):
    import torch

    L, mats, shape, pts, rng = setup
    csr = [(ip, ix, B.to_mont(P, d)) for ip, ix, d in mats]
    gk = L.CommitmentKey(B.CURVE_GRUMPKIN, B.affine_bases(C, pts))
    bk = L.CommitmentKey(B.CURVE_BN254, B.affine_bases(B.BN254, B.BN254.synth_bases(4)))
    ident = B.to_mont(B.BN254_R, [1, 1])
    fr_shape = L.R1CSShape(B.FIELD_BN254_FR, 2, 2, 0, *[([0, 1, 2], [0, 1], ident)] * 3)
    w2, x2 = B.to_mont(P, [1] * NV), B.to_mont(P, [2] * NIO)

    def valid():  # a step on a fresh Grumpkin context: W <- 5 W2
        c = L.FoldingContext(B.CURVE_GRUMPKIN, shape, gk)
        c.begin(w2, x2)
        c.finish(B.to_mont(P, [5]))
        assert B.from_mont(P, c.read()[0])[:NV] == [5] * NV
        c.close()

    with pytest.raises(L.LurkHipError, match="unknown curve id"):
        L.R1CSShape.for_curve(7, M, NV, NIO, *csr)
    valid()
    # the field-id calls keep refusing the fourth field: only for_curve makes such a shape, only a context folds over it
    with pytest.raises(L.LurkHipError, match="unknown field id"):
        L.R1CSShape(B.FIELD_BN254_FQ, M, NV, NIO, *csr)
    d = torch.zeros((4, 4), dtype=torch.int64, device="cuda")
    for call in (lambda: L.fold_vecs(B.FIELD_BN254_FQ, [(d, d)], B.to_mont(P, [1])), lambda: L.fold_vec(B.FIELD_BN254_FQ, d, d, B.to_mont(P, [1]))):
        with pytest.raises(L.LurkHipError, match="unknown field id"):
            call()
    valid()
    # a shape over Fq under a BN254 key: the field is named; under a BN254 key on Grumpkin: the key's curve is
    with pytest.raises(L.LurkHipError, match="BN254 base field"):
        L.FoldingContext(B.CURVE_BN254, shape, bk)
    with pytest.raises(L.LurkHipError, match="Grumpkin"):
        L.FoldingContext(B.CURVE_GRUMPKIN, shape, bk)
    # a shape over Fr under a Grumpkin key, curve Grumpkin
    with pytest.raises(L.LurkHipError, match="BN254 scalar field.*Grumpkin"):
        L.FoldingContext(B.CURVE_GRUMPKIN, fr_shape, gk)
    valid()
    # the transcript calls: no random oracle over Grumpkin's base field; the open step stays open and closes
    ctx = L.FoldingContext(B.CURVE_GRUMPKIN, shape, gk)
    for call in (lambda: ctx.set_pp_digest(0xABCDEF), lambda: ctx.step(w2, x2, 0xABCDEF)):
        with pytest.raises(L.LurkHipError, match="Grumpkin"):
            call()
    ctx.begin(w2, x2)
    with pytest.raises(L.LurkHipError, match="Grumpkin"):
        ctx.challenge()
    ctx.finish(B.to_mont(P, [5]))
    assert B.from_mont(P, ctx.read()[0])[:NV] == [5] * NV
    ctx.close()
    # everything downstream of a transpose is refused for a shape over Fq, with nothing launched
    with pytest.raises(L.LurkHipError, match="BN254 base field"):
        shape.transposed()
    eq = torch.zeros((128, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(L.LurkHipError):
        shape.sparse_mle(eq, eq)
    valid()
    z = [rng.randrange(P) for _ in range(NCOLS)]
    assert [_host(g) for g in shape.multiply_vec(_dev(z))] == [R.spmv(P, *m, z) for m in mats]
    for h in (gk, bk, fr_shape):
        h.close()
