"""GPU: the same rows through every consumer of the shared row product (r1cs_shape.cuh: r1cs_row) - multiply_vec, both cross terms,
is_sat and sparse_mle - each against the C oracle (oracle/coracle.py, oracle/spartan_fast.py), never against another call of the library:
all of them run one row function, and a mistake they shared would cancel out in a comparison among themselves.

One shape of 87 rows x 700 columns whose three matrices have DIFFERENT row lengths (a row that is long in one matrix only is seen by
the cross terms too), around every bound the row function and its callers have: fold.hip's FOLD_LONG (32 / 33, in C only), the class
bounds (8 / 9, 96 / 97), the 64-term re-entry (64 / 65, 129 / 130), the limb-wise / one-by-one switch of a lane group (255 / 256 / 257,
300, 700), rows without an entry.  Coefficients and z are p - 1 in two thirds of their places: the largest terms the lazy accumulation
can meet.  Fields: Pallas Fq and BN254 Fr."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from oracle import spartan_fast as SF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (1, 2)  # Pallas Fq, BN254 Fr
NCOLS, NIO = 700, 2
NV = NCOLS - 1 - NIO
LA = [0, 1, 700, 0, 65, 64, 129, 5, 8, 9, 96, 97, 256, 257, 3] + [4] * 70 + [1, 1]
LB = [0, 2, 3, 1, 8, 300, 1, 66, 9, 8, 1, 2, 255, 1, 0] + [3] * 70 + [1, 1]
LC = [0, 1, 1, 0, 2, 1, 130, 1, 1, 33, 97, 96, 1, 2, 64] + [1] * 70 + [32, 33]
ROWS = len(LA)
BUMPED = 17  # is_sat: the first 17 rows fail one at a time (every edge row, the first of the 4 / 3 / 1 rows after them)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _extreme(f, stream, n, phase=0):
    """n canonical elements, p - 1 in two thirds of the places."""
    p = R.modulus(f)
    return C.ints_to_limbs([p - 1 if (k + phase) % 3 else R.uniform_fe(stream, k, p) for k in range(n)])


@functools.lru_cache(maxsize=None)
def case(f):
    """The matrices (canonical CSR), three z vectors and everything the oracle says about them; computed once per field, read-only."""
    rng = np.random.default_rng(3)

    def matrix(lens, salt):
        indptr = np.zeros(len(lens) + 1, dtype=np.uint64)
        np.cumsum(np.array(lens, dtype=np.uint64), out=indptr[1:])
        nnz = int(indptr[-1])
        return indptr, rng.integers(0, NCOLS, nnz).astype(np.uint64), _extreme(f, 83 + salt, nnz)

    mats = (matrix(LA, 0), matrix(LB, 1), matrix(LC, 2))
    zs = [_extreme(f, 90 + k, NCOLS, phase=(0, 2, 1)[k]) for k in range(3)]  # u = z[NV]: p - 1 in zs[0] and zs[2], uniform in zs[1]
    us = [C.limbs_to_ints(z[NV:NV + 1])[0] for z in zs]
    prods = [[C.spmv(f, *M, z) for M in mats] for z in zs]
    return {"mats": mats, "z": zs, "u": us, "abc": prods}


def _shape(f):
    from lurk_beta_amd import R1CSShape

    assert ROWS == 87 and len(LB) == ROWS and len(LC) == ROWS and ROWS % 64
    return R1CSShape(f, ROWS, NV, NIO, *[(M[0], M[1], C.to_mont(f, M[2])) for M in case(f)["mats"]])


def _canon(f, t):
    return C.from_mont(f, _host(t))


@pytest.mark.parametrize("f", FIELDS)
def test_multiply_vec(hip, f):
    c, sh = case(f), _shape(f)
    for k in range(2):
        got = sh.multiply_vec(_dev(C.to_mont(f, c["z"][k])))
        for w in range(3):
            assert np.array_equal(_canon(f, got[w]), c["abc"][k][w]), (k, w)
    sh.close()


@pytest.mark.parametrize("f", FIELDS)
def test_cross_terms(hip, f):
    import torch

    c, sh = case(f), _shape(f)
    mont = lambda a: C.to_mont(f, a)
    z1, z2 = _dev(mont(c["z"][0])), _dev(mont(c["z"][1]))
    want = C.cross_term(f, *c["abc"][0], *c["abc"][1], c["u"][0], c["u"][1])
    t = sh.cross_term(z1, z2)
    assert np.array_equal(_canon(f, t), want)
    # the cached form: A z1, B z1, C z1 handed in, z2 alone gathered
    abc1 = [_dev(mont(v)) for v in c["abc"][0]]
    t_c, abc2 = sh.cross_term_cached(z2, abc1, mont(C.ints_to_limbs([c["u"][0]])))
    torch.cuda.synchronize()
    assert torch.equal(t_c, t)
    for w in range(3):
        assert np.array_equal(_canon(f, abc2[w]), c["abc"][1][w]), w
        assert np.array_equal(_canon(f, abc1[w]), c["abc"][0][w]), w  # nothing to fold in: the cache is left alone
    # ... with the previous step's products folded into the cache by the same launch: the running instance is z1 + r z3
    r = R.uniform_fe(96, f, R.modulus(f))
    z1f = C.axpy(f, c["z"][0], c["z"][2], r)
    abc1f = [C.axpy(f, c["abc"][0][w], c["abc"][2][w], r) for w in range(3)]
    u1f = C.limbs_to_ints(z1f[NV:NV + 1])[0]
    want_f = C.cross_term(f, *abc1f, *c["abc"][1], u1f, c["u"][1])
    t_f = sh.cross_term(_dev(mont(z1f)), z2)
    assert np.array_equal(_canon(f, t_f), want_f)
    prev = [_dev(mont(v)) for v in c["abc"][2]]
    t_cf, abc2f = sh.cross_term_cached(z2, abc1, mont(C.ints_to_limbs([u1f])), prev=prev, r_prev_mont=mont(C.ints_to_limbs([r])))
    torch.cuda.synchronize()
    assert torch.equal(t_cf, t_f)
    for w in range(3):
        assert np.array_equal(_canon(f, abc2f[w]), c["abc"][1][w]), w
        assert np.array_equal(_canon(f, abc1[w]), abc1f[w]), w  # the cache, folded in place
    sh.close()


def check_is_sat(f):
    """E := the oracle's residual of z satisfies every row; one more on row i fails row i alone."""
    c, sh = case(f), _shape(f)
    p = R.modulus(f)
    z = _dev(C.to_mont(f, c["z"][0]))
    e = C.limbs_to_ints(C.relaxed_residual(f, *c["abc"][0], c["u"][0], np.zeros((ROWS, 4), dtype=np.uint64)))
    assert any(e) and sh.is_sat(z, _dev(C.to_mont(f, C.ints_to_limbs(e)))) == (0, ROWS)
    for i in range(BUMPED):
        e2 = list(e)
        e2[i] = (e2[i] + 1) % p
        assert sh.is_sat(z, _dev(C.to_mont(f, C.ints_to_limbs(e2)))) == (1, i), i
    sh.close()


@pytest.mark.parametrize("f", FIELDS)
def test_is_sat(hip, f):
    check_is_sat(f)


CHILD = r'''
import sys
sys.path.insert(0, %r)
from tests import test_gpu_r1cs_rows as T
for f in T.FIELDS:
    T.check_is_sat(f)
print("child ok")
'''


@pytest.mark.parametrize("env", [{"LURK_SAT_GROUP": "4"}, {"LURK_SAT_GROUP": "8"}, {"LURK_SAT_GROUP": "16"}, {"LURK_SAT_LDS": "1"}])
def test_is_sat_under_its_measurement_switches(hip, env):
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stderr[-2000:]


@pytest.mark.parametrize("f", FIELDS)
def test_sparse_mle(hip, f):
    c, sh = case(f), _shape(f)
    q = R.modulus(f)
    tables = [(C.synth_scalars(f, 41, 0, ROWS), C.synth_scalars(f, 42, 0, NCOLS)),
              (np.tile(C.ints_to_limbs([q - 1]), (ROWS, 1)), np.tile(C.ints_to_limbs([q - 1]), (NCOLS, 1)))]
    for ex, ey in tables:
        got = C.limbs_to_ints(C.from_mont(f, sh.sparse_mle(_dev(C.to_mont(f, ex)), _dev(C.to_mont(f, ey)))))
        assert got == [SF.sparse_mle(f, M, np.ascontiguousarray(ex), np.ascontiguousarray(ey)) for M in c["mats"]]
    sh.close()
