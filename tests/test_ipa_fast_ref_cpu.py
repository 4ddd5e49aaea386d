"""CPU-only: tests/ipa_fast_ref.py (the proof from Python-integer scalars and commitments under the original key) is the oracle's
ipa_prove (which folds the key point by point) wherever both can run - the GPU tests use the fast form at 2^13."""
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import ipa_fast_ref as F


@pytest.mark.parametrize("cn,c", [("pallas", 0), ("vesta", 1)])
@pytest.mark.parametrize("log_n", [1, 2, 4])
def test_fast_reference_is_the_oracles_proof(cn, c, log_n):
    sf, bf = (1, 0) if c == 0 else (0, 1)
    q = R.CURVES[cn]["order"]
    n = 1 << log_n
    B = C.synth_bases(c, n + 1)
    pts = [tuple(C.limbs_to_ints(C.from_mont(bf, B[i].reshape(2, 4)))) for i in range(n + 1)]
    a = C.limbs_to_ints(C.synth_scalars(sf, 160, 1, n))
    b = C.limbs_to_ints(C.synth_scalars(sf, 161, 0, n))
    a[0], b[n - 1] = q - 1, 0
    r0 = R.uniform_fe(162, 0, q)
    chal = [R.uniform_fe(163, j, q) for j in range(log_n)]
    assert F.ipa_prove(c, B, a, b, r0, chal) == R.ipa_prove(cn, pts[:n], pts[n], a, b, r0, chal)


def test_limbs_are_the_oracles():
    vals = [0, 1, (1 << 256) - 1, R.PALLAS_Q - 1, 1 << 64, (1 << 192) + 5]
    assert (F.limbs(vals) == C.ints_to_limbs(vals)).all()
