"""The inner-product argument's proof at sizes where oracle/pyref.py: ipa_prove is unusable (it folds the key with Python point
arithmetic: n/2 double scalar multiples per round).

Everything scalar is Python integers: the folds of a and b, the cross inner products c_L and c_R, and the coefficient vector
coef_k[i] = the product of the fold weights the original key element i met in the first k rounds.  The folded key of round k is
ck_k[p] = sum over i = p mod m (m = n / 2^k) of coef_k[i] ck[i], so every point of the proof is a commitment under the ORIGINAL key:
    L_j    = sum_{i : (i mod m) >= m/2} a[(i mod m) - m/2] coef_j[i] ck[i] + c_L ck_c'
    R_j    = sum_{i : (i mod m) <  m/2} a[(i mod m) + m/2] coef_j[i] ck[i] + c_R ck_c'
    ck_hat = sum_i coef_last[i] ck[i],          ck_c' = r0 ck_c
computed by the oracle's C Pippenger (oracle.c: orc_msm_pippenger), the extra base as one more term of the same sum.
tests/test_ipa_fast_ref_cpu.py pins this against ipa_prove at the sizes both can run."""
import numpy as np

from oracle import coracle as C
from oracle import pyref as R


def limbs(vals):
    """Python integers below 2^256 -> (n, 4) u64 limbs (C.ints_to_limbs without its per-limb loop)."""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def _commit(curve, bases, scalars):
    xy = C.jac_to_affine(curve, C.msm_pippenger(curve, bases, limbs(scalars)))
    return None if xy == (0, 0) else xy


def ipa_prove(curve, bases, a, b, r0, challenges):
    """curve: 0 Pallas, 1 Vesta.  bases: (n + 1, 8) u64 affine Montgomery points, the key's n elements and then the extra base ck_c
    (C.synth_bases' layout); a, b, r0, challenges: integers.  Returns what R.ipa_prove returns: (L_vec, R_vec, a_hat, ck_hat) with
    points as canonical affine (x, y) tuples, None for the identity."""
    q = R.CURVES["pallas" if curve == 0 else "vesta"]["order"]
    n = len(a)
    assert len(b) == n and n & (n - 1) == 0 and len(challenges) == n.bit_length() - 1 and bases.shape[0] == n + 1
    bases = np.ascontiguousarray(bases, dtype=np.uint64)
    a, b = [x % q for x in a], [x % q for x in b]
    coef = [1] * n
    Ls, Rs = [], []
    m = n
    for r in challenges:
        h = m // 2
        c_l = sum(x * y for x, y in zip(a[:h], b[h:])) % q
        c_r = sum(x * y for x, y in zip(a[h:], b[:h])) % q
        l, rr = [0] * n, [0] * n
        for i in range(n):
            p = i & (m - 1)
            if p >= h:
                l[i] = a[p - h] * coef[i] % q
            else:
                rr[i] = a[p + h] * coef[i] % q
        Ls.append(_commit(curve, bases, l + [c_l * r0 % q]))
        Rs.append(_commit(curve, bases, rr + [c_r * r0 % q]))
        ri = pow(r, q - 2, q)
        a = [(x * r + ri * y) % q for x, y in zip(a[:h], a[h:])]
        b = [(x * ri + r * y) % q for x, y in zip(b[:h], b[h:])]
        coef = [c * (r if (i & (m - 1)) >= h else ri) % q for i, c in enumerate(coef)]  # ck' = [r^-1] ck_L + [r] ck_R
        m = h
    return Ls, Rs, a[0], _commit(curve, bases[:n], coef)
