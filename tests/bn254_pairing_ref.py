"""CPU reference for the BN254 pairing-product check (include/lurk_hip.h, "the BN254 pairing check"): Python integers only, and built
DIFFERENTLY from lurk_beta_amd/csrc/bn254_pairing.hpp on purpose, so that agreement means something:

    product                                          this reference
    tower Fq2 / Fq6 / Fq12                           Fq12 = Fp[w]/(w^12 - 18 w^6 + 82), twelve integers; a + b u -> (a - 9 b) + b w^6
    optimal ate: loop over 6x + 2, Frobenius lines   the plain ate pairing: loop over T = t - 1 = 6 x^2, no Frobenius step
    sparse line (three coefficients)                 the chord's equation written out in Fq12 on the untwisted points (x w^2, y w^3)
    final exponentiation split easy / hard           one pow by (p^12 - 1) / r

Both are non-degenerate bilinear pairings on G1 x G2, so the DECISION prod e(P_i, Q_i) == 1 is the same; the values in GT are not.
G1 points are (x, y) tuples / None (tests/bn254_ref.py), G2 points ((x0, x1), (y0, y1)) / None on the twist y^2 = x^3 + 3/(9 + u)."""
from tests import bn254_ref as BN

X = 4965661367192848881  # the BN parameter
P = 36 * X**4 + 36 * X**3 + 24 * X**2 + 6 * X + 1
R = 36 * X**4 + 36 * X**3 + 18 * X**2 + 6 * X + 1
ATE_T = 6 * X * X  # the trace minus one
HARD_EXPONENT = (P**4 - P**2 + 1) // R
FINAL_EXPONENT = (P**12 - 1) // R


# ---- Fq2 = Fp[u]/(u^2 + 1), pairs of integers ------------------------------------------------------------------------------------------
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2_sqrt(a):
    """a square root of a in Fq2, or None (p = 3 mod 4: through the norm)"""
    fp_sqrt = lambda v: (lambda s: s if s * s % P == v % P else None)(pow(v, (P + 1) // 4, P))
    if a[1] == 0:
        s = fp_sqrt(a[0])
        if s is not None:
            return (s, 0)
        s = fp_sqrt(-a[0] % P)
        return None if s is None else (0, s)
    s = fp_sqrt((a[0] * a[0] + a[1] * a[1]) % P)
    if s is None:
        return None
    half = pow(2, -1, P)
    for t in ((a[0] + s) * half % P, (a[0] - s) * half % P):
        x0 = fp_sqrt(t)
        if x0:
            r = (x0, a[1] * pow(2 * x0, -1, P) % P)
            if f2_mul(r, r) == (a[0] % P, a[1] % P):
                return r
    return None


XI = (9, 1)
B_TWIST = f2_mul((3, 0), f2_inv(XI))
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


# ---- G2: affine on the twist -----------------------------------------------------------------------------------------------------------
def g2_on_twist(q):
    if q is None:
        return True
    x, y = q
    return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), B_TWIST)


def g2_neg(q):
    return None if q is None else (q[0], f2_sub((0, 0), q[1]))


def _slope(a, b):
    """the slope of the line through a and b (the tangent when they are equal), or None when it is vertical"""
    if a[0] == b[0]:
        if a[1] != b[1] or a[1] == (0, 0):
            return None
        xx = f2_mul(a[0], a[0])
        return f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(a[1], a[1])))
    return f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    lam = _slope(a, b)
    if lam is None:
        return None
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), a[0]), b[0])
    return (x3, f2_sub(f2_mul(lam, f2_sub(a[0], x3)), a[1]))


def g2_mul(k, q):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = g2_add(acc, acc)
        if bit == "1":
            acc = g2_add(acc, q)
    return acc


def g2_in_subgroup(q):
    return g2_on_twist(q) and g2_mul(R, q) is None


def g2_outside_subgroup():
    """A point on the twist that is not in the order-r subgroup: the first x = (k, 1), k = 0, 1, ..., for which x^3 + 3/xi is a square.
    The twist has (2p - r) r points, so a point found this way is outside with overwhelming probability; the caller asserts it."""
    for k in range(1000):
        x = (k, 1)
        y = f2_sqrt(f2_add(f2_mul(f2_mul(x, x), x), B_TWIST))
        if y is not None:
            return (x, y)
    raise AssertionError("no twist point found")


# ---- Fq12 = Fp[w]/(w^12 - 18 w^6 + 82): lists of twelve integers ---------------------------------------------------------------------------
def f12_mul(a, b):
    t = [0] * 23
    for i, ai in enumerate(a):
        if ai:
            for j, bj in enumerate(b):
                t[i + j] += ai * bj
    for k in range(22, 11, -1):  # w^12 = 18 w^6 - 82
        c = t[k]
        if c:
            t[k - 6] += 18 * c
            t[k - 12] -= 82 * c
    return [v % P for v in t[:12]]


F12_ONE = [1] + [0] * 11


def f12_pow(a, e):
    acc = F12_ONE
    for bit in bin(e)[2:]:
        acc = f12_mul(acc, acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


def f12_from_f2(a, shift=0):
    """(a0 + a1 u) w^shift with u = w^6 - 9, shift < 6"""
    out = [0] * 12
    out[shift] = (a[0] - 9 * a[1]) % P
    out[shift + 6] = a[1] % P
    return out


def _line(t, lam, p):
    """The line of slope lam through the twist point t, untwisted to E(Fq12) and evaluated at the G1 point p:
    (yP - yT w^3) - (lam w) (xP - xT w^2) - on E(Fq12) the twist point (x, y) is (x w^2, y w^3) and a slope lam becomes lam w."""
    dy = [(a - b) % P for a, b in zip(f12_from_f2((p[1], 0)), f12_from_f2(t[1], 3))]
    dx = [(a - b) % P for a, b in zip(f12_from_f2((p[0], 0)), f12_from_f2(t[0], 2))]
    m = f12_mul(f12_from_f2(lam, 1), dx)
    return [(a - b) % P for a, b in zip(dy, m)]


def miller_ate(p, q):
    """f_{T, Q}(P) for T = 6 x^2 (vertical lines dropped: they lie in a proper subfield)"""
    f, t = F12_ONE, q
    for bit in bin(ATE_T)[3:]:
        lam = _slope(t, t)
        f = f12_mul(f12_mul(f, f), _line(t, lam, p))
        t = g2_add(t, t)
        if bit == "1":
            lam = _slope(t, q)
            f = f12_mul(f, _line(t, lam, p))
            t = g2_add(t, q)
    return f


def pairing_product_is_one(pairs):
    """pairs: [(P, Q)] with P in G1 and Q in G2 (the caller's promise); an identity on either side contributes 1"""
    f = F12_ONE
    for p, q in pairs:
        if p is not None and q is not None:
            f = f12_mul(f, miller_ate(p, q))
    return f12_pow(f, FINAL_EXPONENT) == F12_ONE
