"""CPU reference for the HyperKZG opening argument over BN254 G1 (include/lurk_hip.h, "HyperKZG"): Python integers and the curve
arithmetic of tests/bn254_ref.py only.

The reference prover knows the trapdoor tau of its own key ck[i] = [tau^i]G, so a commitment is ONE scalar multiple, [P(tau)]G - a
reference proof is cheap at any size - and a proof is accepted iff L == [tau]R in G1: no pairing is needed.  The verifier below is the
one of the header, check for check, with the same failed-check codes."""
from tests import bn254_ref as BN

Q = BN.BN254_R  # the scalar field
CURVE = BN.BN254
ACCEPTED, MALFORMED, FOLD = 0, 1, 2


def fold_pairs(p, x):
    """out[j] = p[2j] + x (p[2j+1] - p[2j]); an element past the end reads as zero"""
    p = list(p) + [0] * (len(p) & 1)
    return [(p[2 * j] + x * (p[2 * j + 1] - p[2 * j])) % Q for j in range(len(p) // 2)]


def poly_eval(c, u, m=Q):
    acc = 0
    for a in reversed(c):
        acc = (acc * u + a) % m
    return acc


def div_linear(c, u, m=Q):
    """(quotient, remainder) of c(X) by (X - u): h_{j-1} = c_j + u h_j"""
    h = [0] * (len(c) - 1)
    acc = 0
    for j in range(len(c) - 1, 0, -1):
        acc = (c[j] + u * acc) % m
        h[j - 1] = acc
    return h, (c[0] + u * acc) % m


def commit_trapdoor(tau, coeffs):
    return CURVE.mul(poly_eval(coeffs, tau), CURVE.gen)


def folds(p0, x):
    """[P_0 .. P_{ell-1}] and y"""
    ell = len(x)
    assert len(p0) == 1 << ell and ell >= 1
    ps = [[v % Q for v in p0]]
    for i in range(ell - 1):
        ps.append(fold_pairs(ps[-1], x[ell - 1 - i]))
    return ps, fold_pairs(ps[-1], x[0])[0]


def prove(tau, p0, x, challenge):
    """challenge(stage, data) -> canonical integer; stage 0: the list of com points, stage 1: the 3 ell scalars (t-major).
    Returns dict(com, v, w, y, r, q) with points as (x, y) tuples / None."""
    ell = len(x)
    ps, y = folds(p0, x)
    com = [commit_trapdoor(tau, p) for p in ps[1:]]
    r = challenge(0, com) % Q
    if r == 0:
        raise ValueError("zero challenge")
    u = [r, (-r) % Q, r * r % Q]
    v = [[poly_eval(p, ut) for p in ps] for ut in u]
    q = challenge(1, [e for row in v for e in row]) % Q
    n = len(p0)
    b = [0] * n
    qp = 1
    for p in ps:
        for j, a in enumerate(p):
            b[j] = (b[j] + qp * a) % Q
        qp = qp * q % Q
    w = []
    for t in range(3):
        h, rem = div_linear(b, u[t])
        assert rem == sum(pow(q, i, Q) * v[t][i] for i in range(ell)) % Q
        w.append(commit_trapdoor(tau, h))
    return {"com": com, "v": v, "w": w, "y": y, "r": r, "q": q}


def pairing_inputs(ell, c, x, y, com, v, w, r, q, d):
    """-> (L, R, accepted, failed_check).  v: three rows of ell scalars."""
    scalars = [y, r, q, d] + list(x) + [e for row in v for e in row]
    pts = [c] + list(com) + list(w)
    if any(not (0 <= s < Q) for s in scalars) or r == 0 or any(not CURVE.on_curve(p) for p in pts) or len(com) != ell - 1:
        return None, None, False, MALFORMED
    for i in range(ell):
        xi = x[ell - 1 - i]
        ynext = v[2][i + 1] if i + 1 < ell else y
        if (2 * r * ynext - (r * (1 - xi) * (v[0][i] + v[1][i]) + xi * (v[0][i] - v[1][i]))) % Q:
            return None, None, False, FOLD
    u = [r, (-r) % Q, r * r % Q]
    bcom = None
    for i, p in enumerate([c] + list(com)):
        bcom = CURVE.add(bcom, CURVE.mul(pow(q, i, Q), p))
    L = R = None
    for t in range(3):
        bt = sum(pow(q, i, Q) * v[t][i] for i in range(ell)) % Q
        term = CURVE.add(CURVE.add(bcom, CURVE.mul((-bt) % Q, CURVE.gen)), CURVE.mul(u[t], w[t]))
        dt = pow(d, t, Q)
        L = CURVE.add(L, CURVE.mul(dt, term))
        R = CURVE.add(R, CURVE.mul(dt, w[t]))
    return L, R, True, ACCEPTED


def trapdoor_holds(tau, L, R):
    return L == CURVE.mul(tau, R)


class Transcript:
    """A deterministic stand-in for the caller's transcript (SHA-256 over the canonical bytes seen so far): the tests' own, no claim of
    compatibility with anything.  Points are absorbed as affine (x, y), the identity as (0, 0)."""

    def __init__(self, seed=b"hyperkzg-test"):
        import hashlib

        self._h = hashlib.sha256(seed)
        self.seen = []

    def _squeeze(self):
        import hashlib

        d = self._h.digest()
        self._h = hashlib.sha256(d)
        return int.from_bytes(d + hashlib.sha256(d + b"2").digest(), "little") % Q

    def __call__(self, stage, data):
        self._h.update(bytes([stage]))
        for e in data:
            if e is None or isinstance(e, tuple):
                xy = (0, 0) if e is None else e
                self._h.update(xy[0].to_bytes(32, "little") + xy[1].to_bytes(32, "little"))
            else:
                self._h.update(int(e).to_bytes(32, "little"))
        c = self._squeeze()
        self.seen.append((stage, c))
        return c
