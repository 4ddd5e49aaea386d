"""CPU reference for the BN254 / Grumpkin cycle: Python big integers only, independent of oracle/'s curve tables.

Short-Weierstrass curves y^2 = x^3 + b with a = 0, parameterised by (p, b, order, generator); affine add / double / scalar multiple;
the synthetic inputs of lurk_hip_synth_* through the generic pieces of oracle/pyref.py (which take the modulus as an argument).
Points are (x, y) tuples, the identity is None; `to_xy` / `from_xy` convert to the (0, 0)-for-identity convention of the C ABI."""
import numpy as np

from oracle import pyref as R

BN254_P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47  # Fq: BN254 base field = Grumpkin scalar field
BN254_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001  # Fr: BN254 scalar field = Grumpkin base field
FIELD_BN254_FR, FIELD_BN254_FQ = 2, 3
CURVE_BN254, CURVE_GRUMPKIN = 2, 3
FIELD_MODULUS = {FIELD_BN254_FR: BN254_R, FIELD_BN254_FQ: BN254_P}


class Curve:
    def __init__(self, cid, name, p, b, order, gen, scalar_field, base_field):
        self.id, self.name, self.p, self.b, self.order, self.gen = cid, name, p, b % p, order, gen
        self.scalar_field, self.base_field = scalar_field, base_field

    def on_curve(self, P):
        return P is None or (P[1] * P[1] - P[0] * P[0] * P[0] - self.b) % self.p == 0

    def neg(self, P):
        return None if P is None else (P[0], (-P[1]) % self.p)

    def add(self, P, Q):
        if P is None:
            return Q
        if Q is None:
            return P
        p = self.p
        if P[0] == Q[0]:
            if (P[1] + Q[1]) % p == 0:
                return None
            lam = 3 * P[0] * P[0] * pow(2 * P[1], -1, p) % p
        else:
            lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
        x = (lam * lam - P[0] - Q[0]) % p
        return x, (lam * (P[0] - x) - P[1]) % p

    def mul(self, k, P):
        """[k]P by Jacobian double-and-add (one inversion at the end: a 254-bit multiple in ~1 ms)"""
        k %= self.order
        if P is None or k == 0:
            return None
        p = self.p
        X, Y, Z = 0, 1, 0
        for bit in bin(k)[2:]:
            if Z:
                A, B = X * X % p, Y * Y % p
                C = B * B % p
                D = 2 * ((X + B) * (X + B) - A - C) % p
                E = 3 * A % p
                X3 = (E * E - 2 * D) % p
                Y3 = (E * (D - X3) - 8 * C) % p
                Z = 2 * Y * Z % p
                X, Y = X3, Y3
            if bit == "1":
                if not Z:
                    X, Y, Z = P[0], P[1], 1
                else:
                    Z2 = Z * Z % p
                    U2, S2 = P[0] * Z2 % p, P[1] * Z2 * Z % p
                    H, r = (U2 - X) % p, (S2 - Y) % p
                    if H == 0:
                        return self._slow_tail(k, P)  # a prefix of k is +/-1 mod the order: not reached for 0 < k < order
                    H2 = H * H % p
                    H3 = H * H2 % p
                    V = X * H2 % p
                    X3 = (r * r - H3 - 2 * V) % p
                    Y = (r * (V - X3) - Y * H3) % p
                    X, Z = X3, Z * H % p
        return self._affine(X, Y, Z)

    def _affine(self, X, Y, Z):
        if not Z:
            return None
        zi = pow(Z, -1, self.p)
        return X * zi * zi % self.p, Y * zi * zi * zi % self.p

    def _slow_tail(self, k, P):
        acc = None
        for bit in bin(k)[2:]:
            acc = self.add(acc, acc)
            if bit == "1":
                acc = self.add(acc, P)
        return acc

    def msm(self, scalars, points):
        acc = None
        for s, P in zip(scalars, points):
            acc = self.add(acc, self.mul(s, P))
        return acc

    # ---- synthetic inputs: the rules of lurk_hip_synth_bases_dev / lurk_hip_synth_scalars_dev ----
    def base_scalar(self, i):
        return R.synth_base_scalar(i, self.order)

    def synth_bases(self, n, first=0):
        return [self.mul(self.base_scalar(first + i), self.gen) for i in range(n)]

    def synth_scalars(self, stream, dist, n, first=0):
        f = R.uniform_fe if dist == 0 else R.witness_like_fe
        return [f(stream, first + i, self.order) for i in range(n)]

    def dlog_checksum(self, scalars, first=0):
        """sum_i s_i P_i for the synthetic bases P_i = [k_i]G as ONE scalar multiple"""
        k = sum(s * self.base_scalar(first + i) for i, s in enumerate(scalars)) % self.order
        return self.mul(k, self.gen)


BN254 = Curve(CURVE_BN254, "BN254", BN254_P, 3, BN254_R, (1, 2), FIELD_BN254_FR, FIELD_BN254_FQ)
GRUMPKIN = Curve(CURVE_GRUMPKIN, "Grumpkin", BN254_R, -17, BN254_P, (1, 0x2CF135E7506A45D632D270D45F1181294833FC48D823F272C), FIELD_BN254_FQ, FIELD_BN254_FR)
CURVES = {CURVE_BN254: BN254, CURVE_GRUMPKIN: GRUMPKIN}


# ---- the C ABI's layouts: 4 x u64 little-endian limbs per field element ----------------------------------------------------
def int_to_limbs(x):
    return [(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def ints_to_limbs(xs):
    return np.array([int_to_limbs(x) for x in xs], dtype=np.uint64).reshape(-1, 4)


def limbs_to_ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def to_mont(p, xs):
    return ints_to_limbs([(x << 256) % p for x in xs])


def from_mont(p, a):
    rinv = pow(1 << 256, -1, p)
    return [x * rinv % p for x in limbs_to_ints(a)]


def affine_bases(curve, points):
    """points -> (n, 8) u64 affine Montgomery records, identity = (0, 0)"""
    flat = []
    for P in points:
        flat += [0, 0] if P is None else [P[0], P[1]]
    return to_mont(curve.p, flat).reshape(-1, 8)


def from_xy(xy):
    return None if tuple(xy) == (0, 0) else tuple(xy)


def jacobian(curve, P):
    """point -> 12 u64 Jacobian Montgomery record with Z = 1 (identity: all zero)"""
    if P is None:
        return np.zeros(12, dtype=np.uint64)
    return to_mont(curve.p, [P[0], P[1], 1]).reshape(12)


# ---- the same synthetic inputs, vectorised (numpy) for the large checksums: 2^22 Python-integer draws would take a minute ------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix_at_np(stream, index):
    """R.splitmix_at for an array of uint64 indices"""
    with np.errstate(over="ignore"):
        s = np.uint64((R.SEED + (stream << 32)) & 0xFFFFFFFFFFFFFFFF) + index * np.uint64(0x9E3779B97F4A7C15)
        z = s + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _ge(a, p):
    """rows of the (n, 4) u64 array a whose 256-bit value is >= p"""
    pl = int_to_limbs(p)
    ge = np.ones(a.shape[0], dtype=bool)
    for k in range(4):  # from the least significant limb up: the most significant difference decides
        ge = np.where(a[:, k] == np.uint64(pl[k]), ge, a[:, k] > np.uint64(pl[k]))
    return ge


def uniform_fe_np(stream, first, n, p):
    """R.uniform_fe(stream, first + i, p) for i < n as an (n, 4) u64 array"""
    idx = np.arange(first, first + n, dtype=np.uint64)
    out = np.zeros((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    retry = 0
    top = np.uint64((1 << (p.bit_length() - 192)) - 1)
    while todo.size:
        with np.errstate(over="ignore"):
            base = idx[todo] * np.uint64(4) + np.uint64((retry << 40) & 0xFFFFFFFFFFFFFFFF)
            v = np.stack([splitmix_at_np(stream, base + np.uint64(w)) for w in range(4)], axis=1)
        v[:, 3] &= top
        bad = _ge(v, p)
        out[todo[~bad]] = v[~bad]
        todo = todo[bad]
        retry += 1
    return out


def base_scalars_np(curve, n, first=0):
    k = uniform_fe_np(0, first, n, curve.order)
    k[(k == 0).all(axis=1), 0] = 1
    return k


def limbs12(x):
    """(n, 4) u64 -> (n, 22) float64: the 12-bit limbs of every 256-bit row"""
    out = np.empty((x.shape[0], 22), dtype=np.float64)
    for j in range(22):
        bit = 12 * j
        w, sh = bit >> 6, bit & 63
        v = x[:, w] >> np.uint64(sh)
        if sh > 52 and w + 1 < 4:
            v = v | (x[:, w + 1] << np.uint64(64 - sh))
        out[:, j] = (v & np.uint64(0xFFF)).astype(np.float64)
    return out


def dot_mod(la, lb, m):
    """sum_i a_i b_i mod m from the 12-bit limbs of both vectors: one float64 matrix product (every entry is a sum of n products below
    2^24: exact in a double up to n = 2^29)"""
    assert la.shape[0] < (1 << 29)
    M = la.T @ lb
    return sum(int(M[i, j]) << (12 * (i + j)) for i in range(22) for j in range(22)) % m


_base_limbs = {}


def dlog_checksum_np(curve, scalars_u64, first=0):
    """the checksum point for canonical scalars given as an (n, 4) u64 array (the base scalars' limbs are computed once per curve
    and prefix length, and shared)"""
    s = np.asarray(scalars_u64, dtype=np.uint64).reshape(-1, 4)
    n = s.shape[0]
    key = (curve.id, first)
    if key not in _base_limbs or _base_limbs[key].shape[0] < n:
        _base_limbs[key] = limbs12(base_scalars_np(curve, n, first))
    return curve.mul(dot_mod(limbs12(s), _base_limbs[key][:n], curve.order), curve.gen)
