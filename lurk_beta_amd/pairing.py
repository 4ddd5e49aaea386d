"""Host-side mirror of the BN254 pairing check (include/lurk_hip.h, "the BN254 pairing check"): G2 multiples and the decision
prod_i e(P_i, Q_i) == 1.  Host code of the library, no device needed.  A G2 point is a (16,) u64 array: affine on the twist,
{x.c0, x.c1, y.c0, y.c1} of four Montgomery limbs each, all-zero for the identity; ``g2_to_ints`` / ``g2_from_ints`` convert to and from
canonical integers ((x0, x1), (y0, y1)), None for the identity.  A G1 point is the 96-byte Jacobian ((12,) u64) of every other module."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

BN254_P = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
BN254_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
_MONT = (1 << 256) % BN254_P
_MONT_INV = pow(_MONT, -1, BN254_P)


def _limbs(v: int) -> np.ndarray:
    return np.array([(v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)], dtype=np.uint64)


def _scalar(k: int) -> np.ndarray:
    k = int(k)
    if k < 0 or k >> 256:
        raise ValueError("a scalar does not fit 32 bytes")
    return _limbs(k)


def g2_from_ints(pt) -> np.ndarray:
    """((x0, x1), (y0, y1)) canonical, or None -> the 128-byte form.  Nothing is checked: the library does that."""
    if pt is None:
        return np.zeros(16, dtype=np.uint64)
    (x0, x1), (y0, y1) = pt
    return np.concatenate([_limbs(int(c) % BN254_P * _MONT % BN254_P) for c in (x0, x1, y0, y1)])


def g2_to_ints(g2):
    a = np.ascontiguousarray(g2, dtype=np.uint64).reshape(4, 4)
    c = [(int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192) * _MONT_INV % BN254_P for r in a]
    return None if not any(c) else ((c[0], c[1]), (c[2], c[3]))


def g2_mul(point, k: int) -> np.ndarray:
    """[k] point as a (16,) u64 array (lurk_hip_bn254_g2_mul); point None = the generator H.  k: a canonical scalar below the group
    order; a point off the twist is refused."""
    out = np.zeros(16, dtype=np.uint64)
    p = None if point is None else np.ascontiguousarray(point, dtype=np.uint64).reshape(16)
    ks = _scalar(k)
    _lib.check(_lib.load().lurk_hip_bn254_g2_mul(_lib.ptr(out), _lib.ptr(p), _lib.ptr(ks)))
    return out


def g2_generator() -> np.ndarray:
    """The generator H of the order-r subgroup of the twist."""
    return g2_mul(None, 1)


def pairing_check(g1_points, g2_points) -> bool:
    """prod_i e(P_i, Q_i) == 1 (lurk_hip_bn254_pairing_check).  g1_points: (n, 12) u64 Jacobians; g2_points: (n, 16) u64.  An identity on
    either side contributes 1; no pairs give True.  A point off its curve, or a G2 point outside the order-r subgroup, is refused
    (``LurkHipError`` naming the index and the reason)."""
    g1 = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, 12)
    g2 = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, 16)
    if g1.shape[0] != g2.shape[0]:
        raise ValueError("as many G1 points as G2 points")
    n = g1.shape[0]
    out = ctypes.c_int(0)
    _lib.check(_lib.load().lurk_hip_bn254_pairing_check(n, _lib.ptr(g1) if n else None, _lib.ptr(g2) if n else None, ctypes.byref(out)))
    return bool(out.value)
