"""Operands at the edges of the field multipliers' carry patterns, shared by the asm emulator test and the GPU arithmetic test.

Random operands almost never produce limbs of 0xFFFFFFFF, p - 1 or radix-2^29 limbs at the very edge of their contract, where a
column-wise multiplier breaks; these lists do."""
import random

from oracle import pyref as R

FIELDS = {"PallasFp": 0, "PallasFq": 1, "Bn254Fr": 2}
W29, MASK29 = 29, (1 << 29) - 1


def modulus(field):
    return R.modulus(FIELDS[field])


def _limbs_int(limbs, w=32):
    return sum(x << (w * i) for i, x in enumerate(limbs))


def structured(field):
    """~40 canonical values (< p): small values, p - small, halves, powers of two, the largest 2^k - 1 below p, the Montgomery
    constants and 8 x 32 limb patterns of 0xFFFFFFFF / 0x80000000 / 0 (each reduced below p)."""
    p = modulus(field)
    nbits = R.FIELD_NUM_BITS[FIELDS[field]]
    r = (1 << 256) % p
    vals = [0, 1, 2, 0xFFFFFFFF, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << (nbits - 1)) - 1, r, r * r % p]
    vals += [1 << k for k in (31, 32, 33, 63, 64, 127, 128, 191, 192, 223, 224, nbits - 2)]
    vals += [p - (1 << k) for k in (32, 64, 128, 192, 224)]
    vals += [(0xFFFFFFFF << (32 * i)) % p for i in range(8)]
    vals += [_limbs_int([0xFFFFFFFF, 0] * 4) % p, _limbs_int([0, 0xFFFFFFFF] * 4) % p,
             _limbs_int([0x80000000] * 8) % p, _limbs_int([0xFFFFFFFF] * 7 + [0]) % p]
    assert all(0 <= v < p for v in vals)
    return vals


def uniform(field, n, seed):
    p = modulus(field)
    rng = random.Random(f"{field}/{seed}")
    return [rng.randrange(p) for _ in range(n)]


def to29(x, n=9):
    return [(x >> (W29 * i)) & MASK29 for i in range(n)]


def from29(limbs):
    return _limbs_int(limbs, W29)


def limit_vectors(bound):
    """9-limb vectors whose limbs reach `bound` (inclusive): the radix-2^29 layer's contract limits (field29.cuh: tight < 2^29,
    both operands < 2^30, or tight x loose < 2^31).  Their values are mostly far above p."""
    z = [0] * 9
    vecs = [[bound] * 9, [bound] * 8 + [0], [0] * 8 + [bound], [bound, 0] * 4 + [bound], [0, bound] * 4 + [0],
            [bound] * 8 + [MASK29 >> 6], [1] + [bound] * 8]
    for i in range(9):
        v = list(z)
        v[i] = bound
        vecs.append(v)
    vecs.append([MASK29] * 4 + [bound] * 5)
    vecs.append([bound] * 4 + [MASK29] * 5)
    return vecs


def uniform_limbs(n, bound, seed):
    rng = random.Random(f"limbs/{bound}/{seed}")
    return [[rng.randrange(bound + 1) for _ in range(9)] for _ in range(n)]
