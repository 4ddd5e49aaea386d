"""Shared by the NTT tests (tests/test_gpu_ntt.py on the device, tests/test_host_harness.py on the host harness): the launch plan
lurk_hip_ntt_dev picks per size, the structured and extreme inputs, and the canonical-range check."""
import numpy as np

from oracle import coracle as C
from oracle import pyref as R

# one size from each plan family: LDS path (3, 11), two wave passes (12, 15), three (17, 21), four (25)
FAMILY_SIZES = (3, 11, 12, 15, 17, 21, 25)


def plan(log_n: int):
    """The pass plan of ntt.hip: ntt_device.  None below 2^12 (one LDS-stage pass); else the stages per wave-resident pass."""
    if log_n < 12:
        return None
    passes = (log_n + 7) // 8
    s0, out = 0, []
    for p in range(passes):
        ns = (log_n - s0 + (passes - p) - 1) // (passes - p)
        out.append(ns)
        s0 += ns
    return out


def below_p(limbs: np.ndarray, f: int) -> bool:
    """Every row of 4 x u64 limbs is a canonical value (< p), compared limb-wise from the top."""
    a = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    pl = C.ints_to_limbs([R.modulus(f)])[0]
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[:, k] < pl[k])
        eq &= a[:, k] == pl[k]
    return bool(lt.all())


def extreme_inputs(f: int, log_n: int) -> dict:
    """The operands where a lazily reduced kernel goes wrong, as name -> a function that builds the (n, 4) array (one alive at a
    time at 2^25): all p - 1; alternating 0 and p - 1; p - 1 in the lower half and 0 in the upper; a mix of p - 1 - small,
    2^253 + small and high-limb-heavy values (top word just below p's, low words all ones)."""
    n = 1 << log_n
    p = R.modulus(f)
    pm1 = C.ints_to_limbs([p - 1])[0]

    def alternating():
        a = np.zeros((n, 4), dtype=np.uint64)
        a[1::2] = pm1
        return a

    def half():
        a = np.zeros((n, 4), dtype=np.uint64)
        a[: max(n // 2, 1)] = pm1
        return a

    def mixed():
        top = p >> 192
        pool = [p - 1 - s for s in range(8)] + [(1 << 253) + s for s in range(8)]
        pool += [((top - 1 - s) << 192) | ((1 << 192) - 1 - s) for s in range(8)]
        assert all(0 <= v < p for v in pool)
        return C.ints_to_limbs(pool)[np.random.default_rng(log_n * 2 + f).integers(0, len(pool), n)]

    return {"all_p_minus_1": lambda: np.tile(pm1, (n, 1)), "alternating_0_p_minus_1": alternating, "half_p_minus_1": half, "mixed_extremes": mixed}


def structured_specs(f: int, log_n: int) -> list:
    """Inputs whose transforms are known in closed form (test_gpu_ntt.py: test_known_answers_without_the_oracle), as (name, kind,
    value): constants c = 1, p - 1 and a random c; delta_k for k = 0, 1, n / 2, n - 1 and a random k."""
    n = 1 << log_n
    p = R.modulus(f)
    out = [("const_1", "const", 1), ("const_p_minus_1", "const", p - 1), ("const_random", "const", R.uniform_fe(880 + f, log_n, p))]
    for k in sorted({0, 1, n // 2 % n, n - 1, int(np.random.default_rng(log_n).integers(0, n))}):
        out.append((f"delta_{k}", "delta", k))
    return out


def structured_array(n: int, kind: str, v: int) -> np.ndarray:
    if kind == "const":
        return np.tile(C.ints_to_limbs([v])[0], (n, 1))
    a = np.zeros((n, 4), dtype=np.uint64)
    a[v, 0] = 1
    return a
