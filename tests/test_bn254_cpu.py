"""CPU: the fourth field pack (Bn254Fq, the BN254 base field) and the radix-2^29 curve layer over both BN254-cycle fields.

* the pack's constants against their Python derivation, and the curves' parameters;
* the new generated asm headers: what the generators emit under --bn254fq (the default output is held by tests/test_asm_emulator.py),
  every block through the one-lane emulator - static checks and exact REDC values on the operand sets the other fields get;
* field29.cuh / curve29.cuh / msm_precompute.cuh built for the host with LURK_F29_CHECK (tests/host_harness_bn254): products,
  squarings, lazy subtraction, the reduction, conversions, mixed and general XYZZ additions, a window-table row, against
  tests/bn254_ref.py.  A violated bound aborts the process, so each group runs in a child;
* the new translation units compile for gfx950 within the register budgets of their launch bounds, and their accumulate, finalize
  and reduction kernels use no scratch memory."""
import ctypes
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import bn254_ref as B
from tests import gfx950_asm_emu as E
from tests import test_asm_emulator as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lurk_beta_amd", "csrc")
NEW_HEADERS = {"gen_field_asm.py": "field_mul_asm_bn254fq.cuh", "gen_field29_asm.py": "field29_mul_asm_bn254fq.cuh"}
P = B.BN254_P
MASK29 = (1 << 29) - 1


# ---- the pack --------------------------------------------------------------------------------------------------------------
def _pack(name):
    src = open(os.path.join(CSRC, "field.cuh")).read()
    body = src[src.index(f"struct {name} {{"):]
    body = body[:body.index("\n};")]
    arrays = {m.group(1): sum(int(w, 16) << (32 * i) for i, w in enumerate(re.findall(r"0x([0-9a-f]{8})u", m.group(2))))
              for m in re.finditer(r"uint32_t (\w+)\(int i\) \{\s*constexpr uint32_t m\[8\] = \{([^}]*)\}", body)}
    scal = {k: int(v, 0) for k, v in re.findall(r"static constexpr \w+ (\w+) = (\w+?)u?;", body)}
    return arrays, scal, body


def test_pack_constants_equal_their_derivation():
    arrays, scal, body = _pack("Bn254Fq")
    assert arrays["mod"] == P == 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
    assert scal == {"ID": 3, "NBITS": P.bit_length(), "INV": (-pow(P, -1, 1 << 32)) % (1 << 32)}
    assert scal["NBITS"] == 254 and scal["INV"] == 0xE4866389 and P % 4 == 3
    assert arrays["r"] == (1 << 256) % P and arrays["r2"] == pow(2, 512, P)
    assert (P - 1) % 4 == 2 and "w32(int i) { return 0; }" in body  # 2-adicity 1: no NTT
    assert P >> 224 < (1 << 31) - 1  # fe_mul_cios' "no extra carry word" condition
    hdr = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    for name, val in (("LURK_FIELD_BN254_FQ", 3), ("LURK_CURVE_BN254", 2), ("LURK_CURVE_GRUMPKIN", 3), ("LURK_HIP_ABI_VERSION", 4)):
        assert re.search(rf"#define {name} {val}\b", hdr), name


def test_curve_parameters():
    for c in B.CURVES.values():
        assert c.on_curve(c.gen) and c.mul(c.order, c.gen) is None and c.mul(c.order - 1, c.gen) == c.neg(c.gen)
        assert c.add(c.gen, c.gen) == c.mul(2, c.gen) and c.add(c.mul(5, c.gen), c.mul(7, c.gen)) == c.mul(12, c.gen)
    assert B.BN254.order == B.GRUMPKIN.p and B.GRUMPKIN.order == B.BN254.p
    # the generator's y as synth.hip spells it (8 x u32, little-endian)
    src = open(os.path.join(CSRC, "synth.hip")).read()
    words = re.search(r"const uint32_t w\[8\] = \{([^}]*)\}", src).group(1)
    assert sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(words.split(","))) == B.GRUMPKIN.gen[1]


# ---- generated headers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", sorted(NEW_HEADERS))
def test_new_header_is_what_the_generator_emits(gen):
    out = subprocess.run([sys.executable, os.path.join(CSRC, gen), "--bn254fq"], check=True, capture_output=True).stdout
    with open(os.path.join(CSRC, NEW_HEADERS[gen]), "rb") as f:
        assert out == f.read(), f"{NEW_HEADERS[gen]} differs from `python {gen} --bn254fq`: regenerate it"
    # the new header holds the new field alone, and the default output does not mention it
    assert set(re.findall(rb"_asm<(\w+)>", out)) == {b"Bn254Fq"}
    assert b"Bn254Fq" not in subprocess.run([sys.executable, os.path.join(CSRC, gen)], check=True, capture_output=True).stdout
    inc = open(os.path.join(CSRC, "field.cuh" if gen == "gen_field_asm.py" else "field29.cuh")).read()
    old = NEW_HEADERS[gen].replace("_bn254fq", "")
    assert f'#include "{old}"\n#include "{NEW_HEADERS[gen]}"\n' in inc


def _blocks():
    out = {}
    for h in NEW_HEADERS.values():
        path = os.path.join(CSRC, h)
        blocks = E.parse_header(path)
        assert len(blocks) == len(re.findall(r"\basm\s*\(", open(path).read()))  # no asm statement escapes the parser
        for b in blocks:
            out[b.name, b.field] = b
    return out


BLOCKS = _blocks()


class _Field:
    """tests/field_cases.py's operand sets for a modulus its table does not hold (the table belongs to oracle/)"""

    def __init__(self):
        from tests import field_cases as FC

        self.FC = FC

    def structured(self):
        FC, p, nbits = self.FC, P, 254
        r = (1 << 256) % p
        vals = [0, 1, 2, 0xFFFFFFFF, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << (nbits - 1)) - 1, r, r * r % p]
        vals += [1 << k for k in (31, 32, 33, 63, 64, 127, 128, 191, 192, 223, 224, nbits - 2)]
        vals += [p - (1 << k) for k in (32, 64, 128, 192, 224)]
        vals += [(0xFFFFFFFF << (32 * i)) % p for i in range(8)]
        vals += [FC._limbs_int([0xFFFFFFFF, 0] * 4) % p, FC._limbs_int([0, 0xFFFFFFFF] * 4) % p, FC._limbs_int([0x80000000] * 8) % p,
                 FC._limbs_int([0xFFFFFFFF] * 7 + [0]) % p]
        assert all(0 <= v < p for v in vals)
        return vals

    def uniform(self, n, seed):
        rng = random.Random(f"Bn254Fq/{seed}")
        return [rng.randrange(P) for _ in range(n)]


F = _Field()


def test_blocks_found_and_static_checks():
    assert set(BLOCKS) == {(n, "Bn254Fq") for n in ("fe_mul_asm", "fe_redc16_asm", "f29_mul_asm", "f29_sqr_asm")}
    for b in BLOCKS.values():
        b.compile()  # hazards, register use
        assert {l.split()[0] for l in b.lines} <= set(E.MNEMONICS)
    assert all(any(l.startswith("v_addc") for l in b.lines) for k, b in BLOCKS.items() if k[0].startswith("fe_"))
    # the counts the issue model prices: no zero or one limbs to skip in this modulus
    assert sum(l.startswith("v_mad") for l in BLOCKS["f29_mul_asm", "Bn254Fq"].lines) == 162
    assert sum(l.startswith("v_mad") for l in BLOCKS["fe_mul_asm", "Bn254Fq"].lines) == 128


def test_fe_mul_and_redc_blocks_exact():
    s, u = F.structured(), F.uniform(2 * T.N_UNIFORM, 1)
    pairs = [(a, b) for a in s for b in s] + list(zip(u[::2], u[1::2]))
    assert T.check_fe_mul(BLOCKS["fe_mul_asm", "Bn254Fq"], P, pairs) == len(s) ** 2 + T.N_UNIFORM
    T.check_fe_mul(BLOCKS["fe_mul_asm", "Bn254Fq"], P, [(a, a) for a in s + F.uniform(T.N_UNIFORM, 9)])
    u = F.uniform(9 * 300, 10)
    vals = [a * b for a in s for b in s] + [k * (P - 1) ** 2 for k in (1, 2, 3, 5, 9)]
    vals += [sum(x * y for x, y in zip(u[9 * i:9 * i + k], u[9 * i + 1:9 * i + k + 1])) for i in range(299) for k in (3, 9)]
    vals += [sum(s[(i + j) % len(s)] * s[(3 * i + j) % len(s)] for j in range(9)) for i in range(len(s))]
    assert max(vals) <= 9 * (P - 1) ** 2
    T.check_fe_redc16(BLOCKS["fe_redc16_asm", "Bn254Fq"], P, vals)


def _f29_pairs():
    FC = F.FC
    s = [FC.to29(v) for v in F.structured()]
    tight, loose31, both30 = FC.limit_vectors(FC.MASK29), FC.limit_vectors((1 << 31) - 1), FC.limit_vectors((1 << 30) - 1)
    pairs = [(a, b) for a in s for b in s]
    pairs += [(a, b) for a in tight + s for b in loose31] + [(b, a) for a in tight + s for b in loose31]
    pairs += [(a, b) for a in both30 for b in both30 + s]
    u = F.uniform(2 * T.N_UNIFORM, 2)
    pairs += [(FC.to29(a), FC.to29(b)) for a, b in zip(u[::2], u[1::2])]
    pairs += list(zip(FC.uniform_limbs(500, FC.MASK29, 3), FC.uniform_limbs(500, (1 << 31) - 1, 4)))
    pairs += list(zip(FC.uniform_limbs(500, (1 << 30) - 1, 5), FC.uniform_limbs(500, (1 << 30) - 1, 6)))
    return pairs


def test_f29_blocks_exact():
    FC = F.FC
    T.check_f29_mul(BLOCKS["f29_mul_asm", "Bn254Fq"], P, _f29_pairs())
    ops = [FC.to29(v) for v in F.structured()] + FC.limit_vectors(FC.MASK29) + [FC.to29(v) for v in F.uniform(T.N_UNIFORM, 7)] + FC.uniform_limbs(500, FC.MASK29, 8)
    T.check_f29_mul(BLOCKS["f29_sqr_asm", "Bn254Fq"], P, [(a, None) for a in ops], square=True)


def test_checker_notices_a_wrong_modulus_literal():
    for key, b in BLOCKS.items():
        lits = [i for i, l in enumerate(b.lines) if re.fullmatch(r"s_mov_b32 s\d+, 0x[0-9a-f]{8}", l)]
        reg, lit = b.lines[lits[0]].split(", ")
        lines = list(b.lines)
        lines[lits[0]] = f"{reg}, 0x{int(lit, 16) ^ 0x10:08x}"
        edited = b.copy_with(lines).compile()
        u = F.uniform(40, 11)
        with pytest.raises(AssertionError):
            if key[0] == "fe_mul_asm":
                T.check_fe_mul(edited, P, list(zip(u[::2], u[1::2])))
            elif key[0] == "fe_redc16_asm":
                T.check_fe_redc16(edited, P, [a * b for a, b in zip(u[::2], u[1::2])])
            else:
                sq = key[0] == "f29_sqr_asm"
                T.check_f29_mul(edited, P, [(F.FC.to29(a), None if sq else F.FC.to29(b)) for a, b in zip(u[::2], u[1::2])], square=sq)


# ---- the radix-2^29 layer on the host, bound assertions on -------------------------------------------------------------------
# A violated bound aborts: the checks run in ONE child process per field, which prints "ok <count>" when every comparison held.
_CHILD = r'''
import ctypes, random, sys
import numpy as np
from tests import bn254_ref as B
from tests import host_harness_bn254 as H
from tests import field_cases as FC

field = int(sys.argv[1])
p = B.FIELD_MODULUS[field]
curve = B.GRUMPKIN if field == B.FIELD_BN254_FR else B.BN254   # the curve whose BASE field this is
assert curve.p == p
L = H.lib()
u32 = lambda xs: np.array(xs, dtype=np.uint32)
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
R261, R256 = 1 << 261, 1 << 256
rng = random.Random(f"bn254-harness/{field}")
count = 0

def f29(op, a, b=None):
    o = np.zeros(9, dtype=np.uint32)
    aa, bb = u32(a), u32(b if b is not None else [0] * 9)
    L.hb_f29_op(field, op, ptr(aa), ptr(bb), ptr(o))
    return [int(x) for x in o]

def w8(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]

def i8(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))

edge = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << 253) - 1, (1 << 256) % p, 0xFFFFFFFF, (1 << 224) - 1]
vals = edge + [rng.randrange(p) for _ in range(300)]
ones = [[FC.MASK29] * 9, [FC.MASK29] * 8 + [0], [0] * 8 + [FC.MASK29], [FC.MASK29] * 8 + [FC.MASK29 >> 6]]
tight = [FC.to29(v) for v in vals] + ones + FC.uniform_limbs(200, FC.MASK29, field)
# products and squarings: exact REDC, limbs 0..7 tight
for a in tight:
    for b in (tight[:14] + ones + [[(1 << 30) - 1] * 9]):
        t = FC.from29(f29(0, a, b))
        x, y = FC.from29(a), FC.from29(b)
        m = (-x * y * pow(p, -1, R261)) % R261
        assert t == (x * y + m * p) >> 261, (a, b)
        count += 1
    t = f29(1, a)
    x = FC.from29(a)
    m = (-x * x * pow(p, -1, R261)) % R261
    assert FC.from29(t) == (x * x + m * p) >> 261 and all(w <= FC.MASK29 for w in t[:8])
    count += 1
# lazy subtraction (+ carry): a - b + 64p, for every subtrahend the bias admits (tight, value < 2^259)
sub_b = [FC.to29(v) for v in vals] + [[FC.MASK29] * 8 + [(1 << 27) - 1]] + [FC.to29(rng.randrange(1 << 259)) for _ in range(200)]
for a, b in zip(tight + tight, sub_b + sub_b[::-1]):
    t = f29(2, a, b)
    assert FC.from29(t) == FC.from29(a) - FC.from29(b) + 64 * p and all(w <= FC.MASK29 for w in t[:8])
    count += 1
# the reduction: any tight value with a top limb below 2^31 comes back congruent, tight and below 2^255.1
red = tight + [[FC.MASK29] * 8 + [(1 << 31) - 1], [0] * 8 + [(1 << 31) - 1], [0] * 8 + [1 << 22], [FC.MASK29] * 8 + [(1 << 22) - 1]]
red += [FC.to29(rng.randrange(1 << 232)) [:8] + [rng.randrange(1 << 31)] for _ in range(500)]
red += [FC.to29(k * p) for k in (1, 2, 3, 63, 64, 65, 127, 128, 200, 511)] + [FC.to29(k * p - 1) for k in (1, 2, 64, 128, 511)]
for a in red:
    t = f29(3, a)
    v, w = FC.from29(a), FC.from29(t)
    assert w % p == v % p and w <= v and all(x <= FC.MASK29 for x in t) and w < 2 * p + (1 << 243), (a, t)
    count += 1
# multiples of p are recognised, their neighbours are not
for k in list(range(0, 140)) + [169]:
    if k * p < R261:
        assert L.hb_f29_is_multiple(field, ptr(u32(FC.to29(k * p)))) == 1, k
        assert L.hb_f29_is_multiple(field, ptr(u32(FC.to29(k * p + 1)))) == 0, k
        count += 2
for v in vals[2:]:
    assert L.hb_f29_is_multiple(field, ptr(u32(FC.to29(v)))) == 0
# conversions: Montgomery(2^256) -> 9 x 29 is a 5-bit shift; back: canonical for every lazy value
for v in vals:
    o9 = np.zeros(9, dtype=np.uint32)
    L.hb_f29_conv(field, 0, ptr(u32(w8(v))), ptr(o9))
    assert FC.from29([int(x) for x in o9]) == v << 5
    count += 1
for a in tight + red[:40]:
    if FC.from29(a) >= R261:
        continue
    o8 = np.zeros(8, dtype=np.uint32)
    L.hb_f29_conv(field, 1, ptr(u32(a)), ptr(o8))
    assert i8(o8) == FC.from29(a) * pow(32, -1, p) % p, a
    count += 1
if field == B.FIELD_BN254_FQ:  # the three 8 x 32 host forms over the new pack
    for a in vals[:60]:
        for b in vals[:12] + vals[-12:]:
            o = np.zeros(24, dtype=np.uint32)
            L.hb_fe_mul(field, ptr(u32(w8(a))), ptr(u32(w8(b))), ptr(o))
            want = a * b * pow(R256, -1, p) % p
            assert i8(o[:8]) == i8(o[8:16]) == i8(o[16:]) == want
            count += 1

# ---- points --------------------------------------------------------------------------------------------------------------
def mont(x):
    return w8(x * R256 % p)

def aff_rec(P):
    return mont(0) + mont(0) if P is None else mont(P[0]) + mont(P[1])

def xyzz_to_point(words):
    o = np.zeros(16, dtype=np.uint32)
    L.hb_to_affine(field, ptr(u32(words)), ptr(o))
    rinv = pow(R256, -1, p)
    xy = (i8(o[:8]) * rinv % p, i8(o[8:]) * rinv % p)
    return None if xy == (0, 0) else xy

def task(points, entries):
    table = u32([w for P in points for w in aff_rec(P)])
    srt = u32(entries)
    o29, o32 = np.zeros(32, dtype=np.uint32), np.zeros(32, dtype=np.uint32)
    L.hb_task(field, ptr(srt), len(entries), ptr(table), ptr(o29), ptr(o32))
    return xyzz_to_point(o29), xyzz_to_point(o32), [int(x) for x in o29]

G = curve.gen
pts = [curve.mul(rng.randrange(1, curve.order), G) for _ in range(24)] + [G, curve.mul(2, G), curve.neg(G), None]
NEG = 0x80000000
cases = [list(range(24)), [0], [0 | NEG], [0, 0], [0, 0 | NEG], [24, 24, 24, 24], [24, 26], [27, 0, 27, 1], [0, 1 | NEG, 2, 3 | NEG] * 8,
         [24, 24, 25 | NEG, 25 | NEG, 24], [27, 27], [5] * 9, [rng.randrange(28) | (NEG if rng.random() < 0.5 else 0) for _ in range(64)]]
sums = []
for ent in cases:
    want = None
    for e in ent:
        Q = pts[e & 0x7FFFFFFF]
        want = curve.add(want, curve.neg(Q) if e & NEG else Q)
    got29, got32, raw = task(pts, ent)
    assert got29 == want and got32 == want, ent
    sums.append(raw)
    count += 1
# general additions (finalize / reduction trees): partial sums incl. equal, opposite and identity operands
groups = [sums[:6], [sums[0], sums[0]], [sums[1], sums[2]], [sums[3], sums[3], sums[3]], sums]
for g in groups:
    flat = u32([w for s in g for w in s])
    o29, o32 = np.zeros(32, dtype=np.uint32), np.zeros(32, dtype=np.uint32)
    L.hb_sum(field, ptr(flat), len(g), ptr(o29), ptr(o32))
    want = None
    for s in g:
        want = curve.add(want, xyzz_to_point(s))
    assert xyzz_to_point(o29) == want == xyzz_to_point(o32)
    count += 1
# a window-table row: 2^(c w) P for the widths the key forms use
for c, Pt in ((16, pts[0]), (20, pts[1]), (8, G), (6, pts[2])):
    W = (256 + c - 1) // c
    tab = np.zeros(W * 16, dtype=np.uint32)
    L.hb_precompute(field, ptr(u32(aff_rec(Pt))), c, W, ptr(tab))
    rinv = pow(R256, -1, p)
    for w in range(W):
        xy = (i8(tab[16 * w:16 * w + 8]) * rinv % p, i8(tab[16 * w + 8:16 * w + 16]) * rinv % p)
        assert xy == curve.mul(1 << (c * w), Pt), (c, w)
        count += 1
# the signed-digit recoding of 254-bit scalars: the top window never carries out, the digits recompose the scalar
order = B.FIELD_MODULUS[field]  # as a SCALAR field (of the cycle's other curve): 254-bit scalars
for c in (6, 8, 16, 17, 18, 19, 20):
    W = (256 + c - 1) // c
    for s in [0, 1, order - 1, (1 << 254) - 1, (1 << 253), order >> 1] + [rng.randrange(order) for _ in range(50)]:
        a, b = np.zeros(W + 1, dtype=np.uint32), np.zeros(W + 1, dtype=np.uint32)
        L.hb_digits(ptr(u32(w8(s))), c, ptr(a), ptr(b))
        assert list(a) == list(b) and a[W] == 0
        val = sum((-(int(d) & 0x7FFFFFFF) if int(d) & NEG else int(d)) << (c * w) for w, d in enumerate(a[:W]))
        assert val == s and all((int(d) & 0x7FFFFFFF) <= 1 << (c - 1) for d in a[:W])
        count += 1
print("ok", count)
'''


@pytest.mark.parametrize("field", [B.FIELD_BN254_FR, B.FIELD_BN254_FQ])
def test_radix29_layer_with_bound_assertions(field):
    r = subprocess.run([sys.executable, "-c", _CHILD, str(field)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert "F29 bound violated" not in r.stdout + r.stderr, (r.stdout + r.stderr)[-600:]
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    m = re.search(r"ok (\d+)", r.stdout)
    assert m and int(m.group(1)) > 5000


# ---- the new translation units on the compiler's own numbers ------------------------------------------------------------------
NEW_UNITS = ("msm_acc_bn254.hip", "msm_acc_persistent_bn254.hip", "msm_finalize_bn254.hip", "msm_reduce_bn254.hip", "msm_bucket_direct_bn254.hip",
             "msm_small_bn254.hip", "msm_precompute_bn254.hip", "msm_sort_bn254.hip")


def _usage(src, tmp):
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-unused-variable",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, src + ".o")], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    out, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, ln)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


_USAGE = {}


def _all_usage(tmp):
    if not _USAGE:
        from concurrent.futures import ThreadPoolExecutor

        units = NEW_UNITS + tuple(u.replace("_bn254", "") for u in NEW_UNITS[:4])
        with ThreadPoolExecutor(6) as ex:
            _USAGE.update(zip(units, ex.map(lambda s: _usage(s, tmp), units)))
    return _USAGE


def _kind(name):
    """kernel name without its field pack: the key that pairs a BN254 kernel with the Pasta kernel of the same template"""
    return re.sub(r"7Bn254F[qr]|8PallasF[pq]", "F", name)


def test_new_units_compile_for_gfx950_and_fit_the_register_budgets(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    res = _all_usage(str(tmp_path))
    for src in NEW_UNITS:
        assert res[src], src
        assert all("Bn254" in k or "msm_canon" in k for k in res[src]), (src, sorted(res[src]))  # no Pasta kernel moved into a new unit
    granule = lambda v: -(-v // 8) * 8
    persistent = max(v["vgpr"] for v in res["msm_acc_persistent_bn254.hip"].values())
    assert persistent <= 256
    # the tail kernels are built scratch-free (two waves per SIMD): a wave of theirs fits beside ONE resident accumulation of its own
    # curve, not beside two as the 128-register Pasta forms do - the finding DESIGN.md section 3.2.1 states
    for src, needle in (("msm_finalize_bn254.hip", "msm_finalize_kernel"), ("msm_reduce_bn254.hip", "msm_planes29")):
        tail = {k: v["vgpr"] for k, v in res[src].items() if needle in k}
        assert tail and all(v <= 256 and granule(v) + granule(persistent) <= 512 for v in tail.values()), (tail, persistent)
    # no accumulate / finalize / reduction kernel needs more scratch than the Pasta kernel of the same template
    checked = 0
    for src in NEW_UNITS[:4]:
        pasta = {}
        for k, v in res[src.replace("_bn254", "")].items():
            pasta[_kind(k)] = max(pasta.get(_kind(k), 0), v["scratch"])
        for k, v in res[src].items():
            assert v["scratch"] <= pasta[_kind(k)], (src, k, v, pasta[_kind(k)])
            checked += 1
    assert checked >= 2 + 2 + 2 + 2 * 8


def test_no_new_accumulate_finalize_or_reduction_kernel_uses_scratch(tmp_path):
    """The new units are built so that nothing spills and no out-of-line branch owns a stack frame: the rare doubling branches of
    curve29.cuh inlined (LURK_F29_RARE_ATTR), the tail kernels at two waves per SIMD.  (The Pasta units keep their forms: 192 bytes per
    lane in the accumulations, 336-560 in the 128-register tail kernels.)"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    res = _all_usage(str(tmp_path))
    bad = {(src, k[:60]): v["scratch"] for src in NEW_UNITS[:4] for k, v in res[src].items() if v["scratch"] != 0}
    assert not bad, bad
