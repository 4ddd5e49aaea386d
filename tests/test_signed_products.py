"""CPU: the signed product blocks of field29_mul_asm_p1s.cuh (gen_field29_asm.py --p1-signed) and their portable forms.

The header must be what the generator writes, byte for byte.  Each block is then run one lane at a time, instruction by instruction,
by a small interpreter of its seven mnemonics (the static register and hazard rules are those of tests/test_asm_emulator_p1.py, applied
to the same text with the signed mad read as the unsigned one: the operands are the same).  Block and portable form (compiled into
tests/host_signed_madd, which prints its limbs) must give the SAME nine limbs, and those the exact signed Montgomery quotient in Python
integers: t = (a b + m p) / 2^261 with m = -a b / p mod 2^261, limbs 0..7 tight, the top limb signed.

Operands: every class of the contract (field29.cuh, "signed operands") at its extremes - all-ones tight limbs, most-negative and
most-positive differences, the widest top limbs the value contract |a b| < 2^522 allows - zeros in the low limbs (a reduction column
that is exactly 0, the case the H = A - 1 form exists for), sparse limbs and random ones."""
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

from tests import field_cases as FC
from tests import gfx950_asm_emu as E
from tests.test_asm_emulator_p1 import P1Block

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(E.CSRC, "field29_mul_asm_p1s.cuh")
FIELDS = ["PallasFp", "PallasFq"]
MASK = FC.MASK29
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
BLOCKS = {(b.name, b.field): b for b in E.parse_header(HEADER)}


def s32(x):
    return x - (1 << 32) if x >> 31 else x


def s64(x):
    return x - (1 << 64) if x >> 63 else x


def run_block(b, inputs):
    """one lane: inputs are signed limbs in operand order; returns the nine output limbs as signed 32-bit values"""
    reg = {f"o{b.n_out + i}": v & M32 for i, v in enumerate(inputs)}

    def r32(t):
        regs = E_regs(t)
        return (int(t, 0) & M32) if regs is None else reg[regs[0]]

    def r64(t):
        regs = E_regs(t)
        return (int(t, 0) & M64) if regs is None else reg[regs[0]] | (reg[regs[1]] << 32)

    def w64(t, v):
        lo, hi = E_regs(t)
        reg[lo], reg[hi] = v & M32, (v >> 32) & M32

    for line in b.lines:
        mn, _, rest = line.partition(" ")
        ops = [o.strip() for o in rest.split(",")]
        if mn in ("v_mad_u64_u32", "v_mad_i64_i32"):
            d, sd, s0, s1, s2 = ops
            x, y = (s32(r32(s0)), s32(r32(s1))) if mn == "v_mad_i64_i32" else (r32(s0), r32(s1))
            acc = s64(r64(s2))
            assert abs(acc + x * y) < 1 << 63, "column at or above 2^63"
            w64(d, (acc + x * y) & M64)
        elif mn in ("v_mov_b32", "s_mov_b32"):
            reg[E_regs(ops[0])[0]] = r32(ops[1])
        elif mn == "v_not_b32":
            reg[E_regs(ops[0])[0]] = ~r32(ops[1]) & M32
        elif mn == "v_and_b32":
            reg[E_regs(ops[0])[0]] = r32(ops[1]) & r32(ops[2])
        elif mn == "v_ashrrev_i64":
            w64(ops[0], (s64(r64(ops[2])) >> (r32(ops[1]) & 63)) & M64)
        elif mn == "v_lshl_add_u64":
            w64(ops[0], ((r64(ops[1]) << (r32(ops[2]) & 7)) + r64(ops[3])) & M64)
        else:
            raise E.AsmError(f"mnemonic {mn!r} is not modelled")
    return [s32(reg[f"o{i}"]) for i in range(b.n_out)]


def E_regs(text):
    return None if re.fullmatch(r"-\d+", text.strip()) else E._regs(text)


def value(limbs):
    return sum(l << (29 * i) for i, l in enumerate(limbs))


def quotient(v, p):
    m = (-v * pow(p, -1, 1 << 261)) % (1 << 261)
    assert (v + m * p) % (1 << 261) == 0
    return (v + m * p) >> 261


def operands(field):
    rng = random.Random(f"p1s/{field}")
    M = MASK
    rl = lambda lo, hi, top: [rng.randint(lo, hi) for _ in range(8)] + [rng.randint(-top, top)]
    T30, T29, T28 = (1 << 30) - 1, (1 << 29) - 1, (1 << 28) - 1
    wide = [[M] * 8 + [T30], [M] * 8 + [-T30], [-M] * 8 + [-T30], [-M] * 8 + [T30]]
    mid = [[M] * 8 + [T29], [-M] * 8 + [-T29], [-M] * 8 + [T29], [M] * 8 + [-T29]]
    narrow = [[M] * 8 + [T28], [-M] * 8 + [-T28], [M] * 8 + [-T28], [M] * 8 + [0], [-M] * 8 + [0], [0] * 9, [1] * 8 + [-1], [-1] * 9]
    pairs = [(a, b) for a in wide for b in narrow] + [(b, a) for a in wide for b in narrow] + [(a, b) for a in mid + narrow for b in mid + narrow]
    for k in range(1, 9):  # low k limbs zero: a reduction column that is exactly 0
        a, b = rl(-M, M, T28), rl(-M, M, T28)
        pairs += [([0] * k + a[k:], b), (a, [0] * k + b[k:]), ([0] * k + a[k:], [0] * k + b[k:])]
    pairs += [(rng.choices([0, 1, -1, M, -M], k=9), rng.choices([0, 1, -1, M, -M], k=9)) for _ in range(200)]
    pairs += [(rl(0, M, T28), rl(-M, M, T28)) for _ in range(300)]      # s-tight x s-diff
    pairs += [(rl(-M, M, T29), rl(-M, M, T29)) for _ in range(300)]    # s-diff x s-diff
    pairs += [(a, a) for a in [rl(-M, M, T29) for _ in range(200)] + mid + narrow]   # squares
    return pairs


def test_generated_header_is_current_and_other_modes_are_unchanged():
    out = subprocess.run([sys.executable, os.path.join(E.CSRC, "gen_field29_asm.py"), "--p1-signed"], check=True, capture_output=True).stdout
    with open(HEADER, "rb") as f:
        assert out == f.read(), "field29_mul_asm_p1s.cuh differs from `python gen_field29_asm.py --p1-signed`: regenerate it"


def test_blocks_keep_the_mad_counts_and_the_static_rules():
    assert set(BLOCKS) == {(n, f) for f in FIELDS for n in ("f29_mul_s_asm", "f29_sqr_s_asm")}
    for (name, field), b in BLOCKS.items():
        signed = [l for l in b.lines if l.startswith("v_mad_i64_i32")]
        unsigned = [l for l in b.lines if l.startswith("v_mad_u64_u32")]
        assert (len(signed), len(unsigned)) == ((81, 45) if "mul" in name else (45, 45)), (name, field)   # 126 per product, 90 per squaring
        assert all(re.search(r", v\d+, (s\d+|1), v\[16:17\]$", l) for l in unsigned)                    # unsigned: m_k x modulus limb only
        assert not any(l.startswith("v_lshrrev_b64") for l in b.lines)                                   # every shift of the accumulator is arithmetic
        P1Block(b.name, b.field, [l.replace("v_mad_i64_i32", "v_mad_u64_u32") for l in b.lines], b.n_out, b.n_in, b.clobbers).compile()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("signed_products") / "signed_madd_host")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-DLURK_F29_CHECK=1", os.path.join(ROOT, "tests", "host_signed_madd", "main.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


@pytest.mark.parametrize("fi,field", list(enumerate(FIELDS)))
def test_blocks_and_portable_form_give_the_exact_signed_quotient(host, tmp_path, fi, field):
    p = FC.modulus(field)
    pairs = operands(field)
    path = tmp_path / "operands.txt"
    path.write_text("".join(" ".join(str(x) for x in a + b) + "\n" for a, b in pairs))
    r = subprocess.run([host, "mul", str(fi), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])      # (a bound assertion of the portable form would abort)
    portable = [[int(x) for x in l.split()] for l in r.stdout.splitlines()]
    assert len(portable) == len(pairs)
    mul, sqr = BLOCKS["f29_mul_s_asm", field], BLOCKS["f29_sqr_s_asm", field]
    for (a, b), got in zip(pairs, portable):
        assert abs(value(a) * value(b)) < 1 << 522
        want = quotient(value(a) * value(b), p)
        assert value(got) == want and all(0 <= x <= MASK for x in got[:8]) and abs(want) < (1 << 261) + p, (field, a, b)
        assert run_block(mul, a + b) == got, (field, a, b)
        if a == b:
            assert run_block(sqr, a + [(x << 1) for x in a]) == got, (field, a)
