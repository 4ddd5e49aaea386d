"""CPU: the generated gfx950 multiplier asm blocks, executed instruction by instruction for one lane (tests/gfx950_asm_emu.py),
against Python integers, with the hazard and register rules asserted; plus the headers' freshness against their generators.

The host build of field.cuh / field29.cuh never runs this asm, and the GPU tests reach it only through whole kernels with random
operands.  Here every block of both headers sees the structured operands of tests/field_cases.py, the radix-2^29 contract limits
and seeded uniform pairs.  The self-tests edit copies of the blocks and require the checker to notice."""
import os
import re
import subprocess
import sys

import pytest

from tests import field_cases as FC
from tests import gfx950_asm_emu as E

FIELDS = list(FC.FIELDS)
BLOCKS = E.all_blocks()
N_UNIFORM = 2000


def limbs32(x, n=8):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def int32(words):
    return sum(w << (32 * i) for i, w in enumerate(words))


def redc(v, p, rbits):
    """exact Montgomery reduction (v + m p) / 2^rbits with m = -v p^-1 mod 2^rbits: what a column-wise REDC computes"""
    m = (-v * pow(p, -1, 1 << rbits)) % (1 << rbits)
    return (v + m * p) >> rbits


def test_every_block_is_found_and_passes_the_static_checks():
    want = {(n, f) for f in FIELDS for n in ("fe_mul_asm", "fe_redc16_asm", "f29_mul_asm", "f29_sqr_asm")}
    assert set(BLOCKS) == want
    # no asm statement of either header escapes the parser
    assert sum(len(re.findall(r"\basm\s*\(", open(h).read())) for h in E.HEADERS) == len(BLOCKS)
    for b in BLOCKS.values():
        b.compile()
        used = {l.split()[0] for l in b.lines}
        assert used <= set(E.MNEMONICS)
    # every fe block keeps carries in flight and pads them: the hazard check has something to check
    assert all(any(l.startswith("v_addc") for l in b.lines) for k, b in BLOCKS.items() if k[0].startswith("fe_"))


# ---- value checks (also used by the self-tests on edited blocks) ------------------------------------------------------------
def check_fe_mul(block, p, pairs):
    """fe_mul_asm: raw output = a*b/2^256 (exact REDC) < 2p; after fe_cond_sub, a*b/2^256 mod p"""
    for a, b in pairs:
        raw = int32(block.run(*limbs32(a), *limbs32(b)))
        want = redc(a * b, p, 256)
        assert raw == want, (block.name, block.field, hex(a), hex(b))
        assert raw < 2 * p, (block.name, hex(a), hex(b))            # the bound fe_cond_sub relies on
        out = raw - p if raw >= p else raw
        assert out == a * b * pow(2, -256, p) % p
    return len(pairs)


def check_fe_redc16(block, p, values):
    for v in values:
        t = int32(block.run(*limbs32(v, 16)))
        want = redc(v, p, 256)
        assert want < (1 << 256), hex(v)                            # the block's stated bound (its result is 8 words)
        assert t == want, (block.field, hex(v))
        assert t % p == v * pow(2, -256, p) % p
    return len(values)


def check_f29_mul(block, p, pairs, square=False):
    """f29_mul_asm / f29_sqr_asm: exact REDC with R = 2^261, limbs 0..7 tight; the top limb is tight whenever the value bound
    a*b < 2^261 (2^261 - p) holds; a tight operand < 2^260 times a canonical one gives < 2^255 + p (ntt29.cuh)."""
    for la, lb in pairs:
        if square:
            assert lb is None and all(x <= FC.MASK29 for x in la)
            out = block.run(*la, *[(x << 1) & 0xFFFFFFFF for x in la])
            lb = la
        else:
            out = block.run(*la, *lb)
        a, b = FC.from29(la), FC.from29(lb)
        t = FC.from29(out)
        assert t == redc(a * b, p, 261), (block.name, block.field, la, lb)
        assert all(x <= FC.MASK29 for x in out[:8]), (block.name, la, lb, out)
        if a * b < (1 << 261) * ((1 << 261) - p):
            assert out[8] <= FC.MASK29, (block.name, la, lb, out)
        tight_a, tight_b = all(x <= FC.MASK29 for x in la), all(x <= FC.MASK29 for x in lb)
        if (b < p and tight_a and a < (1 << 260)) or (a < p and tight_b and b < (1 << 260)):
            assert t < (1 << 255) + p, (block.name, la, lb)
    return len(pairs)


def _fe_pairs(field):
    s = FC.structured(field)
    u = FC.uniform(field, 2 * N_UNIFORM, 1)
    return [(a, b) for a in s for b in s] + list(zip(u[::2], u[1::2]))


def _f29_pairs(field):
    s = [FC.to29(v) for v in FC.structured(field)]
    tight = FC.limit_vectors(FC.MASK29)
    loose31 = FC.limit_vectors((1 << 31) - 1)
    both30 = FC.limit_vectors((1 << 30) - 1)
    pairs = [(a, b) for a in s for b in s]
    pairs += [(a, b) for a in tight + s for b in loose31] + [(b, a) for a in tight + s for b in loose31]
    pairs += [(a, b) for a in both30 for b in both30 + s]
    u = FC.uniform(field, 2 * N_UNIFORM, 2)
    pairs += [(FC.to29(a), FC.to29(b)) for a, b in zip(u[::2], u[1::2])]
    pairs += list(zip(FC.uniform_limbs(500, FC.MASK29, 3), FC.uniform_limbs(500, (1 << 31) - 1, 4)))
    pairs += list(zip(FC.uniform_limbs(500, (1 << 30) - 1, 5), FC.uniform_limbs(500, (1 << 30) - 1, 6)))
    assert all(max(a) < (1 << 31) and max(b) < (1 << 31) for a, b in pairs)
    return pairs


def _f29_square_operands(field):
    s = [FC.to29(v) for v in FC.structured(field)]
    u = [FC.to29(v) for v in FC.uniform(field, N_UNIFORM, 7)]
    return s + FC.limit_vectors(FC.MASK29) + u + FC.uniform_limbs(500, FC.MASK29, 8)


@pytest.mark.parametrize("field", FIELDS)
def test_fe_mul_block(field):
    assert check_fe_mul(BLOCKS["fe_mul_asm", field], FC.modulus(field), _fe_pairs(field)) == len(FC.structured(field)) ** 2 + N_UNIFORM


@pytest.mark.parametrize("field", FIELDS)
def test_fe_mul_block_as_square(field):
    vals = FC.structured(field) + FC.uniform(field, N_UNIFORM, 9)
    check_fe_mul(BLOCKS["fe_mul_asm", field], FC.modulus(field), [(a, a) for a in vals])


@pytest.mark.parametrize("field", FIELDS)
def test_fe_redc16_block(field):
    """inputs as dot_finish feeds them: sums of T <= 9 products of canonical values (< 9 p^2), incl. the worst case"""
    p = FC.modulus(field)
    s = FC.structured(field)
    u = FC.uniform(field, 9 * 300, 10)
    vals = [a * b for a in s for b in s]
    vals += [T * (p - 1) ** 2 for T in (1, 2, 3, 5, 9)]
    vals += [sum(x * y for x, y in zip(u[9 * i:9 * i + T], u[9 * i + 1:9 * i + T + 1])) for i in range(299) for T in (3, 9)]
    vals += [sum(s[(i + j) % len(s)] * s[(3 * i + j) % len(s)] for j in range(9)) for i in range(len(s))]
    assert max(vals) <= 9 * (p - 1) ** 2
    check_fe_redc16(BLOCKS["fe_redc16_asm", field], p, vals)


@pytest.mark.parametrize("field", FIELDS)
def test_f29_mul_block(field):
    check_f29_mul(BLOCKS["f29_mul_asm", field], FC.modulus(field), _f29_pairs(field))


@pytest.mark.parametrize("field", FIELDS)
def test_f29_sqr_block(field):
    check_f29_mul(BLOCKS["f29_sqr_asm", field], FC.modulus(field), [(a, None) for a in _f29_square_operands(field)], square=True)


# ---- self-tests: the checker must notice an edited block ----------------------------------------------------------------
def _value_check(block):
    field = block.field
    p = FC.modulus(field)
    if block.name == "fe_mul_asm":
        check_fe_mul(block, p, _fe_pairs(field)[-200:])
    elif block.name == "fe_redc16_asm":
        u = FC.uniform(field, 400, 11)
        check_fe_redc16(block, p, [a * b for a, b in zip(u[::2], u[1::2])])
    elif block.name == "f29_mul_asm":
        check_f29_mul(block, p, _f29_pairs(field)[-200:])
    else:
        check_f29_mul(block, p, [(a, None) for a in _f29_square_operands(field)[-200:]], square=True)


@pytest.mark.parametrize("key", [k for k in BLOCKS if any(l.startswith("s_nop") for l in BLOCKS[k].lines)])
def test_self_check_deleted_nop_is_a_hazard(key):
    b = BLOCKS[key]
    nops = [i for i, l in enumerate(b.lines) if l.startswith("s_nop")]
    assert nops
    for i in nops:
        with pytest.raises(E.HazardError):
            b.copy_with(b.lines[:i] + b.lines[i + 1:]).compile()


def _tight_folds(lines):
    """indices of v_addc folds whose carry pair was written exactly two wait states earlier"""
    out = []
    for i, l in enumerate(lines):
        if not l.startswith("v_addc"):
            continue
        pair = l.split(",")[-1].strip()
        clock, j = 0, i - 1
        while j >= 0:
            m = lines[j]
            if m.startswith("v_mad") and m.split(",")[1].strip() == pair:
                break
            clock += int(m.split()[1]) + 1 if m.startswith("s_nop") else 1
            j -= 1
        if j >= 0 and clock == E.HAZARD_WAIT_STATES and not lines[i - 1].startswith("s_nop") and i - 1 != j:
            out.append(i)
    return out


@pytest.mark.parametrize("key", [k for k in BLOCKS if k[0].startswith("fe_")])
def test_self_check_fold_one_instruction_earlier_is_a_hazard(key):
    b = BLOCKS[key]
    folds = _tight_folds(b.lines)
    assert len(folds) >= 8, "the schedule has folds at the minimum distance"
    for i in folds:
        lines = list(b.lines)
        lines[i - 1], lines[i] = lines[i], lines[i - 1]
        with pytest.raises(E.HazardError):
            b.copy_with(lines).compile()


@pytest.mark.parametrize("key", sorted(BLOCKS))
def test_self_check_wrong_modulus_literal_fails_the_values(key):
    b = BLOCKS[key]
    _value_check(b)  # the unedited block passes the same check
    lits = [i for i, l in enumerate(b.lines) if re.fullmatch(r"s_mov_b32 s\d+, 0x[0-9a-f]{8}", l)]
    assert lits
    for i in (lits[0], lits[-1]):
        reg, lit = b.lines[i].split(", ")
        lines = list(b.lines)
        lines[i] = f"{reg}, 0x{int(lit, 16) ^ 0x10:08x}"
        edited = b.copy_with(lines).compile()  # still well-formed: hazards and registers are unchanged
        with pytest.raises(AssertionError):
            _value_check(edited)


def test_self_check_undeclared_register_and_vcc_read():
    b = BLOCKS["fe_mul_asm", "PallasFp"]
    i = next(i for i, l in enumerate(b.lines) if l.startswith("v_sub_u32"))
    lines = list(b.lines)
    lines.insert(i + 1, "v_mov_b32 v40, v16")
    with pytest.raises(E.RegisterError):
        b.copy_with(lines).compile()
    lines = list(b.lines)
    lines.insert(len(lines), "v_mov_b32 %0, vcc")
    with pytest.raises(E.HazardError):
        b.copy_with(lines).compile()
    with pytest.raises(E.AsmError):
        b.copy_with(b.lines + ["v_add_u32 v16, v16, v17"]).compile()


# ---- the committed headers are what the generators produce ----------------------------------------------------------------
@pytest.mark.parametrize("gen,header", [("gen_field_asm.py", "field_mul_asm.cuh"), ("gen_field29_asm.py", "field29_mul_asm.cuh")])
def test_generated_header_is_current(gen, header):
    out = subprocess.run([sys.executable, os.path.join(E.CSRC, gen)], check=True, capture_output=True).stdout
    with open(os.path.join(E.CSRC, header), "rb") as f:
        assert out == f.read(), f"{header} differs from `python {gen}`: regenerate it"
