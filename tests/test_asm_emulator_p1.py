"""CPU: the Pasta blocks of field29_mul_asm_p1.cuh (gen_field29_asm.py --p1), one lane, instruction by instruction.

These blocks carry the accumulator one below its true value through the nine reduction columns and issue no mad by modulus limb 0
(p == 1 mod 2^29).  They must give the SAME nine limbs as the plain blocks of field29_mul_asm.cuh, not merely congruent ones, and
the exact Montgomery quotient a b 2^-261 + (< p).  The emulator of tests/gfx950_asm_emu.py knows the plain blocks' nine mnemonics;
P1Block below adds the three new ones (v_not_b32, v_ashrrev_i64, v_lshl_add_u64) and signed inline constants, with the helper's
register and hazard rules.

Contract of the new blocks (field29.cuh, f29_mul30 / f29_sqr30): 9 la lb + 5 2^58 + carry < 2^63, i.e. tight x (limbs < 2^30), and
a tight operand for the squaring.  All operands here stay inside it; the emulator asserts the signed accumulator bound as it runs."""
import os
import random
import re
import subprocess
import sys

import pytest

from tests import field_cases as FC
from tests import gfx950_asm_emu as E

HEADER = os.path.join(E.CSRC, "field29_mul_asm_p1.cuh")
FIELDS = ["PallasFp", "PallasFq"]
MASK = FC.MASK29
M30 = (1 << 30) - 1
M32 = E.M32
EXTRA_MNEMONICS = ("v_not_b32", "v_ashrrev_i64", "v_lshl_add_u64")


def _regs(text):
    """E._regs plus signed inline constants (-16..-1)"""
    if re.fullmatch(r"-\d+", text.strip()):
        if not -16 <= int(text) <= -1:
            raise E.AsmError(f"not an inline constant: {text}")
        return None
    return E._regs(text)


class P1Block(E.Block):
    """E.Block whose compile() also understands EXTRA_MNEMONICS.  The checks are the helper's: every register read was written
    earlier or is an input operand, every write goes to an output operand or a declared clobber, a VALU that reads an SGPR a VALU
    wrote needs two wait states in between, vcc is never read.  A 64-bit source that is an inline constant is sign-extended."""

    @classmethod
    def of(cls, b):
        return cls(b.name, b.field, b.lines, b.n_out, b.n_in, b.clobbers)

    def copy_with(self, lines):
        return P1Block(self.name, self.field, lines, self.n_out, self.n_in, self.clobbers)

    def compile(self):
        written, clob = set(), set()
        for c in self.clobbers:
            clob.update(["vcc_lo", "vcc_hi"] if c == "vcc" else [c])
        sgpr_valu_write, clock, py = {}, 0, []

        def read(text, idx, valu):
            for r in _regs(text) or ():
                if r.startswith("vcc"):
                    raise E.HazardError(f"line {idx}: reads vcc ({self.lines[idx]})")
                if valu and r in sgpr_valu_write and clock - sgpr_valu_write[r] - 1 < E.HAZARD_WAIT_STATES:
                    raise E.HazardError(f"line {idx}: {r} read too soon after a VALU wrote it ({self.lines[idx]})")
                if r.startswith("o") and int(r[1:]) >= self.n_out:
                    continue
                if r not in written:
                    raise E.RegisterError(f"line {idx}: {r} read before it is written ({self.lines[idx]})")

        def write(text, idx, valu, width):
            regs = _regs(text)
            if regs is None or len(regs) != width:
                raise E.AsmError(f"line {idx}: {width * 32}-bit destination expected ({self.lines[idx]})")
            for r in regs:
                if r.startswith("o"):
                    if int(r[1:]) >= self.n_out:
                        raise E.RegisterError(f"line {idx}: writes input operand {r} ({self.lines[idx]})")
                elif r not in clob:
                    raise E.RegisterError(f"line {idx}: writes {r}, which is not a declared clobber ({self.lines[idx]})")
                written.add(r)
                if r[0] == "s" or r.startswith("vcc"):
                    if valu:
                        sgpr_valu_write[r] = clock
                    else:
                        sgpr_valu_write.pop(r, None)
            return regs

        def val32(text):
            regs = _regs(text)
            if regs is None:
                return str(int(text, 0) & M32)
            if len(regs) != 1:
                raise E.AsmError(f"32-bit operand expected: {text}")
            return regs[0]

        def val64(text):
            regs = _regs(text)
            if regs is None:
                return str(int(text, 0) & 0xFFFFFFFFFFFFFFFF)      # inline constants are sign-extended to 64 bits
            if len(regs) != 2:
                raise E.AsmError(f"64-bit operand expected: {text}")
            return f"({regs[0]} | ({regs[1]} << 32))"

        def put64(dr):
            return f"{dr[0]} = t & {M32}; {dr[1]} = (t >> 32) & {M32}"

        for idx, line in enumerate(self.lines):
            mn, _, rest = line.partition(" ")
            ops = [o.strip() for o in rest.split(",")] if rest.strip() else []
            valu = mn.startswith("v_")
            if mn == "s_nop":
                clock += int(ops[0], 0) + 1
                continue
            if mn == "v_mad_u64_u32":            # D64, SDST64 = S0 * S1 + S2(64); the carry-out of the 64-bit sum goes to SDST
                d, sd, s0, s1, s2 = ops
                for o in (s0, s1, s2):
                    read(o, idx, valu)
                py.append(f"t = {val32(s0)} * {val32(s1)} + {val64(s2)}")
                dr, sr = write(d, idx, valu, 2), write(sd, idx, valu, 2)
                py.append(put64(dr) + f"; {sr[0]} = (t >> 64) & 1; {sr[1]} = 0")
            elif mn in ("v_mov_b32", "s_mov_b32", "v_not_b32"):
                d, s0 = ops
                read(s0, idx, valu)
                py.append(f"{val32(d)} = ({'~' if mn == 'v_not_b32' else ''}{val32(s0)}) & {M32}")
                write(d, idx, valu, 1)
            elif mn == "v_and_b32":
                d, s0, s1 = ops
                read(s0, idx, valu)
                read(s1, idx, valu)
                py.append(f"{val32(d)} = {val32(s0)} & {val32(s1)}")
                write(d, idx, valu, 1)
            elif mn in ("v_lshrrev_b64", "v_ashrrev_i64"):   # D64 = S1(64) >> S0, logical / arithmetic
                d, s0, s1 = ops
                read(s0, idx, valu)
                read(s1, idx, valu)
                if mn == "v_ashrrev_i64":
                    # the block's bound: the accumulator is a signed value >= -1 here (A - 1 with 0 <= A <= 2^63)
                    py.append(f"t = {val64(s1)}")
                    py.append("assert t < (1 << 63) or t == (1 << 64) - 1, 'reduction column at or above 2^63'")
                    py.append(f"t = ((t - ((t >> 63) << 64)) >> ({val32(s0)} & 63)) & {0xFFFFFFFFFFFFFFFF}")
                else:
                    py.append(f"t = {val64(s1)} >> ({val32(s0)} & 63)")
                py.append(put64(write(d, idx, valu, 2)))
            elif mn == "v_lshl_add_u64":         # D64 = (S0(64) << S1) + S2(64)
                d, s0, s1, s2 = ops
                for o in (s0, s1, s2):
                    read(o, idx, valu)
                py.append(f"t = (({val64(s0)} << ({val32(s1)} & 7)) + {val64(s2)}) & {0xFFFFFFFFFFFFFFFF}")
                py.append(put64(write(d, idx, valu, 2)))
            else:
                raise E.AsmError(f"line {idx}: mnemonic {mn!r} is not modelled")
            clock += 1
        missing = [f"o{i}" for i in range(self.n_out) if f"o{i}" not in written]
        if missing:
            raise E.RegisterError(f"output operands never written: {missing}")
        args = ", ".join(f"o{i}" for i in range(self.n_out, self.n_out + self.n_in))
        src = f"def _block({args}):\n" + "".join(f"    {l}\n" for l in py)
        src += "    return (" + "".join(f"o{i}, " for i in range(self.n_out)) + ")\n"
        ns = {}
        exec(compile(src, f"<{self.name}<{self.field}>>", "exec"), ns)
        self._fn = ns["_block"]
        return self


BLOCKS = {(b.name, b.field): P1Block.of(b) for b in E.parse_header(HEADER)}
OLD = E.all_blocks()


def redc(v, p):
    m = (-v * pow(p, -1, 1 << 261)) % (1 << 261)
    return (v + m * p) >> 261


# ---- operands: the smallest that can break the scheme ---------------------------------------------------------------------
def _rand_limbs(rng, bound):
    return [rng.randrange(bound + 1) for _ in range(9)]


def mul_pairs(field):
    p = FC.modulus(field)
    rng = random.Random(f"p1/{field}")
    zero, ones, max30 = [0] * 9, [MASK] * 9, [M30] * 9
    pairs = [(zero, zero), (zero, _rand_limbs(rng, M30)), (_rand_limbs(rng, MASK), zero)]          # every column holds -1
    for _ in range(20):                                                                               # a_0 b_0 = 0, the rest random
        a, b = _rand_limbs(rng, MASK), _rand_limbs(rng, M30)
        pairs += [([0] + a[1:], b), (a, [0] + b[1:]), ([0] + a[1:], [0] + b[1:])]
    for k in range(1, 9):                                                                             # low k limbs zero: true column = 0
        a, b = _rand_limbs(rng, MASK), _rand_limbs(rng, M30)                                          # in the middle of the reduction
        pairs += [([0] * k + a[k:], b), (a, [0] * k + b[k:]), ([0] * k + a[k:], [0] * k + b[k:]),
                  ([0] * k + ones[k:], max30), (ones, [0] * k + max30[k:])]
    pairs += [(ones, max30), (ones, ones), (ones, [M30, 0] * 4 + [M30])]
    edge = [FC.to29(v) for v in (p - 1, p, p + 1, (1 << 261) % p, 1, 2, (1 << 29) - 1, 1 << 29)]
    pairs += [(a, b) for a in edge for b in edge + [max30, zero]]
    pairs += [(a, b) for a in FC.limit_vectors(MASK) for b in FC.limit_vectors(M30)]
    pairs += [(rng.choices([0, 1, MASK], k=9), rng.choices([0, 1, M30], k=9)) for _ in range(300)]   # sparse limbs
    pairs += [(_rand_limbs(rng, MASK), _rand_limbs(rng, MASK)) for _ in range(2000)]                  # tight x tight
    pairs += [(_rand_limbs(rng, MASK), _rand_limbs(rng, M30)) for _ in range(2000)]                   # tight x (2^30 - 1)-bounded
    assert all(max(a) <= MASK and max(b) <= M30 for a, b in pairs)
    return pairs


def sqr_operands(field):
    p = FC.modulus(field)
    rng = random.Random(f"p1sq/{field}")
    ops = [[0] * 9, [MASK] * 9]
    ops += [[0] * k + _rand_limbs(rng, MASK)[k:] for k in range(1, 9)] + [[0] * k + [MASK] * (9 - k) for k in range(1, 9)]
    ops += [FC.to29(v) for v in (p - 1, p, p + 1, (1 << 261) % p, 1, 2, 1 << 29)]
    ops += FC.limit_vectors(MASK) + [rng.choices([0, 1, MASK], k=9) for _ in range(300)]
    ops += [_rand_limbs(rng, MASK) for _ in range(2000)]
    return ops


def check_mul(new, old, p, pairs):
    for a, b in pairs:
        out = new.run(*a, *b)
        assert FC.from29(out) == redc(FC.from29(a) * FC.from29(b), p), (new.field, a, b)
        assert all(x <= MASK for x in out[:8]), (new.field, a, b, out)
        assert out == old.run(*a, *b), (new.field, a, b)             # the same nine limbs, not merely congruent
    return len(pairs)


def check_sqr(new, old, p, ops):
    for a in ops:
        d = [x << 1 for x in a]
        out = new.run(*a, *d)
        assert FC.from29(out) == redc(FC.from29(a) ** 2, p), (new.field, a)
        assert all(x <= MASK for x in out[:8]), (new.field, a, out)
        assert out == old.run(*a, *d), (new.field, a)
    return len(ops)


# ---- the tests ----------------------------------------------------------------------------------------------------------------
def test_every_block_is_found_and_passes_the_static_checks():
    assert set(BLOCKS) == {(n, f) for f in FIELDS for n in ("f29_mul_p1_asm", "f29_sqr_p1_asm")}
    assert len(re.findall(r"\basm\s*\(", open(HEADER).read())) == len(BLOCKS)
    for (name, field), b in BLOCKS.items():
        b.compile()
        used = {l.split()[0] for l in b.lines}
        assert used <= set(E.MNEMONICS) | set(EXTRA_MNEMONICS)
        mads = [l for l in b.lines if l.startswith("v_mad_u64_u32")]
        old_mads = [l for l in OLD[name.replace("_p1", ""), field].lines if l.startswith("v_mad_u64_u32")]
        assert len(mads) == len(old_mads) - 9 == (126 if "mul" in name else 90)
        assert mads[0].endswith(", -1") and not any(l.endswith(", 1, v[16:17]") for l in mads)   # entered by -1; no mad by limb 0
        assert sum(l.startswith("v_ashrrev_i64") for l in b.lines) == 9 and sum(l.startswith("v_lshl_add_u64") for l in b.lines) == 1
        assert len(b.lines) == len(OLD[name.replace("_p1", ""), field].lines) - 8                # -9 mads, +1 increment


@pytest.mark.parametrize("field", FIELDS)
def test_mul_block_equals_the_plain_block_and_the_exact_quotient(field):
    pairs = mul_pairs(field)
    assert check_mul(BLOCKS["f29_mul_p1_asm", field], OLD["f29_mul_asm", field], FC.modulus(field), pairs) == len(pairs) > 4000


@pytest.mark.parametrize("field", FIELDS)
def test_sqr_block_equals_the_plain_block_and_the_exact_quotient(field):
    ops = sqr_operands(field)
    assert check_sqr(BLOCKS["f29_sqr_p1_asm", field], OLD["f29_sqr_asm", field], FC.modulus(field), ops) == len(ops) > 2000


@pytest.mark.parametrize("key", sorted(BLOCKS))
def test_self_check_deleted_increment_fails_the_values(key):
    b = BLOCKS[key]
    field = key[1]
    (i,) = [i for i, l in enumerate(b.lines) if l.startswith("v_lshl_add_u64")]
    edited = b.copy_with(b.lines[:i] + b.lines[i + 1:]).compile()        # still well-formed
    with pytest.raises(AssertionError):
        if "mul" in key[0]:
            check_mul(edited, OLD["f29_mul_asm", field], FC.modulus(field), mul_pairs(field)[-50:])
        else:
            check_sqr(edited, OLD["f29_sqr_asm", field], FC.modulus(field), sqr_operands(field)[-50:])


def test_self_check_operands_outside_the_contract_trip_the_signed_bound():
    b = BLOCKS["f29_mul_p1_asm", "PallasFp"]
    with pytest.raises(AssertionError, match="2\\^63"):
        b.run(*[M30] * 9, *[M30] * 9)                                    # 2^30 x 2^30: the plain block's contract, not this one's
    with pytest.raises(AssertionError, match="2\\^63"):
        b.run(*[MASK] * 9, *[(1 << 31) - 1] * 9)                         # tight x loose


def test_self_check_register_rules_hold_for_the_new_mnemonics():
    b = BLOCKS["f29_mul_p1_asm", "PallasFq"]
    i = next(i for i, l in enumerate(b.lines) if l.startswith("v_not_b32"))
    with pytest.raises(E.RegisterError):
        b.copy_with(b.lines[:i] + ["v_not_b32 v40, v16"] + b.lines[i:]).compile()
    with pytest.raises(E.RegisterError):
        b.copy_with(["v_ashrrev_i64 v[16:17], 29, v[16:17]"] + b.lines).compile()  # read before written
    with pytest.raises(E.AsmError):
        b.copy_with(b.lines + ["v_add_u32 v16, v16, v17"]).compile()


def test_generated_header_is_current():
    out = subprocess.run([sys.executable, os.path.join(E.CSRC, "gen_field29_asm.py"), "--p1"], check=True, capture_output=True).stdout
    with open(HEADER, "rb") as f:
        assert out == f.read(), "field29_mul_asm_p1.cuh differs from `python gen_field29_asm.py --p1`: regenerate it"


def test_the_new_mode_refuses_a_modulus_that_is_not_one_mod_2_29():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import gen_field29_asm as G\n"
            "G.gen_mul(G.FIELDS['PallasFp'], p1=True)\n"
            "try:\n    G.gen_mul(G.BN254FQ_FIELDS['Bn254Fq'], p1=True)\nexcept SystemExit as e:\n    print('refused:', e)\n")
    r = subprocess.run([sys.executable, "-c", code, E.CSRC], capture_output=True, text=True, check=True)
    assert "refused" in r.stdout and "not 1 mod 2^29" in r.stdout
