"""One-lane emulator of the generated gfx950 multiplier asm blocks (field_mul_asm.cuh, field29_mul_asm.cuh).

Both headers are device-only: the host build of field.cuh / field29.cuh switches to portable code, so nothing on the CPU ever
executes the asm text itself.  This module parses every block of both headers (instruction strings, operand list, clobber
list) and checks it for one lane of a wave:

  * hazards - gen_field_asm.py's rule: a VALU that writes an SGPR (the carry-out pair of v_mad_u64_u32, the vcc of
    v_addc_co_u32) must be separated by at least two wait states from any VALU that reads that SGPR.  Every instruction
    counts as one wait state, `s_nop N` as N + 1.  Nothing inside an asm string is padded by the compiler, so a missed pad
    gives wrong carries on some waves with no fault.  vcc is a write-only sink in these blocks: reading it is an error.
  * registers - every register read was written earlier in the block or is an input operand; every write goes to an
    output operand or to a declared clobber; every output operand is written.
  * values - `Block.run` executes the block on Python integers (32-bit VGPRs and SGPRs; a carry-out lane mask is modelled
    by its lane-0 bit), so the tests can compare the result with exact big-integer arithmetic.

Only the nine mnemonics the generators emit are understood; anything else is an error.  The block has no branches, so the
hazard and register checks do not depend on the operand values: they run once, when a Block is compiled.
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lurk_beta_amd", "csrc")
HEADERS = (os.path.join(CSRC, "field_mul_asm.cuh"), os.path.join(CSRC, "field29_mul_asm.cuh"))

MNEMONICS = ("v_mad_u64_u32", "v_addc_co_u32_e64", "v_mov_b32", "v_sub_u32", "v_mul_lo_u32", "v_and_b32",
             "v_lshrrev_b64", "s_mov_b32", "s_nop")
HAZARD_WAIT_STATES = 2
M32 = 0xFFFFFFFF


class AsmError(Exception):
    pass


class HazardError(AsmError):
    pass


class RegisterError(AsmError):
    pass


_BLOCK_RE = re.compile(r"__device__ __forceinline__ [^\n]*?\b(\w+_asm)<(\w+)>\([^\n]*\{\n(?:[^\n]*\n)*?\s*asm(?:\s+volatile)?\(\s*"
                       r"((?:\s*\"[^\"\n]*\"\s*\n?)+)\s*:\s*([^;]*?);")


def _regs(text):
    """operand text -> list of 32-bit register names it covers, or None for a constant"""
    text = text.strip()
    m = re.fullmatch(r"([vs])(\d+)", text)
    if m:
        return [text]
    m = re.fullmatch(r"([vs])\[(\d+):(\d+)\]", text)
    if m:
        return [f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)]
    m = re.fullmatch(r"%(\d+)", text)
    if m:
        return [f"o{m.group(1)}"]
    if text == "vcc":
        return ["vcc_lo", "vcc_hi"]
    if re.fullmatch(r"0x[0-9a-fA-F]+|\d+", text):
        return None
    raise AsmError(f"unknown operand {text!r}")


def _const(text):
    return int(text, 0)


class Block:
    """One asm statement: `name` (fe_mul_asm, fe_redc16_asm, f29_mul_asm, f29_sqr_asm), `field`, its instruction lines,
    n_out output operands followed by n_in input operands, and the declared clobbers."""

    def __init__(self, name, field, lines, n_out, n_in, clobbers):
        self.name, self.field, self.lines = name, field, list(lines)
        self.n_out, self.n_in, self.clobbers = n_out, n_in, set(clobbers)
        self._fn = None

    def copy_with(self, lines):
        return Block(self.name, self.field, lines, self.n_out, self.n_in, self.clobbers)

    # ---- static checks + translation to Python ------------------------------------------------------------------
    def compile(self):
        """Checks hazards and register use (raises HazardError / RegisterError) and builds the value function."""
        written = set()
        clob = set()
        for c in self.clobbers:
            clob.update(["vcc_lo", "vcc_hi"] if c == "vcc" else [c])
        sgpr_valu_write = {}   # sgpr -> wait-state clock of the VALU that wrote it
        clock = 0
        py = []

        def read(regs, idx, valu):
            for r in regs or ():
                if r.startswith("vcc"):
                    raise HazardError(f"line {idx}: reads vcc ({self.lines[idx]})")
                if valu and r in sgpr_valu_write:
                    gap = clock - sgpr_valu_write[r] - 1
                    if gap < HAZARD_WAIT_STATES:
                        raise HazardError(f"line {idx}: {r} read {gap} wait state(s) after a VALU wrote it ({self.lines[idx]})")
                if r.startswith("o") and int(r[1:]) >= self.n_out:
                    continue           # input operand
                if r not in written:
                    raise RegisterError(f"line {idx}: {r} read before it is written ({self.lines[idx]})")

        def write(regs, idx, valu):
            for r in regs:
                if r.startswith("o"):
                    if int(r[1:]) >= self.n_out:
                        raise RegisterError(f"line {idx}: writes input operand {r} ({self.lines[idx]})")
                elif r not in clob:
                    raise RegisterError(f"line {idx}: writes {r}, which is not a declared clobber ({self.lines[idx]})")
                written.add(r)
                if r[0] == "s" or r.startswith("vcc"):
                    if valu:
                        sgpr_valu_write[r] = clock
                    else:
                        sgpr_valu_write.pop(r, None)

        def val32(text):
            regs = _regs(text)
            if regs is None:
                return str(_const(text) & M32)
            if len(regs) != 1:
                raise AsmError(f"32-bit operand expected: {text}")
            return regs[0]

        def val64(text):
            regs = _regs(text)
            if regs is None:
                return str(_const(text))
            if len(regs) != 2:
                raise AsmError(f"64-bit operand expected: {text}")
            return f"({regs[0]} | ({regs[1]} << 32))"

        for idx, line in enumerate(self.lines):
            mn, _, rest = line.partition(" ")
            ops = [o.strip() for o in rest.split(",")] if rest.strip() else []
            if mn not in MNEMONICS:
                raise AsmError(f"line {idx}: mnemonic {mn!r} is not modelled")
            valu = mn.startswith("v_")
            if mn == "s_nop":
                clock += _const(ops[0]) + 1
                continue
            if mn == "v_mad_u64_u32":       # D64, SDST64 = S0 * S1 + S2(64)
                d, sd, s0, s1, s2 = ops
                for o in (s0, s1):
                    read(_regs(o), idx, valu)
                read(_regs(s2), idx, valu)
                dr, sr = _regs(d), _regs(sd)
                py.append(f"t = {val32(s0)} * {val32(s1)} + {val64(s2)}")
                py.append(f"{dr[0]} = t & {M32}; {dr[1]} = (t >> 32) & {M32}; {sr[0]} = t >> 64; {sr[1]} = 0")
                write(dr + sr, idx, valu)
            elif mn == "v_addc_co_u32_e64":  # D, SDST = S0 + S1 + carry-in(S2 lane mask)
                d, sd, s0, s1, s2 = ops
                for o in (s0, s1, s2):
                    read(_regs(o), idx, valu)
                cr = _regs(s2)
                if cr is None or len(cr) != 2:
                    raise AsmError(f"line {idx}: carry-in must be an SGPR pair")
                dr, sr = _regs(d), _regs(sd)
                py.append(f"t = {val32(s0)} + {val32(s1)} + ({cr[0]} & 1)")
                py.append(f"{dr[0]} = t & {M32}; {sr[0]} = t >> 32; {sr[1]} = 0")
                write(dr + sr, idx, valu)
            elif mn in ("v_mov_b32", "s_mov_b32"):
                d, s0 = ops
                read(_regs(s0), idx, valu)
                py.append(f"{val32(d)} = {val32(s0)}")
                write(_regs(d), idx, valu)
            elif mn in ("v_sub_u32", "v_mul_lo_u32", "v_and_b32"):
                d, s0, s1 = ops
                read(_regs(s0), idx, valu)
                read(_regs(s1), idx, valu)
                op = {"v_sub_u32": "-", "v_mul_lo_u32": "*", "v_and_b32": "&"}[mn]
                py.append(f"{val32(d)} = ({val32(s0)} {op} {val32(s1)}) & {M32}")
                write(_regs(d), idx, valu)
            elif mn == "v_lshrrev_b64":      # D64 = S1(64) >> S0
                d, s0, s1 = ops
                read(_regs(s0), idx, valu)
                read(_regs(s1), idx, valu)
                dr = _regs(d)
                py.append(f"t = {val64(s1)} >> ({val32(s0)} & 63)")
                py.append(f"{dr[0]} = t & {M32}; {dr[1]} = (t >> 32) & {M32}")
                write(dr, idx, valu)
            clock += 1
        missing = [f"o{i}" for i in range(self.n_out) if f"o{i}" not in written]
        if missing:
            raise RegisterError(f"output operands never written: {missing}")
        args = ", ".join(f"o{i}" for i in range(self.n_out, self.n_out + self.n_in))
        src = f"def _block({args}):\n" + "".join(f"    {l}\n" for l in py)
        src += "    return (" + "".join(f"o{i}, " for i in range(self.n_out)) + ")\n"
        ns = {}
        exec(compile(src, f"<{self.name}<{self.field}>>", "exec"), ns)
        self._fn = ns["_block"]
        return self

    def run(self, *inputs):
        """inputs: the n_in 32-bit input operand values in operand order; returns the n_out output words"""
        if self._fn is None:
            self.compile()
        if len(inputs) != self.n_in or any(not 0 <= x <= M32 for x in inputs):
            raise ValueError("input operands must be n_in 32-bit words")
        return self._fn(*inputs)


def parse_header(path):
    src = open(path).read()
    blocks = []
    for m in _BLOCK_RE.finditer(src):
        name, field, body, tail = m.groups()
        lines = [l.replace("\\n", "").replace("\\t", "").strip() for l in re.findall(r'"([^"\n]*)"', body)]
        lines = [l for l in lines if l]
        parts = tail.split(":")
        if len(parts) != 3:
            raise AsmError(f"{name}<{field}>: expected outputs : inputs : clobbers")
        outs = re.findall(r'"([^"]*)"\([^()]*\)', parts[0])
        ins = re.findall(r'"([^"]*)"\([^()]*\)', parts[1])
        if any(c != "=&v" for c in outs) or any(c != "v" for c in ins):
            raise AsmError(f"{name}<{field}>: unexpected constraints {outs} {ins}")
        clobbers = re.findall(r'"([^"]*)"', parts[2])
        blocks.append(Block(name, field, lines, len(outs), len(ins), clobbers))
    return blocks


def all_blocks():
    """{(name, field): Block} for every asm block of both generated headers"""
    out = {}
    for h in HEADERS:
        for b in parse_header(h):
            out[(b.name, b.field)] = b
    return out
