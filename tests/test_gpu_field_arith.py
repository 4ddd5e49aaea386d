"""GPU: the device arithmetic layer (field.cuh, field29.cuh and the generated asm blocks) one operation per lane, against Python
integers.

tests/gpu_field/field_probe.hip is compiled here with the Makefile's CXXFLAGS in two variants: the default one, where fe_mul is
the noinline fe_mul_call, and LURK_MUL_FORCE_INLINE, the way the MSM accumulation kernels compile it.  The operand registers
the compiler chose around every asm block of each variant are checked by bench_tools/check_asm_operands.py.  Each variant runs
once as a child process: inputs go in through a file, outputs come back through one.  The probe runs every op with 64 and with
256 threads per block and fails unless the two agree.

Operands per field: the cross product of tests/field_cases.structured (the pair index walks the second operand fastest, so
neighbouring lanes of a wave take different carry outcomes), 2^18 seeded uniform pairs, the radix-2^29 contract limits, and one
set in which every lane takes the same pair.  The emulator test (test_asm_emulator.py) models one lane; carries here are real
lane masks."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import field_cases as FC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "gpu_field", "field_probe.hip")
N_UNIFORM = 1 << 18

OPS = {name: i for i, name in enumerate(
    ["fe_add", "fe_sub", "fe_neg", "fe_mul", "fe_sqr", "fe_to_mont", "fe_from_mont", "fe_inv", "fe_dot3", "fe_dot9",
     "f29_mul", "f29_sqr", "f29_add", "f29_sub", "f29_carry", "f29_from_mont256", "f29_to_mont256", "f29_invert", "f29_dot3",
     "f29_dot9"])}
FE_OPS = [o for o in OPS if o.startswith("fe_")]
# ops on canonical operands given as 8 x 32 words (the f29 ones take the 9 x 29 limbs of the same integer)
CANONICAL_OPS = FE_OPS + ["f29_mul", "f29_sqr", "f29_add", "f29_sub", "f29_from_mont256", "f29_to_mont256", "f29_invert",
                          "f29_dot3", "f29_dot9"]


def hipcc():
    path = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(path), "hipcc not found: the probe cannot be built"
    return path


def makefile_cxxflags():
    mk = open(os.path.join(ROOT, "lurk_beta_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def build_probe(tmp, variant_defs):
    os.makedirs(tmp, exist_ok=True)
    exe = os.path.join(tmp, "field_probe")
    subprocess.run([hipcc(), *makefile_cxxflags(), *variant_defs, "-save-temps", "-o", exe, PROBE], cwd=tmp, check=True,
                   timeout=600)
    (asm,) = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")]
    chk = subprocess.run([sys.executable, os.path.join(ROOT, "bench_tools", "check_asm_operands.py"), os.path.join(tmp, asm)],
                         capture_output=True, text=True, timeout=300)
    assert chk.returncode == 0, chk.stdout + chk.stderr
    assert re.search(r"matched blocks: [1-9]\d* overlaps: 0", chk.stdout), chk.stdout
    return exe


# ---- operand sets ---------------------------------------------------------------------------------------------------------
def words8(vals):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u4").reshape(len(vals), 8)


def limbs9(vecs):
    return np.array(vecs, dtype=np.uint32).reshape(len(vecs), 9)


def as_int(arr, w):
    acc = np.zeros(arr.shape[0], dtype=object)
    for k in reversed(range(arr.shape[1])):
        acc = (acc << w) + arr[:, k].astype(np.uint64).astype(object)
    return acc


def operand_sets():
    """[(field, name, width, ops, A, B)]"""
    sets = []
    for field in FC.FIELDS:
        p = FC.modulus(field)
        s = FC.structured(field)
        u = FC.uniform(field, 2 * N_UNIFORM, "gpu")
        a = [x for x in s for _ in s] + u[::2]
        b = [y for _ in s for y in s] + u[1::2]
        sets.append((field, "canonical", 8, CANONICAL_OPS, words8(a), words8(b)))
        sets.append((field, "same pair", 8, CANONICAL_OPS, words8([p - 1] * 256), words8([p - 2] * 256)))
        tight, loose31, both30 = FC.limit_vectors(FC.MASK29), FC.limit_vectors((1 << 31) - 1), FC.limit_vectors((1 << 30) - 1)
        st = [FC.to29(x) for x in s]
        pa = [x for x in tight + st for _ in loose31] + [y for _ in tight + st for y in loose31]
        pb = [y for _ in tight + st for y in loose31] + [x for x in tight + st for _ in loose31]
        pa += [x for x in both30 for _ in both30] + FC.uniform_limbs(4096, FC.MASK29, 1)
        pb += [y for _ in both30 for y in both30] + FC.uniform_limbs(4096, (1 << 31) - 1, 2)
        sets.append((field, "limits", 9, ["f29_mul"], limbs9(pa), limbs9(pb)))
        sets.append((field, "same limits", 9, ["f29_mul"], limbs9([[FC.MASK29] * 9] * 256), limbs9([[(1 << 31) - 1] * 9] * 256)))
        ta = tight + FC.uniform_limbs(4096, FC.MASK29, 3)
        sets.append((field, "tight limits", 9, ["f29_sqr", "f29_to_mont256", "f29_carry"], limbs9(ta), limbs9(ta)))
        la = loose31 + both30 + FC.uniform_limbs(4096, (1 << 31) - 1, 4)
        sets.append((field, "loose limits", 9, ["f29_carry"], limbs9(la), limbs9(la)))
        # f29_sub: minuend tight or < 2^30; every subtrahend limb at most the matching limb of the 64p bias (field29.cuh),
        # up to the bias itself
        bias = [x + ((1 << 30) if i < 8 else 0) - (2 if i else 0) for i, x in enumerate(FC.to29(64 * p))]
        subs = [FC.to29(y) for y in (0, 1, p - 1, 2 * p, int(2 ** 259.5))] + [bias, [bias[i] if i % 2 else 0 for i in range(9)]]
        sa = [x for x in tight + both30 + st for _ in subs]
        sb = [y for _ in tight + both30 + st for y in subs]
        sets.append((field, "sub limits", 9, ["f29_sub", "f29_add"], limbs9(sa), limbs9(sb)))
    return sets


def write_input(path, sets):
    with open(path, "wb") as f:
        f.write(np.uint32(len(sets)).tobytes())
        for field, _, width, ops, A, B in sets:
            f.write(np.array([FC.FIELDS[field], A.shape[0], width, len(ops)] + [OPS[o] for o in ops], dtype="<u4").tobytes())
            f.write(np.ascontiguousarray(A, dtype="<u4").tobytes())
            f.write(np.ascontiguousarray(B, dtype="<u4").tobytes())


def split_output(path, sets):
    data = np.fromfile(path, dtype="<u4")
    out, off = {}, 0
    for k, (_, _, _, ops, A, _) in enumerate(sets):
        for o in ops:
            n = A.shape[0] * 9
            out[k, o] = data[off:off + n].reshape(A.shape[0], 9)
            off += n
    assert off == data.size, "probe output has the wrong size"
    return out


# ---- expected values ------------------------------------------------------------------------------------------------------
def _redc(v, p, rbits):
    pinv = pow(p, -1, 1 << rbits)
    mask = (1 << rbits) - 1
    m = ((-v) * pinv) & mask
    return (v + m * p) >> rbits


def _inv(p, scale):
    return np.frompyfunc(lambda x: pow(x, -1, p) * scale % p if x % p else 0, 1, 1)


def _window(x, T):
    return sum(np.roll(x, -j) for j in range(T))


def check(field, op, width, A, B, O):
    """asserts every row of O for op; returns the number of rows checked"""
    p = FC.modulus(field)
    w = 32 if width == 8 else 29
    a, b = as_int(A, w), as_int(B, w)
    R, Ri = (1 << 256) % p, pow(1 << 256, -1, p)
    lo29 = O[:, :8] <= FC.MASK29
    if op.startswith("fe_") or op == "f29_to_mont256":
        got = as_int(O[:, :8], 32)
        assert (O[:, 8] == 0).all()
        want = {
            "fe_add": lambda: (a + b) % p,
            "fe_sub": lambda: (a - b) % p,
            "fe_neg": lambda: (-a) % p,
            "fe_mul": lambda: a * b * Ri % p,
            "fe_sqr": lambda: a * a * Ri % p,
            "fe_to_mont": lambda: a * R % p,
            "fe_from_mont": lambda: a * Ri % p,
            "fe_inv": lambda: _inv(p, R * R % p)(a),            # the exponentiation in the Montgomery domain: R^2 / a
            "fe_dot3": lambda: _window(a * b, 3) * Ri % p,
            "fe_dot9": lambda: _window(a * b, 9) * Ri % p,
            "f29_to_mont256": lambda: a * pow(32, -1, p) % p,   # 2^261 domain -> 2^256 domain, canonical
        }[op]()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (field, op, [(hex(a[i]), hex(b[i]), hex(got[i]), hex(want[i])) for i in bad[:4]])
        return len(got)
    got = as_int(O, 29)
    tight = (O <= FC.MASK29).all(axis=1)
    if op in ("f29_mul", "f29_sqr", "f29_dot3", "f29_dot9"):
        bb = a if op == "f29_sqr" else b
        if op.startswith("f29_dot"):
            want = _redc(_window(a * b, int(op[-1])), p, 261)
        else:
            want = _redc(a * bb, p, 261)
        assert lo29.all(), (field, op)
        # the top limb is tight when a*b < 2^261 (2^261 - p): always for operands below 2^260, and for any canonical one
        need_tight = (a * bb) < (1 << 261) * ((1 << 261) - p) if op != "f29_dot9" else np.ones(len(a), dtype=bool)
        assert tight[need_tight.astype(bool)].all(), (field, op)
    elif op == "f29_add":
        want = a + b
        if width == 9:
            assert (O == A.astype(np.uint64) + B.astype(np.uint64)).all(), (field, op)
    elif op == "f29_sub":
        want = a - b + 64 * p                                   # the bias is 64p with re-balanced limbs
        tight_a = (A <= FC.MASK29).all(axis=1) if width == 9 else np.ones(len(A), dtype=bool)
        assert (O[tight_a] < (1 << 31)).all(), (field, op)      # loose when the minuend is tight
    elif op == "f29_carry":
        want = a
        assert lo29.all(), (field, op)
    elif op == "f29_from_mont256":
        want = a << 5
        assert tight.all(), (field, op)
    elif op == "f29_invert":
        assert tight.all(), (field, op)
        got = got % p
        want = _inv(p, pow(2, 522, p))(a)                       # Montgomery(2^261) inverse: R'^2 / a
    else:
        raise AssertionError(op)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (field, op, [(A[i].tolist(), B[i].tolist(), O[i].tolist()) for i in bad[:4]])
    return len(got)


def run_probe(exe, inp, outp):
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"probe exit {r.returncode}: {r.stdout}{r.stderr}"
    return r.stdout


def test_device_field_arithmetic_against_python_integers(tmp_path):
    default = build_probe(str(tmp_path / "default"), [])
    inline = build_probe(str(tmp_path / "inline"), ["-DLURK_MUL_FORCE_INLINE"])
    sets = operand_sets()
    inp = str(tmp_path / "in.bin")
    write_input(inp, sets)
    run_probe(default, inp, str(tmp_path / "out_default.bin"))
    out = split_output(str(tmp_path / "out_default.bin"), sets)
    counts = {}
    for k, (field, _, width, ops, A, B) in enumerate(sets):
        for op in ops:
            counts[field, op] = counts.get((field, op), 0) + check(field, op, width, A, B, out[k, op])
    del out
    run_probe(inline, inp, str(tmp_path / "out_inline.bin"))
    same = np.array_equal(np.fromfile(str(tmp_path / "out_default.bin"), dtype="<u4"),
                          np.fromfile(str(tmp_path / "out_inline.bin"), dtype="<u4"))
    if not same:  # name the op that differs
        out = split_output(str(tmp_path / "out_inline.bin"), sets)
        for k, (field, _, width, ops, A, B) in enumerate(sets):
            for op in ops:
                check(field, op, width, A, B, out[k, op])
    assert same, "LURK_MUL_FORCE_INLINE build computes different bytes"
    print("\nrows checked per field and op (each in both builds, with 64 and 256 threads per block):")
    for field in FC.FIELDS:
        print(f"  {field}: " + ", ".join(f"{op} {counts[field, op]}" for op in OPS if (field, op) in counts))
    assert all(counts[f, op] >= N_UNIFORM for f in FC.FIELDS for op in CANONICAL_OPS)
