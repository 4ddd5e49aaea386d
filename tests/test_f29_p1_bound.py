"""CPU: the tightened column bound of the Pasta products that drop the mads by modulus limb 0 (field29.cuh: f29_mul30, f29_sqr30,
dot29_finish2) is live under LURK_F29_CHECK.

Their signed shift wants every reduction column below 2^63: 9 la lb + 5 2^58 + carry < 2^63.  tests/host_bound/f29_bound.cpp is
built for the host with the checks on and fed operands whose nine limbs all hold one value: tight x (2^30 - 1) is inside the
contract and must give the plain product's limbs; 2^30 - 1 on both sides and tight x loose are inside the plain product's contract
(< 2^64) and outside this one's, so the Pasta path must abort with the column-overflow message, while BN254 Fr (not 1 mod 2^29:
f29_mul30 is the plain product there) and a build with -DLURK_F29_P1=0 must not."""
import os
import signal
import subprocess

import pytest

from tests import field_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_bound", "f29_bound.cpp")
MASK, M30, M31 = FC.MASK29, (1 << 30) - 1, (1 << 31) - 1
FIELD_NAMES = {v: k for k, v in FC.FIELDS.items()}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("f29_bound")
    out = {}
    for name, defs in (("p1", []), ("plain", ["-DLURK_F29_P1=0"])):
        out[name] = str(d / name)
        subprocess.run(["g++", "-O1", "-std=c++17", *defs, "-o", out[name], SRC], check=True, timeout=300)
    return out


def run(exe, field, op, la, lb):
    return subprocess.run([exe, str(field), op, str(la), str(lb)], capture_output=True, text=True, timeout=60)


def limbs(r):
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return [int(x) for x in r.stdout.split(":")[1].split()]


def redc(v, p):
    return (v + (-v * pow(p, -1, 1 << 261)) % (1 << 261) * p) >> 261


@pytest.mark.parametrize("field", [0, 1])
def test_inside_the_contract_the_pasta_path_gives_the_plain_limbs(exes, field):
    p = FC.modulus(FIELD_NAMES[field])
    for op, la, lb in (("mul30", MASK, M30), ("mul30", MASK, MASK), ("mul30", 0, M30), ("sqr30", MASK, MASK), ("dot2", MASK, MASK)):
        r = run(exes["p1"], field, op, la, lb)
        assert r.stdout.startswith("p1 form 1:"), r.stdout
        got = limbs(r)
        assert got == limbs(run(exes["plain"], field, op, la, lb)), (op, la, lb)
        a, b = FC.from29([la] * 9), FC.from29([lb] * 9)
        want = {"mul30": a * b, "sqr30": a * a, "dot2": 2 * a * b}[op]
        assert FC.from29(got) == redc(want, p), (op, la, lb)


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("op,la,lb,msg", [("mul30", M30, M30, "f29_mul column overflow"), ("mul30", MASK, M31, "f29_mul column overflow"),
                                          ("sqr30", M30, M30, "f29_mul column overflow"), ("dot2", MASK, M30, "dot29 column overflow")])
def test_outside_it_the_pasta_path_aborts_with_the_column_overflow_message(exes, field, op, la, lb, msg):
    r = run(exes["p1"], field, op, la, lb)
    assert r.returncode == -signal.SIGABRT, (r.returncode, r.stdout)
    assert f"F29 bound violated: {msg}" in r.stdout
    # the same operands are inside the plain forms' contract (columns < 2^64)
    plain = run(exes["plain"], field, op, la, lb)
    assert plain.stdout.startswith("p1 form 0:"), plain.stdout
    p = FC.modulus(FIELD_NAMES[field])
    a, b = FC.from29([la] * 9), FC.from29([lb] * 9)
    assert FC.from29(limbs(plain)) == redc({"mul30": a * b, "sqr30": a * a, "dot2": 2 * a * b}[op], p)


def test_the_wide_product_and_the_other_moduli_keep_the_old_limit(exes):
    for field in (0, 1, 2):
        assert limbs(run(exes["p1"], field, "mul", M30, M30)) == limbs(run(exes["plain"], field, "mul", M30, M30))
        assert limbs(run(exes["p1"], field, "mul", MASK, M31))
    r = run(exes["p1"], 2, "mul30", M30, M30)               # BN254 Fr: not 1 mod 2^29, the plain product
    assert r.stdout.startswith("p1 form 0:") and limbs(r) == limbs(run(exes["p1"], 2, "mul", M30, M30))
