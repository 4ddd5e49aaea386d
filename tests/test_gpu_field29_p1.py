"""GPU: the Pasta products without the mads by modulus limb 0 (field29_mul_asm_p1.cuh behind f29_mul30 / f29_sqr30, and the
compiler's dot29_finish2) on the device, against Python integers and against the plain blocks; then through xyzz29_madd in two
small commitments.

tests/gpu_field/f29_p1_probe.hip runs one launch of 4 096 lanes per field: the edge operands of tests/test_asm_emulator_p1.py
(zeros - every reduction column then holds -1 -, zero low limbs, the contract limits, p - 1, p, p + 1, 2^261 mod p) and seeded
random pairs, tight x (limbs < 2^30).  The default build must give the exact Montgomery quotients; a second build with
-DLURK_F29_P1=0 (the plain blocks) must give the same bytes."""
import os
import subprocess

import numpy as np
import pytest

from tests import field_cases as FC
from tests import test_asm_emulator_p1 as P1
from tests.test_gpu_field_arith import as_int, hipcc, makefile_cxxflags

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "gpu_field", "f29_p1_probe.hip")
N = 4096


def operands(field):
    pairs = P1.mul_pairs(field)
    edge = [pr for pr in pairs[:-4000] if max(pr[0]) <= FC.MASK29]
    assert len(edge) < N - 1000
    pairs = edge + pairs[-2000:][: N - len(edge)]                     # the edges, then tight x (2^30 - 1)-bounded random pairs
    pairs += pairs[: N - len(pairs)]
    assert len(pairs) == N
    return (np.array([a for a, _ in pairs], dtype=np.uint32), np.array([b for _, b in pairs], dtype=np.uint32))


def test_probe_matches_python_integers_and_the_plain_blocks(tmp_path):
    exes = {}
    for name, defs in (("p1", []), ("plain", ["-DLURK_F29_P1=0"])):
        exes[name] = str(tmp_path / f"probe_{name}")
        subprocess.run([hipcc(), *makefile_cxxflags(), *defs, "-o", exes[name], PROBE], check=True, timeout=600)
    sets = {f: operands(f) for f in P1.FIELDS}
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as f:
        f.write(np.uint32(N).tobytes())
        for field in P1.FIELDS:
            f.write(sets[field][0].tobytes())
            f.write(sets[field][1].tobytes())
    outs = {}
    for name, exe in exes.items():
        r = subprocess.run([exe, inp, str(tmp_path / f"out_{name}.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"probe {name} exit {r.returncode}: {r.stdout}{r.stderr}"
        outs[name] = np.fromfile(str(tmp_path / f"out_{name}.bin"), dtype="<u4").reshape(2, N, 3, 9)
    for k, field in enumerate(P1.FIELDS):
        p = FC.modulus(field)
        A, B = sets[field]
        a, b, bt = as_int(A, 29), as_int(B, 29), as_int(B & FC.MASK29, 29)
        want = [a * b, a * a, a * bt + np.roll(a, -1) * np.roll(bt, -1)]
        for j, op in enumerate(("f29_mul30", "f29_sqr30", "dot29_finish2")):
            got = as_int(outs["p1"][k, :, j], 29)
            bad = np.nonzero(got != np.frompyfunc(lambda v: P1.redc(v, p), 1, 1)(want[j]))[0]
            assert bad.size == 0, (field, op, [(A[i].tolist(), B[i].tolist(), outs["p1"][k, i, j].tolist()) for i in bad[:4]])
            assert (outs["p1"][k, :, j, :8] <= FC.MASK29).all(), (field, op)
    assert np.array_equal(outs["p1"], outs["plain"]), "the blocks without the mads by limb 0 and the plain blocks give different limbs"


@pytest.mark.parametrize("cn,c", [("pallas", 0), ("vesta", 1)])
def test_msm_4096_points_16_bit_windows_against_the_naive_oracle(hip, cn, c):
    """xyzz29_madd in the bucket pipeline: scalar 0, scalar 1, repeated points (the doubling branch), P and -P (the identity branch)"""
    from oracle import coracle as C
    from oracle import pyref as R

    from lurk_beta_amd import CommitmentKey, point_to_affine

    q = R.CURVES[cn]["order"]
    n = 4096
    B = C.synth_bases(c, n)
    s = [R.uniform_fe(21, i, q) for i in range(n)]
    for i in range(0, 512, 8):
        B[i + 1] = B[i]
        s[i] = s[i + 1] = 12345 + i                      # same bucket, same point: doubling
        B[i + 3] = B[i + 2]
        s[i + 2], s[i + 3] = 777 + i, q - 777 - i        # P and -P in one bucket: identity mid-chain
        s[i + 4], s[i + 5] = 0, 1
    S = C.ints_to_limbs(s)
    want = C.jac_to_affine(c, C.msm_naive(c, B, S))
    for pre in (False, True):
        ck = CommitmentKey(c, B, precompute=pre, window_bits=16 if pre else 0)
        assert point_to_affine(c, ck.commit(S)) == want, pre
        ck.close()


def test_table_key_commitment_2_17_points_against_the_dlog_checksum(hip):
    import torch

    from oracle import coracle as C

    from lurk_beta_amd import CommitmentKey, point_to_affine, synth

    c, sf, n = 0, 1, 1 << 17
    d_bases = synth.bases(c, n)
    d_scalars = synth.scalars(sf, 1, 1, n, mont=True)
    torch.cuda.synchronize()
    ck = CommitmentKey(c, d_bases, n=n, device=True, precompute=True, window_bits=20)
    assert ck.info()["window_bits"] == 20
    got = point_to_affine(c, ck.commit_device(d_scalars, n, is_mont=True))
    want = C.jac_to_affine(c, C.gen_mul(c, C.dot(sf, C.synth_base_scalars(c, n), C.synth_scalars(sf, 1, 1, n))))
    assert got == want
    ck.close()
