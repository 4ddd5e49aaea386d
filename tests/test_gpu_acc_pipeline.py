"""The pipelined task loop of the persistent bucket accumulation (curve29.cuh, msm_acc_persistent.hip) on the GPU: commitments small
enough for a test, forced through the persistent kernel, against the CPU oracle.

LURK_MSM_ACC_PERSISTENT=2 sends every DEFAULT-class commitment in flight through the persistent form whatever its size: one wave per
SIMD, the pipelined loop.  LURK_MSM_BUCKET_DIRECT=0 keeps a short FOLLOW-class commitment on the planned stages, where its accumulation
is the persistent kernel on the slot stream (with the one-launch direct form it would never reach the kernel under test): at two waves
per SIMD, the default, that is the kernel's plain-loop instantiation, and one case sets LURK_MSM_FOLLOW_WGS=1 so that the FOLLOW class
runs the pipelined loop as well.  The switches are read once per process, so each case is a child interpreter (as in
tests/test_gpu_switches.py).

The scalar vectors pick the task shapes: all zero (no task), all equal (one full bucket per window: 64-entry tasks and the big-bucket
path), zero except for groups of one, two and three points with one scalar each (tasks of length 1, 2 and 3: the copy, the
affine + affine form, the first steady trip, the clamped look-ahead at every distance from the end), and the oracle's uniform and
witness vectors.  A second key repeats some records and holds the negation of others (y negated with Python integers), with equal
scalars on them, so that the out-of-line doubling and the cancellation to the identity happen inside tasks while a prefetch is in flight.

Pallas commitments must equal oracle.coracle.msm_fast.  The C oracle has no BN254; that case is held to this suite's BN254 reference,
the discrete-log checksum of tests/bn254_ref.py (Python integers)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = {"LURK_MSM_ACC_PERSISTENT": "2", "LURK_MSM_BUCKET_DIRECT": "0"}

PALLAS_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch
import lurk_beta_amd as L
from oracle import coracle as C
n, window_bits = %(n)d, %(window_bits)d
P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001   # the base field of Pallas
Q = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001   # its scalar field

def neg_y(rec):          # (x, y) limbs -> (x, p - y): the negated point, in whichever form (canonical or Montgomery) the limbs are
    y = C.limbs_to_ints(rec[4:8])[0]
    out = rec.copy()
    out[4:8] = C.ints_to_limbs([P - y])[0]
    return out

def scalar(seed):        # a full-width scalar
    return C.limbs_to_ints(C.synth_scalars(1, seed, 0, 1))[0]

def sparse(groups):      # zero except for the groups: [(positions, scalar)]
    v = np.zeros((n, 4), dtype=np.uint64)
    for pos, s in groups:
        v[list(pos)] = C.ints_to_limbs([s])[0]
    return v

B = C.synth_bases(0, n)
# the second key: repeats and negations
B2 = B.copy()
B2[6] = B2[5]                                    # P P
B2[101] = neg_y(B2[100])                         # P -P
B2[201] = B2[200]; B2[202] = neg_y(B2[200])      # P P -P
B2[301] = neg_y(B2[300]); B2[303] = B2[302]      # P -P Q Q
B2[n - 1] = B2[n - 2]                            # the last two records of the key
special = [((5, 6), scalar(901)), ((100, 101), scalar(902)), ((200, 201, 202), scalar(903)), ((300, 301, 302, 303), scalar(904)), ((n - 2, n - 1), scalar(905))]
dense2 = C.synth_scalars(1, 77, 0, n)            # the same pairs inside ordinary buckets
for pos, s in special:
    dense2[list(pos)] = C.ints_to_limbs([s])[0]

vectors = [
    ("zero", B, np.zeros((n, 4), dtype=np.uint64)),
    ("all equal", B, np.tile(C.ints_to_limbs([scalar(900)]), (n, 1))),
    ("groups of one, two, three", B, sparse([((7,), scalar(910)), ((1000, 2000), scalar(911)), ((11, n // 2, n - 1), scalar(912)), ((0,), 1), ((3,), Q - 1)])),
    ("uniform", B, C.synth_scalars(1, 40, 0, n)),
    ("witness", B, C.synth_scalars(1, 41, 1, n)),
    ("repeats and negations alone", B2, sparse(special)),
    ("repeats and negations in dense buckets", B2, dense2),
    ("repeats and negations, all equal", B2, np.tile(C.ints_to_limbs([scalar(906)]), (n, 1))),
]
keys = {}
for name, bases, v in vectors:
    if id(bases) not in keys:
        keys[id(bases)] = L.CommitmentKey(0, bases, precompute=True, window_bits=window_bits)
        keys[id(bases)].reserve(n, 3)
want = [C.jac_to_affine(0, C.msm_fast(0, bases, v)) for _, bases, v in vectors]
dev = [torch.from_numpy(C.to_mont(1, v).view(np.int64)).cuda() for _, _, v in vectors]
torch.cuda.synchronize()
assert want[0] == (0, 0) and want[1] != (0, 0)
# DEFAULT class, three in flight: the persistent kernel at one wave per SIMD
for lo in range(0, len(vectors), 3):
    batch = list(range(lo, min(lo + 3, len(vectors))))
    for slot, k in enumerate(batch):
        keys[id(vectors[k][1])].submit_device(slot, dev[k], n, is_mont=True)
    for slot, k in enumerate(batch):
        got = L.point_to_affine(0, keys[id(vectors[k][1])].wait(slot))
        assert got == want[k], ("DEFAULT", vectors[k][0])
# FOLLOW class: the persistent kernel on the slot stream (two waves per SIMD unless LURK_MSM_FOLLOW_WGS says otherwise), with nothing to
# follow and behind a foreground commitment
for k in (2, 5):
    key = keys[id(vectors[k][1])]
    key.submit_device(0, dev[k], n, is_mont=True, mode=3)
    assert L.point_to_affine(0, key.wait(0)) == want[k], ("FOLLOW", vectors[k][0])
key = keys[id(B)]
key.submit_device(1, dev[3], n, is_mont=True, mode=1)
key.submit_device(0, dev[4], n, is_mont=True, mode=3)
assert L.point_to_affine(0, key.wait(0)) == want[4] and L.point_to_affine(0, key.wait(1)) == want[3], "FOLLOW behind FOREGROUND"
for k in keys.values():
    k.close()
print("child ok")
'''

BN254_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch
from lurk_beta_amd import CommitmentKey, point_to_affine, synth
from tests import bn254_ref as R
cid, n = R.CURVE_BN254, 1 << 17
c = R.CURVES[cid]
q = c.order
bases = synth.bases(cid, n)
key = CommitmentKey(cid, bases, n=n, device=True, precompute=True, window_bits=16)
key.reserve(n, 3)

def sparse(groups):
    v = np.zeros((n, 4), dtype=np.uint64)
    for pos, s in groups:
        v[list(pos)] = np.array(R.ints_to_limbs([s]), dtype=np.uint64)[0]
    return v

r = c.synth_scalars(9, 0, 4)
host = [
    ("zero", np.zeros((n, 4), dtype=np.uint64)),
    ("all equal", np.tile(np.array(R.ints_to_limbs([r[0]]), dtype=np.uint64), (n, 1))),
    ("groups of one, two, three", sparse([((7,), r[1]), ((1000, 2000), r[2]), ((11, n // 2, n - 1), r[3]), ((0,), 1), ((3,), q - 1)])),
    ("uniform", synth.scalars(c.scalar_field, 40, 0, n).cpu().numpy().view(np.uint64).reshape(n, 4)),
    ("witness", synth.scalars(c.scalar_field, 41, 1, n).cpu().numpy().view(np.uint64).reshape(n, 4)),
]
want = [R.dlog_checksum_np(c, np.ascontiguousarray(v)) for _, v in host]
dev = [torch.from_numpy(np.ascontiguousarray(v).view(np.int64)).cuda() for _, v in host]
torch.cuda.synchronize()
assert want[0] is None and want[1] is not None
for lo in range(0, len(host), 3):
    batch = list(range(lo, min(lo + 3, len(host))))
    for slot, k in enumerate(batch):
        key.submit_device(slot, dev[k], n)
    for slot, k in enumerate(batch):
        assert R.from_xy(point_to_affine(cid, key.wait(slot))) == want[k], ("DEFAULT", host[k][0])
key.submit_device(0, dev[2], n, mode=3)
assert R.from_xy(point_to_affine(cid, key.wait(0))) == want[2], "FOLLOW"
key.close()
print("child ok")
'''


def _run(child, env=None, **kw):
    e = dict(os.environ)
    e.update(ENV)
    e.update(env or {})
    p = subprocess.run([sys.executable, "-c", child % dict(root=ROOT, **kw)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "child ok" in p.stdout


@pytest.mark.parametrize("n,window_bits,env", [(1 << 17, 16, {}), (4096, 20, {}), (4096, 20, {"LURK_MSM_FOLLOW_WGS": "1"})])
def test_pallas_commitments_through_the_pipelined_persistent_kernel(hip, n, window_bits, env):
    _run(PALLAS_CHILD, env=env, n=n, window_bits=window_bits)


def test_bn254_commitments_through_the_pipelined_persistent_kernel(hip):
    _run(BN254_CHILD)
