"""The mixed addition on signed limbs (curve29.cuh: xyzz29_madd_s) in the bucket accumulation on the GPU, both Pasta curves: keys of
2^16 + 1 points - the smallest that takes the bucket pipeline - and of 2^17, as a window table and as a plain key, committed
synchronously (the plain launch or the one-launch direct form) and two in flight (LURK_MSM_ACC_PERSISTENT=2: the persistent kernel at
this size, with both task lengths, LURK_MSM_PERSIST_S = 64 and 128).  One child runs with LURK_MSM_BUCKET_DIRECT=0 so that the
synchronous commitments go through the plain accumulate launch.  The switches are read once per process: each setting is a child.

Scalars: a uniform vector whose first entries are 0, 1 and r - 1; a key that repeats records, holds the negation of others (y negated
with Python integers) and three identity records, under equal scalars on those groups - alone (tasks of two to four entries: the
doubling, the cancellation to the identity and more bases behind it) and inside dense buckets.

Every commitment must equal the oracle's Pippenger (oracle.coracle.msm_pippenger); the vector on the unmodified key also the
discrete-log checksum [sum s_i k_i] G.  The references are computed once per curve, here, and handed to the children.  (One library is
built per tree, so the LURK_ACC_SIGNED=0 build is not loaded beside it: the oracle alone decides.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import coracle as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1 << 16) + 1, 1 << 17)
BASE_FIELD_MODULUS = {0: 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001,   # Pallas: Fp
                      1: 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001}   # Vesta: Fq

# the inputs, rebuilt identically in the parent (references) and in the children (commitments)
INPUTS = r'''
import numpy as np
from oracle import coracle as C
BASE_FIELD_MODULUS = %(moduli)r

def inputs(c, n):
    sf = 1 - c
    p = BASE_FIELD_MODULUS[c]
    order = BASE_FIELD_MODULUS[1 - c]
    def neg_y(rec):
        out = rec.copy()
        out[4:8] = C.ints_to_limbs([p - C.limbs_to_ints(rec[4:8])[0]])[0]
        return out
    scalar = lambda seed: C.limbs_to_ints(C.synth_scalars(sf, seed, 0, 1))[0]
    B = C.synth_bases(c, n)
    B2 = B.copy()
    B2[6] = B2[5]                                    # P P
    B2[101] = neg_y(B2[100])                         # P -P
    B2[201] = B2[200]; B2[202] = neg_y(B2[200])      # P P -P
    B2[301] = neg_y(B2[300]); B2[303] = B2[302]      # P -P Q Q
    B2[n - 1] = B2[n - 2]                            # the last two records of the key
    for k in (0, n // 2, n - 3):                     # identity records
        B2[k] = 0
    special = [((5, 6), scalar(901)), ((100, 101), scalar(902)), ((200, 201, 202), scalar(903)), ((300, 301, 302, 303, 0), scalar(904)),
               ((n - 3, n - 2, n - 1), scalar(905)), ((n // 2,), 1)]
    edge = C.synth_scalars(sf, 40, 0, n)
    edge[0:3] = C.ints_to_limbs([0, 1, order - 1])
    sparse = np.zeros((n, 4), dtype=np.uint64)
    dense = C.synth_scalars(sf, 77, 0, n)
    for pos, s in special:
        sparse[list(pos)] = C.ints_to_limbs([s])[0]
        dense[list(pos)] = C.ints_to_limbs([s])[0]
    return B, B2, [("0, 1, r - 1 and uniform", 0, edge), ("repeats, negations, identities alone", 1, sparse), ("the same in dense buckets", 1, dense)]
''' % dict(moduli=BASE_FIELD_MODULUS)

CHILD = INPUTS + r'''
import json, sys
import torch
import lurk_beta_amd as L
c = %(c)d
want = json.load(open(%(want)r))
for n in %(sizes)r:
    sf = 1 - c
    B, B2, vectors = inputs(c, n)
    dev = [torch.from_numpy(C.to_mont(sf, v).view(np.int64)).cuda() for _, _, v in vectors]
    torch.cuda.synchronize()
    for pre in (True, False):
        keys = [L.CommitmentKey(c, b, precompute=pre) for b in (B, B2)]
        for key in keys:
            key.reserve(n, 2)
        for k, (name, which, _) in enumerate(vectors):
            w = tuple(want["%%d %%d" %% (n, k)])
            got = L.point_to_affine(c, keys[which].commit_device(dev[k], n, is_mont=True))
            assert got == w, ("synchronous", n, pre, name)
        for a, b in ((0, 1), (2, 1), (0, 2)):   # two in flight, on one key or on two
            keys[vectors[a][1]].submit_device(0, dev[a], n, is_mont=True)
            keys[vectors[b][1]].submit_device(1, dev[b], n, is_mont=True)
            for slot, k in ((0, a), (1, b)):
                got = L.point_to_affine(c, keys[vectors[k][1]].wait(slot))
                assert got == tuple(want["%%d %%d" %% (n, k)]), ("in flight", n, pre, vectors[k][0])
        for key in keys:
            key.close()
print("child ok")
'''


@pytest.fixture(scope="module", params=[0, 1], ids=["pallas", "vesta"])
def reference(request, tmp_path_factory):
    c = request.param
    ns = {}
    exec(INPUTS, ns)
    want = {}
    for n in SIZES:
        B, B2, vectors = ns["inputs"](c, n)
        for k, (name, which, v) in enumerate(vectors):
            pt = C.jac_to_affine(c, C.msm_pippenger(c, B2 if which else B, v))
            if not which:  # the unmodified key: the discrete-log checksum as well
                assert pt == C.jac_to_affine(c, C.gen_mul(c, C.dot(1 - c, C.synth_base_scalars(c, n), v))), (n, name)
            assert pt != (0, 0), (n, name)
            want["%d %d" % (n, k)] = [int(pt[0]), int(pt[1])]
    path = str(tmp_path_factory.mktemp("msm_signed") / ("want_%d.json" % c))
    with open(path, "w") as f:
        json.dump(want, f)
    return c, path


@pytest.mark.parametrize("env", [{"LURK_MSM_PERSIST_S": "128"}, {"LURK_MSM_PERSIST_S": "64", "LURK_MSM_BUCKET_DIRECT": "0"}], ids=["tasks of 128", "tasks of 64, no direct form"])
def test_signed_accumulation_matches_the_oracle(hip, reference, env):
    c, want = reference
    e = dict(os.environ, LURK_MSM_ACC_PERSISTENT="2", **env)
    p = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r)\n" % ROOT + CHILD % dict(c=c, want=want, sizes=SIZES)], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "child ok" in p.stdout
