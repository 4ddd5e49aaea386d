"""Task sums and buckets as radix-2^29 records from the accumulation to the last reduction level (msm_stages.hpp: one record array
per slot), through the C ABI on an MI355X.

Keys of 2^16 + 64 points - the smallest that takes the bucket pipeline and not the small-commitment form - as a window table of 16-bit
windows (32 768 buckets: the DIRECT form in a synchronous call, the planned-task stages with LURK_MSM_BUCKET_DIRECT=0), a window table
of 20-bit windows (2^19 buckets, most of them empty or one entry: identity records and one-task stores) and a plain key (16 key spaces),
on Pallas, Vesta, BN254 G1 and Grumpkin.  Every commitment is compared as an affine point with a CPU reference: oracle.coracle's
Pippenger on the Pasta curves; on the BN254 cycle, which that oracle has no tables for, the discrete-log checksum over the synthetic
bases [k_i] G in Python integers (tests/bn254_ref.py: sum s_i [k_i] G == [sum s_i k_i] G, exact), as tests/test_gpu_bn254_msm.py does.

The scalars hit the new branches by construction.  A scalar below 2^15 has one non-zero digit, so the points that carry the scalar v
all land in bucket v - 1 of window 0:
  * buckets of exactly 1, S - 1, S, S + 1, 2 S, MSM_FIN_SMALL S and MSM_FIN_SMALL S + 1 entries (S = the task length of this shape, 8:
    the one-task store, the first two-task bucket, the last lane-summed bucket and the first listed one), and of 256 and 257 entries
    (the DIRECT form's own listing threshold at four lanes per bucket); every other bucket is empty, so identity records reach the
    reduction;
  * a bucket whose task sum is the identity: a repeated base under the scalars v and 2^c - v, which recode to the digits -v and +1;
  * a bucket of two equal points: the doubling branch inside a task whose sum is stored directly;
  * all scalars equal (one hot bucket per window), all zero (every bucket empty: the identity), uniform and witness-like scalars;
  * one pair of commitments split by an index bit (two key spaces).
Each case runs as a synchronous call, on two slots in flight and in the FOLLOW class; a fresh child process with
LURK_MSM_ACC_PERSISTENT=2 (the one-wave persistent pipelined kernel at this size) repeats them with LURK_MSM_BUCKET_DIRECT=0 and 1 and
must print the same points.  One more child keeps the tasks at the full lengths of a large commitment - 64 entries, and 128 for the
persistent form on the accumulate stream - with the boundary counts built for both."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = (1 << 16) + 64
MSM_S, MSM_S_MIN, MSM_TASK_TARGET, MSM_FIN_SMALL = 64, 8, 131072, 16   # msm_sort.hpp, msm_stages.hpp
KINDS = {"table16": (True, 16), "table20": (True, 20), "plain": (False, 16)}   # precompute, window bits
CURVE_NAMES = {0: "pallas", 1: "vesta", 2: "bn254", 3: "grumpkin"}
DUP_TWICE, DUP_CANCEL = (0, 1), (2, 3)   # base 1 = base 0 (the doubling), base 3 = base 2 (the sum that cancels)


def task_len(c, n):
    """msm_make_shape's task length for n scalars under c-bit windows"""
    w, s = (256 + c - 1) // c, MSM_S
    while s > MSM_S_MIN and w * n // s < MSM_TASK_TARGET:
        s //= 2
    return s


def u64x4(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


class Curve:
    """bases (host, with the two repeated points), the reference and the affine form of a result, for one curve id"""

    def __init__(self, cid):
        self.cid = cid
        self.wants = {}
        if cid < 2:
            from oracle import coracle as C

            self.sf = 1 if cid == 0 else 0
            self.bases = C.synth_bases(cid, N).copy()
        else:
            from lurk_beta_amd import synth
            from tests import bn254_ref as B

            self.bn = B.CURVES[cid]
            self.sf = self.bn.scalar_field
            self.bases = synth.bases(cid, N).cpu().numpy().view(np.uint64).copy()
            self.k = B.base_scalars_np(self.bn, N)
        for a, b in (DUP_TWICE, DUP_CANCEL):
            self.bases[b] = self.bases[a]
            if cid >= 2:
                self.k[b] = self.k[a]
        if cid >= 2:
            self.k12 = B.limbs12(self.k)

    def synth(self, stream, dist):
        if self.cid < 2:
            from oracle import coracle as C

            return C.synth_scalars(self.sf, stream, dist, N)
        from lurk_beta_amd import synth

        return synth.scalars(self.sf, stream, dist, N).cpu().numpy().view(np.uint64).copy()

    def want(self, name, scalars):
        """the reference's affine point, computed once per scalar vector and shared by every key kind and path"""
        if name not in self.wants:
            if self.cid < 2:
                from oracle import coracle as C

                self.wants[name] = tuple(C.jac_to_affine(self.cid, C.msm_fast(self.cid, self.bases, scalars)))
            else:
                from tests import bn254_ref as B

                P = self.bn.mul(B.dot_mod(B.limbs12(scalars), self.k12, self.bn.order), self.bn.gen)
                self.wants[name] = (0, 0) if P is None else tuple(P)
        return self.wants[name]

    def affine(self, jac):
        from lurk_beta_amd import point_to_affine

        return tuple(point_to_affine(self.cid, jac))


_curves = {}


def curve(cid):
    if cid not in _curves:
        _curves[cid] = Curve(cid)
    return _curves[cid]


def scalar_cases(cv, c, lens=None):
    """name -> (N, 4) u64 canonical scalars; the names carry what the vector depends on (the window width, the task lengths)"""
    lens = lens or (task_len(c, N),)
    sparse = [0] * N
    pos = 16
    counts = [1, 256, 257]
    for S in lens:
        counts += [S - 1, S, S + 1, 2 * S, MSM_FIN_SMALL * S, MSM_FIN_SMALL * S + 1]
    counts = sorted(set(counts))
    for i, cnt in enumerate(counts):            # cnt points carry the scalar 1000 + i: bucket 999 + i of window 0 holds exactly cnt entries
        for _ in range(cnt):
            sparse[pos] = 1000 + i
            pos += 1
    assert pos < N
    sparse[DUP_TWICE[0]] = sparse[DUP_TWICE[1]] = 77            # P + P inside one task of two entries
    sparse[DUP_CANCEL[0]], sparse[DUP_CANCEL[1]] = 55, (1 << c) - 55   # digits +55 and (-55, +1): bucket 54 sums to the identity
    uniform = cv.synth(31, 0)
    return {
        "boundary buckets, c=%d, S=%s" % (c, lens): u64x4(sparse),
        "all equal": np.tile(uniform[5], (N, 1)),
        "all zero": np.zeros((N, 4), dtype=np.uint64),
        "uniform": uniform,
        "witness-like": cv.synth(32, 1),
    }


def run_kind(cid, kind, pair=True, lens=None):
    """every case of one key kind through the three paths (and one pair); returns the affine points in a fixed order.  lens: the task
    lengths the boundary counts are built for (default: the one msm_make_shape gives this shape)"""
    import torch

    import lurk_beta_amd as L

    cv = curve(cid)
    pre, c = KINDS[kind]
    key = L.CommitmentKey(cid, cv.bases, precompute=pre, window_bits=c if pre else 0, small_form=False if pre else None)
    info = key.info()
    assert info["form"] == ("table" if pre else "plain") and info["window_bits"] == c, info
    outs = []
    for name, S in scalar_cases(cv, c, lens).items():
        want = cv.want(name, S)
        if name == "all zero":
            assert want == (0, 0)
        d_s = torch.from_numpy(S.view(np.int64)).cuda()
        got = {"sync": [cv.affine(key.commit_device(d_s, N))]}
        key.submit_device(0, d_s, N)                       # two slots in flight
        key.submit_device(1, d_s, N)
        got["in flight"] = [cv.affine(key.wait(0)), cv.affine(key.wait(1))]
        key.submit_device(2, d_s, N, mode=1)               # a foreground commitment and one that follows it
        key.submit_device(3, d_s, N, mode=3)
        got["follow"] = [cv.affine(key.wait(2)), cv.affine(key.wait(3))]
        for path, pts in got.items():
            for p in pts:
                print(CURVE_NAMES[cid], kind, name, path, "%x" % p[0])
                assert p == want, (CURVE_NAMES[cid], kind, name, path)
                outs.append(p)
    if pair and pre:
        name, S = "uniform", scalar_cases(cv, c, lens)["uniform"]
        bit = 9
        m = ((np.arange(N) >> bit) & 1).astype(bool)
        lo_s, hi_s = S.copy(), S.copy()
        lo_s[m] = 0
        hi_s[~m] = 0
        d_s = torch.from_numpy(S.view(np.int64)).cuda()
        key.submit_pair_device(0, d_s, N, bit)
        lo, hi = key.wait_pair(0)
        assert cv.affine(lo) == cv.want("uniform, bit %d clear" % bit, lo_s), (CURVE_NAMES[cid], kind, "pair lo")
        assert cv.affine(hi) == cv.want("uniform, bit %d set" % bit, hi_s), (CURVE_NAMES[cid], kind, "pair hi")
        outs += [cv.affine(lo), cv.affine(hi)]
    key.close()
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cid", list(CURVE_NAMES))
def test_commitments_through_bucket_records_match_the_reference(hip, cid, kind):
    assert task_len(KINDS[kind][1], N) == MSM_S_MIN   # (what the boundary counts in the docstring are worked out for)
    assert len(run_kind(cid, kind)) > 0


CHILD = r'''
import sys
sys.path.insert(0, %r)
from tests import test_gpu_msm_bucket_records as T
cid = int(sys.argv[1])
lens = tuple(int(x) for x in sys.argv[2].split(",")) if len(sys.argv) > 2 else None
for kind in T.KINDS:
    for p in T.run_kind(cid, kind, lens=lens):
        print("point", kind, "%%x %%x" %% p)
print("child ok")
'''


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CURVE_NAMES))
def test_persistent_pipelined_kernel_stores_the_same_records_with_and_without_the_direct_form(hip, cid):
    """LURK_MSM_ACC_PERSISTENT=2 is read once per process, so a fresh child: the commitments in flight then take the one-wave persistent
    pipelined kernel at this size (and never the DIRECT form); its synchronous and FOLLOW commitments take the DIRECT form or, with
    LURK_MSM_BUCKET_DIRECT=0, the planned-task stages.  Both children check every point against the reference and must print the same."""
    points = []
    for direct in ("0", "1"):
        e = dict(os.environ)
        e["LURK_MSM_ACC_PERSISTENT"] = "2"
        e["LURK_MSM_BUCKET_DIRECT"] = direct
        p = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(cid)], env=e, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
        assert "child ok" in p.stdout
        points.append([ln for ln in p.stdout.splitlines() if ln.startswith("point")])
    assert points[0] and points[0] == points[1]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CURVE_NAMES))
def test_full_length_tasks_of_both_forms(hip, cid):
    """The task lengths of large commitments at this size: LURK_MSM_TASK_TARGET=1 keeps msm_make_shape from shortening the tasks, so
    the synchronous, foreground and FOLLOW commitments cut their buckets into 64-entry tasks and - with LURK_MSM_ACC_PERSISTENT=2 - the
    commitments in flight take the one-wave persistent form with its 128-entry tasks (msm_launch_plan.hpp: persist_s).  The boundary
    buckets hold S - 1, S, S + 1, 2 S, MSM_FIN_SMALL S and MSM_FIN_SMALL S + 1 entries for both lengths; every point is checked
    against the reference inside the child."""
    e = dict(os.environ)
    e.update(LURK_MSM_ACC_PERSISTENT="2", LURK_MSM_TASK_TARGET="1", LURK_MSM_BUCKET_DIRECT="0")
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT, str(cid), "64,128"], env=e, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-2500:])
    assert "child ok" in p.stdout and any(ln.startswith("point") for ln in p.stdout.splitlines())
