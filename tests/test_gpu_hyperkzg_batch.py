"""GPU: lurk_hip_hyperkzg_prove_dev with its short stage-0 commitments as ONE batch (LURK_HYPERKZG_BATCH=1: lurk_hip_msm_ctx_submit_batch_dev)
and each as a submit of its own (0), in one process: the switch is read at each call.  The two proofs are the same bytes, both satisfy the
trapdoor identity L == [tau] R, and a failing transcript callback leaves the key committing."""
import ctypes
import os

import numpy as np
import pytest

from tests import bn254_ref as BN
from tests import hyperkzg_ref as HK
from tests.test_gpu_hyperkzg import TAU, DeviceTranscript, affine, dev, random_instance

pytestmark = pytest.mark.gpu

SWITCH, CAP = "LURK_HYPERKZG_BATCH", "LURK_HYPERKZG_BATCH_MAX_LEN"
_keys = {}


def table_key(n):
    from lurk_beta_amd import hyperkzg

    if n not in _keys:
        _keys[n] = hyperkzg.trapdoor_key(TAU, n, precompute=True, window_bits=20)
        assert _keys[n].info()["form"] == "table"
    return _keys[n]


class Env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def batches_launched(lib, fn):
    """fn() under the library's profiler: (result, batch passes enqueued meanwhile)"""
    assert lib.lurk_hip_profile_enable(1) == 0 and lib.lurk_hip_profile_reset() == 0
    try:
        out = fn()
        ms, launches = ctypes.c_double(), ctypes.c_uint64()
        assert lib.lurk_hip_profile_get(b"msm_batch_sort", ctypes.byref(ms), ctypes.byref(launches)) == 0
    finally:
        lib.lurk_hip_profile_enable(0)
    return out, launches.value


def prove(ck, d_p, x):
    from lurk_beta_amd import hyperkzg

    tr = DeviceTranscript()
    pf = hyperkzg.prove(ck, d_p, x, tr)
    return pf, tr


def same_bytes(a, b):
    return np.array_equal(a["com"], b["com"]) and np.array_equal(a["w"], b["w"]) and (a["v"], a["y"]) == (b["v"], b["y"])


def check_identity(ck, p0, x, pf, tr):
    from lurk_beta_amd import hyperkzg

    ell = len(x)
    d = tr.tr(2, [affine(j) for j in pf["w"]])
    c = BN.jacobian(BN.BN254, HK.commit_trapdoor(TAU, p0))
    L, R, ok, code = hyperkzg.pairing_inputs(ell, c, x, pf["y"], pf["com"], pf["v"], pf["w"], tr.out[0], tr.out[1], d)
    assert ok and code == 0
    assert HK.trapdoor_holds(TAU, affine(L), affine(R))


# ell = 1: no commitment; 2: one (below the two-vector threshold: a submit of its own); 3: two; 10: nine
@pytest.mark.parametrize("ell,want_batches", [(1, 0), (2, 0), (3, 1), (10, 1)])
def test_batched_and_unbatched_proofs_are_the_same_bytes(hip, ell, want_batches):
    ck = table_key(1 << 10)
    p0, x = random_instance(ell, seed=7)
    d_p = dev(HK.Q, p0)
    with Env(**{SWITCH: 0, CAP: None}):
        (pf0, tr0), n0 = batches_launched(hip, lambda: prove(ck, d_p, x))
    with Env(**{SWITCH: 1, CAP: None}):
        (pf1, tr1), n1 = batches_launched(hip, lambda: prove(ck, d_p, x))
    assert (n0, n1) == (0, want_batches)
    assert same_bytes(pf0, pf1) and tr0.out == tr1.out
    assert pf1["com"].shape == (ell - 1, 12)
    check_identity(ck, p0, x, pf1, tr1)
    ref = HK.prove(TAU, p0, x, HK.Transcript())
    assert [affine(j) for j in pf1["com"]] == ref["com"] and pf1["y"] == ref["y"]


def test_some_long_some_batched(hip):
    """with the length threshold lowered to 64, a 2^10 opening commits P_1 .. P_3 (512, 256, 128) on slots of their own and P_4 .. P_9 as one
    batch - the shape of a 2^20 opening; at 1 the threshold leaves one short polynomial: no batch"""
    ell = 10
    ck = table_key(1 << ell)
    p0, x = random_instance(ell, seed=8)
    d_p = dev(HK.Q, p0)
    with Env(**{SWITCH: 0, CAP: None}):
        pf0, tr0 = prove(ck, d_p, x)
    with Env(**{SWITCH: 1, CAP: 64}):
        (pf1, tr1), n1 = batches_launched(hip, lambda: prove(ck, d_p, x))
    with Env(**{SWITCH: 1, CAP: 1}):
        (pf2, tr2), n2 = batches_launched(hip, lambda: prove(ck, d_p, x))
    assert (n1, n2) == (1, 0)
    assert same_bytes(pf0, pf1) and same_bytes(pf0, pf2)
    check_identity(ck, p0, x, pf1, tr1)


def test_a_failing_callback_leaves_the_key_committing(hip):
    from lurk_beta_amd import LurkHipError, hyperkzg

    ell = 10
    ck = table_key(1 << ell)
    p0, x = random_instance(ell, seed=9)
    d_p = dev(HK.Q, p0)
    want = HK.commit_trapdoor(TAU, p0)
    with Env(**{SWITCH: 1, CAP: 64}):
        with pytest.raises(LurkHipError, match="callback failed"):
            hyperkzg.prove(ck, d_p, x, lambda stage, data: None if stage == 0 else 5)
        assert affine(ck.commit_device(d_p, 1 << ell, is_mont=True)) == want
        for slot in range(6):  # every slot is free again: the batch slot too
            ck.submit_device(slot, d_p, 64, is_mont=True)
        for slot in range(6):
            ck.wait(slot)
        pf, tr = prove(ck, d_p, x)
        check_identity(ck, p0, x, pf, tr)


def test_a_plain_key_proves_through_the_fallback(hip):
    from lurk_beta_amd import hyperkzg

    ell = 5
    plain = hyperkzg.trapdoor_key(TAU, 1 << ell)
    assert plain.info()["form"] == "plain"
    p0, x = random_instance(ell, seed=10)
    d_p = dev(HK.Q, p0)
    with Env(**{SWITCH: 1, CAP: None}):
        (pf1, tr1), n1 = batches_launched(hip, lambda: prove(plain, d_p, x))
    with Env(**{SWITCH: 0, CAP: None}):
        pf0, _ = prove(plain, d_p, x)
    assert n1 == 0 and same_bytes(pf0, pf1)
    check_identity(plain, p0, x, pf1, tr1)
    plain.close()
