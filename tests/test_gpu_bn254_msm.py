"""The Pedersen MSM over the BN254 / Grumpkin cycle, through the C ABI, against tests/bn254_ref.py (Python integers; nothing of
oracle/'s curve tables).  Needs an MI355X.

Anchors: the naive Python sum for small commitments and edge lists, and - at full sizes - the discrete-log checksum
sum s_i [k_i]G == [sum s_i k_i mod order] G over lurk_hip_synth_bases_dev's bases (ONE Python scalar multiple)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bn254_ref as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE_IDS = [B.CURVE_BN254, B.CURVE_GRUMPKIN]
MAX_LOG = 22
_dev = {}


def dev_bases(cid, n):
    """the first n synthetic bases of the curve in HBM (one 2^22-point tensor per curve, generated once)"""
    from lurk_beta_amd import synth

    if cid not in _dev:
        _dev[cid] = synth.bases(cid, 1 << MAX_LOG)
    return _dev[cid][:n]


def host_bases(cid, n):
    return dev_bases(cid, n).cpu().numpy().view(np.uint64)


def dev_scalars(cid, stream, dist, n, mont=False):
    from lurk_beta_amd import synth

    return synth.scalars(B.CURVES[cid].scalar_field, stream, dist, n, mont=mont)


def affine(cid, jac):
    from lurk_beta_amd import point_to_affine

    return B.from_xy(point_to_affine(cid, jac))


def test_synth_generators_match_the_python_rules(hip):
    for cid in CURVE_IDS:
        c = B.CURVES[cid]
        for dist in (0, 1):
            got = dev_scalars(cid, 5, dist, 600).cpu().numpy().view(np.uint64)
            assert B.limbs_to_ints(got) == c.synth_scalars(5, dist, 600), (c.name, dist)
        gm = dev_scalars(cid, 5, 0, 50, mont=True).cpu().numpy().view(np.uint64)
        assert B.from_mont(c.order, gm) == c.synth_scalars(5, 0, 50)
        got = host_bases(cid, 40)
        assert np.array_equal(got, B.affine_bases(c, c.synth_bases(40))), c.name


@pytest.mark.parametrize("cid", CURVE_IDS)
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255])
def test_small_commitments_match_the_naive_sum(hip, cid, n):
    from lurk_beta_amd import msm

    c = B.CURVES[cid]
    pts = c.synth_bases(n)
    bases = B.affine_bases(c, pts)
    for dist in (0, 1):
        s = c.synth_scalars(1, dist, n)
        want = c.msm(s, pts)
        assert affine(cid, msm(cid, bases, B.ints_to_limbs(s), is_mont=False)) == want, dist
        assert affine(cid, msm(cid, bases, B.to_mont(c.order, s), is_mont=True)) == want, dist


@pytest.mark.parametrize("cid", CURVE_IDS)
def test_edge_list(hip, cid):
    from lurk_beta_amd import CommitmentKey, msm

    c, q, n = B.CURVES[cid], B.CURVES[cid].order, 64
    pts = c.synth_bases(n)

    def both(points, scalars):
        """the one-shot path and a window-table key must both give the naive sum"""
        bases, S = B.affine_bases(c, points), B.ints_to_limbs(scalars)
        want = c.msm(scalars, points)
        assert affine(cid, msm(cid, bases, S)) == want
        ck = CommitmentKey(cid, bases, precompute=True, small_form=False)
        assert affine(cid, ck.commit(S)) == want
        ck.close()
        return want

    s = c.synth_scalars(9, 0, n)
    out = msm(cid, B.affine_bases(c, pts), np.zeros((n, 4), dtype=np.uint64))  # all-zero scalars
    assert affine(cid, out) is None and not out[8:].any()
    assert both(pts, [0] * n) is None
    both(pts, [1, q - 1] * (n // 2))                                         # scalars 1 and order - 1
    both([None if i % 3 == 0 else P for i, P in enumerate(pts)], s)         # identity bases
    both([pts[0], c.neg(pts[0])] + pts[2:], [777, 777] + s[2:])             # P beside -P: the identity mid-chain
    both([pts[4], pts[4]] + pts[2:], [777, q - 777] + s[2:])                # the same through the recoding's sign
    both([pts[7]] * n, [12345] * n)                                          # one base repeated with equal scalars: the doubling branch
    both(pts, [0] * (n - 1) + [s[5]])                                        # one non-zero scalar at the last position
    both(pts, [0x8000, 0x8001, (1 << 253) | 0xFFFF, int("ffff" * 15, 16) % q, q - 1, q - 2] + s[6:])  # recoding edges of 254-bit scalars
    assert affine(cid, msm(cid, np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))) is None


SIZES = [1 << 12, 1 << 16, (1 << 16) + 1, 1 << 20, 1 << 22]


@pytest.mark.parametrize("cid", CURVE_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_dlog_checksum_plain_and_table_keys_every_window_width(hip, cid, n):
    """plain key and table key at every window width 16..20 (and the key's own choice); at n <= 2^16 also the small form, forced by
    its flag - the plain key there runs the bucket-direct path - all against one checksum and so against each other"""
    from lurk_beta_amd import CommitmentKey

    c = B.CURVES[cid]
    bases = dev_bases(cid, n)
    sd = dev_scalars(cid, 3, 1, n)                       # witness-like: hot buckets, zeros, small values
    want = B.dlog_checksum_np(c, sd.cpu().numpy().view(np.uint64))
    assert want is not None
    sm = dev_scalars(cid, 3, 1, n, mont=True)
    plain = CommitmentKey(cid, bases, n=n, device=True)
    assert plain.info() == {"curve": cid, "npoints": n, "window_bits": 16, "precomputed": False, "form": "plain"}
    assert affine(cid, plain.commit_device(sd, n)) == want, "plain"
    assert affine(cid, plain.commit_device(sm, n, is_mont=True)) == want, "plain, Montgomery scalars"
    plain.close()
    for w in (0, 16, 17, 18, 19, 20):
        ck = CommitmentKey(cid, bases, n=n, device=True, precompute=True, window_bits=w, small_form=False if w == 0 else None)
        info = ck.info()
        assert info["form"] == "table" and (info["window_bits"] == w or w == 0), info
        assert affine(cid, ck.commit_device(sm, n, is_mont=True)) == want, ("table", w)
        ck.close()
    if n <= 1 << 16:
        ck = CommitmentKey(cid, bases, n=n, device=True, precompute=True, small_form=True)
        assert ck.info()["form"] == "small"
        assert affine(cid, ck.commit_device(sd, n)) == want, "small form"
        assert affine(cid, ck.commit_device(sm, n, is_mont=True)) == want, "small form, Montgomery scalars"
        ck.close()


@pytest.mark.parametrize("cid", CURVE_IDS)
def test_uniform_scalars_and_prefixes(hip, cid):
    """uniform scalars at the sizes around the small / bucket-direct threshold; a commitment to a prefix uses ck[..len]"""
    from lurk_beta_amd import CommitmentKey

    c = B.CURVES[cid]
    n = (1 << 16) + 1
    ck, ckt = CommitmentKey(cid, dev_bases(cid, n), n=n, device=True), CommitmentKey(cid, dev_bases(cid, n), n=n, device=True, precompute=True)
    sd = dev_scalars(cid, 4, 0, n)
    host = sd.cpu().numpy().view(np.uint64)
    for m in (n, 1 << 16, 1 << 12, 1000, 1):
        want = B.dlog_checksum_np(c, host[:m])
        assert affine(cid, ck.commit_device(sd, m)) == want, m
        assert affine(cid, ckt.commit_device(sd, m)) == want, ("table", m)
        assert affine(cid, ck.commit(host[:m])) == want, ("host scalars", m)
    ck.close()
    ckt.close()


_SWITCH_CHILD = r'''
import sys
import numpy as np
from lurk_beta_amd import CommitmentKey, point_to_affine, synth
from tests import bn254_ref as B
for cid in (2, 3):
    f = B.CURVES[cid].scalar_field
    for n in (1 << 12, 1 << 16, (1 << 16) + 1):
        bases = synth.bases(cid, n)
        s = synth.scalars(f, 3, 1, n)
        for pre, w in ((False, 0), (True, 16), (True, 19)):
            ck = CommitmentKey(cid, bases, n=n, device=True, precompute=pre, window_bits=w, small_form=False if pre else None)
            print(cid, n, int(pre), w, *point_to_affine(cid, ck.commit_device(s, n)))
            ck.close()
'''


def test_switches_off_and_on_give_the_same_points(hip):
    """LURK_MSM_BUCKET_DIRECT=0 (the planned-task stages where the direct path would run), LURK_MSM_REDUCE_QUAD / _WAVE off: the
    switches are read once per process, so each setting is a child; every setting must print the checksum points"""
    want = []
    for cid in CURVE_IDS:
        c = B.CURVES[cid]
        for n in (1 << 12, 1 << 16, (1 << 16) + 1):
            pt = B.dlog_checksum_np(c, dev_scalars(cid, 3, 1, n).cpu().numpy().view(np.uint64))
            want += [f"{cid} {n} {pre} {w} {pt[0]} {pt[1]}" for pre, w in ((0, 0), (1, 16), (1, 19))]
    for env in ({}, {"LURK_MSM_BUCKET_DIRECT": "0"}, {"LURK_MSM_REDUCE_QUAD": "0"}, {"LURK_MSM_REDUCE_QUAD": "0", "LURK_MSM_REDUCE_WAVE": "0"}):
        r = subprocess.run([sys.executable, "-c", _SWITCH_CHILD], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (env, r.stderr[-800:])
        assert r.stdout.split("\n")[:len(want)] == want, env


@pytest.mark.parametrize("cid", CURVE_IDS)
def test_commitments_in_flight_and_the_pair_call(hip, cid):
    import torch

    from lurk_beta_amd import CommitmentKey

    c = B.CURVES[cid]
    n = 1 << 17
    ckt = CommitmentKey(cid, dev_bases(cid, n), n=n, device=True, precompute=True)
    ckp = CommitmentKey(cid, dev_bases(cid, n), n=n, device=True)
    vecs = [dev_scalars(cid, 10 + k, k & 1, n, mont=True) for k in range(4)]
    torch.cuda.synchronize()
    for ck in (ckt, ckp):
        ck.reserve(n, 4)
        sync = [ck.commit_device(v, n, is_mont=True) for v in vecs]
        for k in range(4):  # the four scheduling classes, all in flight at once
            ck.submit_device(k, vecs[k], n, is_mont=True, mode=k)
        for k in (2, 0, 3, 1):
            assert np.array_equal(ck.wait(k), sync[k]), k
    host0 = np.array(B.ints_to_limbs(B.from_mont(c.order, vecs[0].cpu().numpy().view(np.uint64))))
    assert affine(cid, sync[0]) == B.dlog_checksum_np(c, host0)
    # the pair: indices with bit 16 clear / set, one pass
    assert ckt.supports_pairs() and not ckp.supports_pairs()
    ckt.submit_pair_device(1, vecs[0], n, 16, is_mont=True)
    lo, hi = ckt.wait_pair(1)
    assert np.array_equal(lo, ckt.commit_device(vecs[0], 1 << 16, is_mont=True))
    masked = vecs[0].clone()
    masked[:1 << 16] = 0
    assert np.array_equal(hi, ckt.commit_device(masked, n, is_mont=True))
    from lurk_beta_amd import point_sum

    assert np.array_equal(point_sum(cid, np.stack([lo, hi])), sync[0])
    # rebinding a plain key to other bases (the key's second half), workspaces kept
    from lurk_beta_amd import _lib

    half = dev_bases(cid, n)[1 << 16:]
    _lib.check(hip.lurk_hip_msm_ctx_rebind_dev(ckp._ctx, _lib.ptr(half), 1 << 16))
    sd = dev_scalars(cid, 3, 0, 1 << 16)
    assert affine(cid, ckp.commit_device(sd, 1 << 16)) == B.dlog_checksum_np(c, sd.cpu().numpy().view(np.uint64), first=1 << 16)
    dev = ctypes.c_int(-1)
    _lib.check(hip.lurk_hip_msm_ctx_device(ckp._ctx, ctypes.byref(dev)))
    assert dev.value == 0
    ckt.close()
    ckp.close()


@pytest.mark.parametrize("cid", CURVE_IDS)
def test_one_shot_symbols_equal_the_context_path(hip, cid):
    from lurk_beta_amd import CommitmentKey, _lib, msm

    name = {B.CURVE_BN254: "bn254", B.CURVE_GRUMPKIN: "grumpkin"}[cid]
    c = B.CURVES[cid]
    for n in (300, 1 << 14):
        bases = np.ascontiguousarray(host_bases(cid, n))
        sm = np.ascontiguousarray(dev_scalars(cid, 6, 1, n, mont=True).cpu().numpy().view(np.uint64))
        ck = CommitmentKey(cid, bases)
        want = ck.commit(sm, is_mont=True)
        ck.close()
        assert affine(cid, want) == B.dlog_checksum_np(c, B.ints_to_limbs(B.from_mont(c.order, sm)))
        assert np.array_equal(msm(cid, bases, sm, is_mont=True), want)
        out = np.zeros(12, dtype=np.uint64)
        getattr(hip, "mult_pippenger_" + name)(_lib.ptr(out), _lib.ptr(bases), n, _lib.ptr(sm), True)
        assert np.array_equal(out, want)
        out[:] = 0
        err = getattr(hip, "cuda_pippenger_" + name)(_lib.ptr(out), _lib.ptr(bases), n, _lib.ptr(sm), True)
        assert err.code == 0 and not err.message and np.array_equal(out, want)


def test_key_file_round_trip_records_the_curve(hip, tmp_path):
    from lurk_beta_amd import CommitmentKey, LurkHipError

    n = 3000
    for cid in CURVE_IDS:
        c = B.CURVES[cid]
        sd = dev_scalars(cid, 8, 0, n)
        want = B.dlog_checksum_np(c, sd.cpu().numpy().view(np.uint64))
        ck = CommitmentKey(cid, dev_bases(cid, n), n=n, device=True, precompute=True, window_bits=17)
        plain, table = str(tmp_path / f"k{cid}.plain"), str(tmp_path / f"k{cid}.table")
        ck.save(plain)
        ck.save(table, with_table=True)
        ck.close()
        for path, kw in ((plain, {}), (plain, {"precompute": True}), (table, {"precompute": True}), (table, {})):
            k2 = CommitmentKey.load(path, curve=cid, **kw)
            assert k2.curve == cid and k2.n == n
            assert affine(cid, k2.commit_device(sd, n)) == want, (path, kw)
            k2.close()
        assert CommitmentKey.load(table, precompute=True).info()["window_bits"] == 17
    bn = str(tmp_path / f"k{B.CURVE_BN254}.plain")
    for other, name in ((B.CURVE_GRUMPKIN, "Grumpkin"), (0, "Pallas")):
        with pytest.raises(LurkHipError, match=f"BN254.*{name}"):
            CommitmentKey.load(bn, curve=other)
    assert CommitmentKey.load(bn, curve=B.CURVE_BN254).n == n  # a following valid call works


@pytest.mark.parametrize("cid", CURVE_IDS)
def test_point_helpers_against_python(hip, cid):
    from lurk_beta_amd import point_mul, point_sum, point_to_affine
    from lurk_beta_amd.msm import point_sum_gathered

    c = B.CURVES[cid]
    G = c.gen
    pts = [c.mul(k, G) for k in (5, 7, c.order - 12)] + [None]
    jac = np.stack([B.jacobian(c, P) for P in pts])
    assert affine(cid, point_sum(cid, jac)) is None                      # 5 + 7 - 12
    assert affine(cid, point_sum(cid, jac[:2])) == c.mul(12, G)
    assert affine(cid, point_sum(cid, np.stack([jac[0], jac[0]]))) == c.mul(10, G)
    assert affine(cid, point_sum_gathered(cid, jac[:3])) is None
    assert point_to_affine(cid, jac[3]) == (0, 0) and point_to_affine(cid, jac[1]) == pts[1]
    for k in (0, 1, 2, c.order - 1, 0x1234567890ABCDEF1234567890ABCDEF, c.synth_scalars(2, 0, 1)[0]):
        assert affine(cid, point_mul(cid, jac[1], B.ints_to_limbs([k]), is_mont=False)) == c.mul(7 * k, G), k
        assert affine(cid, point_mul(cid, jac[1], B.to_mont(c.order, [k]), is_mont=True)) == c.mul(7 * k, G), k
    # a non-normalised Jacobian point (Z != 1) goes through the inversion
    z = 0xABCDEF
    P = pts[0]
    j = B.to_mont(c.p, [P[0] * z * z % c.p, P[1] * z * z * z % c.p, z]).reshape(12)
    assert point_to_affine(cid, j) == P


@pytest.mark.parametrize("cid", CURVE_IDS)
def test_device_list_commits_to_the_single_device_point(hip, cid):
    from lurk_beta_amd import MultiCommitmentKey

    c = B.CURVES[cid]
    n = 5001
    bases = host_bases(cid, n)
    s = dev_scalars(cid, 12, 1, n).cpu().numpy().view(np.uint64)
    want = B.dlog_checksum_np(c, s)
    for pre in (False, True):
        mk = MultiCommitmentKey(cid, bases, [0, 0], precompute=pre)
        assert [x[1:] for x in mk.shards()] == [(0, 2501), (2501, 2500)]
        assert affine(cid, mk.commit(s)) == want
        assert affine(cid, mk.commit(s[:2600])) == B.dlog_checksum_np(c, s[:2600])
        mk.close()


def test_out_of_scope_calls_refuse_the_new_curves_by_name(hip):
    import torch

    from lurk_beta_amd import CommitmentKey, LurkHipError, R1CSShape, _lib

    for cid in CURVE_IDS:
        name = B.CURVES[cid].name
        n = 1 << 10
        key = CommitmentKey(cid, dev_bases(cid, n), n=n, device=True, precompute=True, window_bits=16)
        buf = torch.zeros((n, 8), dtype=torch.int64, device="cuda")
        z32, z96, z64 = np.zeros(4, dtype=np.uint64), np.zeros(12, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        h = ctypes.c_void_p()
        calls = {
            "lurk_hip_msm_ctx_from_label": lambda: hip.lurk_hip_msm_ctx_from_label(ctypes.byref(h), cid, b"ck", 2, 16, 0),
            "lurk_hip_ck_from_label_host": lambda: hip.lurk_hip_ck_from_label_host(cid, b"ck", 2, 1, _lib.ptr(z64)),
            "lurk_hip_ck_from_label_dev": lambda: hip.lurk_hip_ck_from_label_dev(cid, b"ck", 2, 16, _lib.ptr(buf), None),
            "lurk_hip_ck_hash_to_curve_dev": lambda: hip.lurk_hip_ck_hash_to_curve_dev(cid, b"p", _lib.ptr(buf), 4, _lib.ptr(buf), None),
            "lurk_hip_msm_ctx_fold_key_dev": lambda: hip.lurk_hip_msm_ctx_fold_key_dev(key._ctx, n, _lib.ptr(np.zeros(8, dtype=np.uint64)), 2, _lib.ptr(buf), None),
            "lurk_hip_points_fold_halves_dev": lambda: hip.lurk_hip_points_fold_halves_dev(cid, _lib.ptr(buf), 8, _lib.ptr(z32), _lib.ptr(z32), _lib.ptr(buf), None),
            "lurk_hip_nifs_challenge": lambda: hip.lurk_hip_nifs_challenge(cid, _lib.ptr(z32), _lib.ptr(z96), _lib.ptr(z96), _lib.ptr(z32), None, _lib.ptr(z96), None, 0,
                                                                        _lib.ptr(z96), _lib.ptr(z32)),
        }
        for fn, call in calls.items():
            rc = call()
            assert rc != 0 and name in hip.lurk_hip_last_error().decode(), (fn, name, hip.lurk_hip_last_error())
        # the opening argument takes the curve from the key (refused before the callback is ever used)
        cb = _lib.IPA_CHALLENGE_FN(lambda *a: 1)
        va, vb = torch.zeros((n, 4), dtype=torch.int64, device="cuda"), torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        ls = np.zeros((10, 12), dtype=np.uint64)
        rc = hip.lurk_hip_ipa_prove_dev(key._ctx, _lib.ptr(va), _lib.ptr(vb), n, _lib.ptr(z96), ctypes.cast(cb, ctypes.c_void_p), None, _lib.ptr(ls),
                                        _lib.ptr(ls.copy()), _lib.ptr(z32), _lib.ptr(z64), None)
        assert rc != 0 and name in hip.lurk_hip_last_error().decode(), hip.lurk_hip_last_error()
        # the compressing SNARK's provers and every verifier: the curve comes from the key as well.  Arguments that pass every check
        # in front of it: a shape over the BN254 scalar field, sizes 2 / 2 / 0, non-null buffers
        ident = B.to_mont(B.BN254_R, [1, 1])
        sh = R1CSShape(B.FIELD_BN254_FR, 2, 2, 0, *[([0, 1, 2], [0, 1], ident)] * 3)
        scratch = np.zeros(4096, dtype=np.uint64)
        sp = _lib.SpartanProofStruct(*[scratch.ctypes.data] * 10)
        bp = _lib.SpartanBatchProofStruct(*[scratch.ctypes.data] * 10)
        inst = _lib.SpartanInstanceStruct(sh._h, sh._h, 2, 2, 0, None, _lib.ptr(z32), _lib.ptr(va), _lib.ptr(vb), _lib.ptr(z96), _lib.ptr(z96))
        acc, why = ctypes.c_int(7), ctypes.c_int(7)
        more = {
            "lurk_hip_spartan_prove_dev": lambda: hip.lurk_hip_spartan_prove_dev(sh._h, sh._h, 2, 2, 0, key._ctx, _lib.ptr(z96), None, _lib.ptr(z32), _lib.ptr(va),
                                                                              _lib.ptr(vb), _lib.ptr(z96), _lib.ptr(z96), b"l", 1, ctypes.byref(sp), None),
            "lurk_hip_spartan_prove_batch_dev": lambda: hip.lurk_hip_spartan_prove_batch_dev(ctypes.byref(inst), 1, key._ctx, _lib.ptr(z96), b"l", 1, ctypes.byref(bp), None),
            "lurk_hip_ipa_verify_dev": lambda: hip.lurk_hip_ipa_verify_dev(key._ctx, 2, _lib.ptr(z96), _lib.ptr(z96), _lib.ptr(va), None, _lib.ptr(ls), _lib.ptr(ls),
                                                                        _lib.ptr(z32), ctypes.cast(cb, ctypes.c_void_p), None, ctypes.byref(acc), ctypes.byref(why), None),
            "lurk_hip_spartan_verify_dev": lambda: hip.lurk_hip_spartan_verify_dev(sh._h, 2, 2, 0, key._ctx, _lib.ptr(z96), None, _lib.ptr(z32), _lib.ptr(z96), _lib.ptr(z96),
                                                                                b"l", 1, ctypes.byref(sp), ctypes.byref(acc), ctypes.byref(why), None),
            "lurk_hip_spartan_verify_batch_dev": lambda: hip.lurk_hip_spartan_verify_batch_dev(ctypes.byref(inst), 1, key._ctx, _lib.ptr(z96), b"l", 1, ctypes.byref(bp),
                                                                                            ctypes.byref(acc), ctypes.byref(why), None),
        }
        for fn, call in more.items():
            rc = call()
            assert rc != 0 and name in hip.lurk_hip_last_error().decode(), (fn, name, hip.lurk_hip_last_error())
            assert acc.value in (0, 7), fn  # never "accepted"
        # the Python mirrors refuse before they build a label or a field for the wrong curve
        from lurk_beta_amd import ipa as IPA, spartan as SP

        for call in (lambda: SP.SpartanProver(cid, B.CURVES[cid].order, [([0, 1, 2], [0, 1], ident)] * 3, 2, 2, 0),
                     lambda: IPA.prove(cid, B.CURVES[cid].order, None, z96, va, vb, 1, lambda *a: 1, key=key),
                     lambda: IPA.verify(key, 2, z96, z96, [z96], [z96], 1, lambda *a: 1, d_b=va)):
            with pytest.raises(LurkHipError, match=name):
                call()
        sh.close()
        # a following valid call works
        sd = dev_scalars(cid, 3, 0, n)
        assert affine(cid, key.commit_device(sd, n)) == B.dlog_checksum_np(B.CURVES[cid], sd.cpu().numpy().view(np.uint64))
        key.close()
