"""lurk_hip_msm_ctx_submit_batch_dev / lurk_hip_msm_ctx_wait_batch: many short commitments under prefixes of one window-table key in one
pass (lurk_beta_amd/csrc/msm_batch.hip).  Needs an MI355X.

Keys of 300 points forced into the table form with LURK_MSM_FLAG_PRECOMPUTE | LURK_MSM_FLAG_WINDOW_BITS(c): the smallest shapes that reach
every branch.  Equality is exact everywhere: as affine points against Python integers (tests/bn254_ref.py for BN254 / Grumpkin: the bases are
[k_i]G, so a commitment is ONE scalar multiple [sum s_i k_i]G; the C oracle's naive sum for Pallas / Vesta), and byte for byte against
lurk_hip_msm_ctx_run_dev on the same vector."""
import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import bn254_ref as B

pytestmark = pytest.mark.gpu

N = 300
PALLAS, VESTA = 0, 1
PASTA_NAME = {PALLAS: "pallas", VESTA: "vesta"}
ALL_CURVES = [PALLAS, VESTA, B.CURVE_BN254, B.CURVE_GRUMPKIN]
CURVE_WIDTHS = [(cid, 20) for cid in ALL_CURVES] + [(cid, c) for cid in (PALLAS, B.CURVE_BN254) for c in (16, 17, 19)]
# special bases of every key: the identity, a repeated point, a point beside its negative
ID_AT, REP_AT, NEG_AT = 1, 3, 5


def order(cid):
    return R.CURVES[PASTA_NAME[cid]]["order"] if cid in PASTA_NAME else B.CURVES[cid].order


def base_p(cid):
    return R.CURVES[PASTA_NAME[cid]]["p"] if cid in PASTA_NAME else B.CURVES[cid].p


_bases, _keys = {}, {}


def bases_of(cid):
    """(host records (N, 8) u64, discrete logs k_i of the BN254-cycle bases or None)"""
    if cid not in _bases:
        if cid in PASTA_NAME:
            rec, logs = C.synth_bases(cid, N).copy(), None
        else:
            c = B.CURVES[cid]
            logs = [c.base_scalar(i) for i in range(N)]
            rec = B.affine_bases(c, c.synth_bases(N))
        rec[ID_AT] = 0
        rec[REP_AT] = rec[REP_AT - 1]
        y = B.limbs_to_ints(rec[NEG_AT - 1, 4:])[0]  # (negation commutes with the Montgomery form)
        rec[NEG_AT, :4] = rec[NEG_AT - 1, :4]
        rec[NEG_AT, 4:] = np.array(B.int_to_limbs((base_p(cid) - y) % base_p(cid)), dtype=np.uint64)
        if logs:
            logs[ID_AT], logs[REP_AT], logs[NEG_AT] = 0, logs[REP_AT - 1], -logs[NEG_AT - 1]
        _bases[cid] = (rec, logs)
    return _bases[cid]


def key_of(cid, c):
    from lurk_beta_amd import CommitmentKey

    if (cid, c) not in _keys:
        ck = CommitmentKey(cid, bases_of(cid)[0], precompute=True, window_bits=c)
        assert ck.info()["form"] == "table" and ck.info()["window_bits"] == c
        _keys[(cid, c)] = ck
    return _keys[(cid, c)]


def reference(cid, scalars):
    """sum_i scalars[i] * base_i as an affine point (None: the identity)"""
    rec, logs = bases_of(cid)
    if not scalars:
        return None
    if logs is None:
        xy = C.jac_to_affine(cid, C.msm_naive(cid, rec[:len(scalars)], C.ints_to_limbs(scalars)))
        return B.from_xy(xy)
    c = B.CURVES[cid]
    return c.mul(sum(s * k for s, k in zip(scalars, logs)) % c.order, c.gen)


def affine(cid, jac):
    from lurk_beta_amd import point_to_affine

    return B.from_xy(point_to_affine(cid, jac))


def pool(cid, c, n=800):
    """n scalars: uniform ones, 0, 1, order - 1, window digits of magnitude exactly 2^(c-1), digits with one half zero and the other not"""
    q, h = order(cid), (c + 1) // 2
    s = [R.uniform_fe(31, i, q) for i in range(n)]
    special = [0, 1, q - 1, 1 << (c - 1), (1 << (c - 1)) << (3 * c), ((1 << (c - 1)) << (5 * c)) | (1 << (c - 1)),
               5 << h, (5 << h) << (2 * c), 3, 3 << (4 * c), ((1 << h) - 1) << c, (1 << h) << c, ((1 << h) + 1) << c,
               (1 << (c - 1)) + 1, q - (1 << (c - 1)), (1 << 253) | 0xFFFF]
    for k, v in enumerate(special):
        for at in (2 * k, 64 + 3 * k, 290 + k // 2, 400 + 5 * k):  # inside every vector of the batches below
            s[at] = v % q
    return s


def to_device(cid, ints, mont):
    import torch

    q = order(cid)
    limbs = B.to_mont(q, ints) if mont else B.ints_to_limbs(ints)
    return torch.from_numpy(limbs.view(np.int64).copy()).cuda()


def run_batch(ck, cid, ints, d_s, offsets, lens, mont, slot=0, check_bytes=True):
    ck.submit_batch_device(slot, d_s, offsets, lens, is_mont=mont)
    got = ck.wait_batch(slot, len(lens))
    assert got.shape == (len(lens), 12)
    for k, (o, n) in enumerate(zip(offsets, lens)):
        assert affine(cid, got[k]) == reference(cid, ints[o:o + n]), (k, o, n)
        if n == 0:
            assert not got[k, 8:].any()
        if check_bytes:
            assert np.array_equal(got[k], ck.commit_device(d_s[o:], n, is_mont=mont)), (k, o, n)
    return got


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("cid,c", CURVE_WIDTHS)
def test_batches_of_every_length_match_the_reference(hip, cid, c, mont):
    ck = key_of(cid, c)
    ints = pool(cid, c)
    d_s = to_device(cid, ints, mont)
    lens = [0, 1, 2, 3, 64, 65, 299, 300]
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at += n
    assert at <= len(ints)
    run_batch(ck, cid, ints, d_s, offs, lens, mont)
    halving = [256 >> k for k in range(8)]
    run_batch(ck, cid, ints, d_s, [sum(halving[:k]) for k in range(8)], halving, mont)
    run_batch(ck, cid, ints, d_s, [7], [300], mont)                      # a single vector
    run_batch(ck, cid, ints, d_s, [5 * k for k in range(64)], [5] * 64, mont, check_bytes=False)  # the most vectors
    got = run_batch(ck, cid, ints, d_s, [0, 10], [0, 0], mont)           # nothing but empty vectors: nothing is launched
    assert not got.any()


def profiled(lib, prefix, fn):
    """fn() under the library's profiler: (result, scopes named `prefix`... opened meanwhile)"""
    import ctypes

    assert lib.lurk_hip_profile_enable(1) == 0 and lib.lurk_hip_profile_reset() == 0
    try:
        out = fn()
        ms, launches = ctypes.c_double(), ctypes.c_uint64()
        assert lib.lurk_hip_profile_get(prefix.encode(), ctypes.byref(ms), ctypes.byref(launches)) == 0
    finally:
        lib.lurk_hip_profile_enable(0)
    return out, launches.value


@pytest.mark.parametrize("cid,c", CURVE_WIDTHS)
def test_the_planned_accumulation_at_small_sizes(hip, cid, c, monkeypatch):
    """LURK_MSM_BATCH_PLANNED=1: the task-planned stages whatever the size (by size they start where a bucket averages more than 32 entries);
    300 equal scalars make buckets of 38 eight-entry tasks: the finalize stage's workgroup path"""
    monkeypatch.setenv("LURK_MSM_BATCH_PLANNED", "1")
    ck = key_of(cid, c)
    v = R.uniform_fe(78, 0, order(cid))
    ints = pool(cid, c) + [v] * 300
    d_s = to_device(cid, ints, True)
    lens = [0, 1, 2, 3, 64, 65, 299, 300]
    _, n = profiled(hip, "msm_batch_tasks", lambda: run_batch(ck, cid, ints, d_s, [sum(lens[:k]) for k in range(8)], lens, True, check_bytes=False))
    assert n == 1
    run_batch(ck, cid, ints, d_s, [800, 0, 790], [300, 300, 300], True, check_bytes=False)
    run_batch(ck, cid, ints, d_s, [5 * k for k in range(64)], [5] * 64, True, check_bytes=False)
    monkeypatch.setenv("LURK_MSM_BATCH_PLANNED", "0")
    _, n = profiled(hip, "msm_batch_tasks", lambda: run_batch(ck, cid, ints, d_s, [800, 0], [300, 300], True, check_bytes=False))
    assert n == 0


@pytest.mark.parametrize("c", [16, 20])
def test_long_vectors_take_the_planned_accumulation_by_size(hip, c):
    """a 4096-point key: batches on either side of the threshold between the two accumulation forms (an average of 32 entries per bucket:
    2 W total > 32 NB, i.e. a mean length above 512 at c = 16 and above 2520 at c = 20),
    against the discrete-log checksum and byte for byte against lurk_hip_msm_ctx_run_dev"""
    from lurk_beta_amd import CommitmentKey, synth

    cid, n = B.CURVE_BN254, 4096
    curve = B.CURVES[cid]
    ck = CommitmentKey(cid, synth.bases(cid, n), n=n, precompute=True, window_bits=c, device=True)
    d_s = synth.scalars(curve.scalar_field, 9, 1, 3 * n)  # witness-like: hot buckets, zeros, small values
    host = d_s.cpu().numpy().view(np.uint64).reshape(-1, 4)
    for lens, planned in (([4096, 4096, 600], True), ([4096, 100, 100, 100], c == 16), ([300, 200], False)):
        offs = [sum(lens[:k]) for k in range(len(lens))]

        def go():
            ck.submit_batch_device(1, d_s, offs, lens)
            return ck.wait_batch(1, len(lens))

        got, tasks = profiled(hip, "msm_batch_tasks", go)
        assert tasks == (1 if planned else 0), (lens, tasks)
        for k, (o, m) in enumerate(zip(offs, lens)):
            assert affine(cid, got[k]) == B.dlog_checksum_np(curve, host[o:o + m]), (lens, k)
            assert np.array_equal(got[k], ck.commit_device(d_s[o:], m)), (lens, k)
    ck.close()


@pytest.mark.parametrize("cid", [PALLAS, B.CURVE_BN254])
def test_equal_scalars_take_the_workgroup_path(hip, cid):
    """300 equal scalars put a whole window into one bucket: more than the direct form's 4 x 64 entries per bucket"""
    ck = key_of(cid, 20)
    v = R.uniform_fe(77, 0, order(cid))
    ints = [v] * 300 + pool(cid, 20, 500)
    d_s = to_device(cid, ints, True)
    run_batch(ck, cid, ints, d_s, [0, 300, 10], [300, 300, 280], True)


@pytest.mark.parametrize("cid", ALL_CURVES)
def test_special_bases_doubling_and_cancellation(hip, cid):
    """equal scalars on the repeated point (the doubling branch), on the point and its negative (cancellation), a scalar on the identity"""
    ck = key_of(cid, 20)
    ints = pool(cid, 20)
    ints[REP_AT - 1] = ints[REP_AT] = 12345
    ints[NEG_AT - 1] = ints[NEG_AT] = 777
    ints[ID_AT] = 999
    d_s = to_device(cid, ints, False)
    got = run_batch(ck, cid, ints, d_s, [0, 0, 0, 0], [6, 300, 2, 0], False)
    only = [0] * 6
    only[NEG_AT - 1] = only[NEG_AT] = 777
    d_o = to_device(cid, only, False)
    got = run_batch(ck, cid, only, d_o, [0], [6], False)
    assert affine(cid, got[0]) is None and not got[0, 8:].any()          # P beside -P alone: the identity


def test_overlapping_and_out_of_order_offsets(hip):
    cid = B.CURVE_BN254
    ck = key_of(cid, 20)
    ints = pool(cid, 20)
    d_s = to_device(cid, ints, True)
    run_batch(ck, cid, ints, d_s, [400, 0, 100, 90, 399, 0], [300, 300, 64, 65, 3, 300], True)


def test_scalars_produced_on_another_stream(hip):
    """the batch is ordered after the stream that produced its scalars"""
    import torch

    from lurk_beta_amd import synth

    cid = B.CURVE_BN254
    ck = key_of(cid, 20)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_s = synth.scalars(B.FIELD_BN254_FR, 5, 0, 600, mont=True)
    lens, offs = [300, 150, 75, 1], [0, 300, 450, 525]
    ck.submit_batch_device(2, d_s, offs, lens, is_mont=True, stream=side.cuda_stream)
    got = ck.wait_batch(2, 4)
    side.synchronize()
    ints = B.CURVES[cid].synth_scalars(5, 0, 600)
    for k in range(4):
        assert affine(cid, got[k]) == reference(cid, ints[offs[k]:offs[k] + lens[k]]), k


def test_two_batches_and_a_commitment_in_flight_and_slot_reuse(hip):
    cid = PALLAS
    ck = key_of(cid, 20)
    ints = pool(cid, 20)
    d_s = to_device(cid, ints, True)
    a = ([0, 300], [300, 128])
    b = ([50, 60, 70], [64, 0, 299])
    for _ in range(2):  # the second round reuses every slot
        ck.submit_batch_device(0, d_s, *a, is_mont=True)
        ck.submit_batch_device(1, d_s, *b, is_mont=True)
        ck.submit_device(2, d_s[20:], 250, is_mont=True)
        one = ck.wait(2)
        got_b = ck.wait_batch(1, 3)
        got_a = ck.wait_batch(0, 2)
        assert affine(cid, one) == reference(cid, ints[20:270])
        for got, (offs, lens) in ((got_a, a), (got_b, b)):
            for k, (o, n) in enumerate(zip(offs, lens)):
                assert affine(cid, got[k]) == reference(cid, ints[o:o + n]), (offs, k)
    ck.submit_device(0, d_s, 300, is_mont=True)  # a batch slot serves an ordinary commitment afterwards
    assert affine(cid, ck.wait(0)) == reference(cid, ints[:300])


def test_refusals_by_message_leave_the_key_usable(hip):
    import ctypes

    from lurk_beta_amd import CommitmentKey, LurkHipError, _lib

    cid = B.CURVE_BN254
    ck = key_of(cid, 20)
    ints = pool(cid, 20)
    d_s = to_device(cid, ints, False)
    lib = hip
    ok_off, ok_len = (ctypes.c_size_t * 2)(0, 100), (ctypes.c_size_t * 2)(100, 50)
    out = np.zeros((64, 12), dtype=np.uint64)

    def still_commits(key=ck):
        assert affine(cid, key.commit_device(d_s, 300)) == reference(cid, ints[:300])

    def refused(word, call):
        with pytest.raises(LurkHipError) as e:
            call()
        assert e.value.code == 2 and word in str(e.value), str(e.value)  # LURK_HIP_ERR_INVALID_ARG
        still_commits()

    raw = lambda ctx, slot, s, off, ln, count: _lib.check(lib.lurk_hip_msm_ctx_submit_batch_dev(ctx, slot, _lib.ptr(s), off, ln, count, 0, None))
    refused("null ctx", lambda: raw(None, 0, d_s, ok_off, ok_len, 2))
    refused("null offsets", lambda: raw(ck._ctx, 0, d_s, None, ok_len, 2))
    refused("null lens", lambda: raw(ck._ctx, 0, d_s, ok_off, None, 2))
    refused("null scalars", lambda: raw(ck._ctx, 0, None, ok_off, ok_len, 2))
    refused("count == 0", lambda: raw(ck._ctx, 0, d_s, ok_off, ok_len, 0))
    refused("LURK_MSM_BATCH_MAX_VECTORS", lambda: ck.submit_batch_device(0, d_s, [0] * 65, [1] * 65))
    refused("LURK_MSM_BATCH_MAX_LEN", lambda: ck.submit_batch_device(0, d_s, [0, 0], [5, (1 << 16) + 1]))
    refused("more scalars than the key has points", lambda: ck.submit_batch_device(0, d_s, [0, 0], [5, 301]))
    refused("slot out of range", lambda: ck.submit_batch_device(6, d_s, [0], [5]))
    refused("slot out of range", lambda: ck.submit_batch_device(-1, d_s, [0], [5]))
    refused("slot out of range", lambda: ck.wait_batch(6, 1))
    refused("null ctx", lambda: _lib.check(lib.lurk_hip_msm_ctx_wait_batch(None, 0, _lib.ptr(out))))
    refused("null output", lambda: _lib.check(lib.lurk_hip_msm_ctx_wait_batch(ck._ctx, 0, None)))
    refused("nothing was submitted", lambda: ck.wait_batch(1, 1))
    # a total above the most needs a key that long vectors fit: 2^16 points, 17 vectors of 2^16 scalars out of one buffer
    import torch

    from lurk_beta_amd import synth

    n16 = 1 << 16
    big = CommitmentKey(cid, synth.bases(cid, n16), n=n16, precompute=True, window_bits=16, device=True)
    d_big = torch.zeros((n16, 4), dtype=torch.int64, device="cuda")
    with pytest.raises(LurkHipError) as e:
        big.submit_batch_device(0, d_big, [0] * 17, [n16] * 17)
    assert e.value.code == 2 and "LURK_MSM_BATCH_MAX_TOTAL" in str(e.value)
    big.submit_batch_device(0, d_big, [0] * 2, [n16, 7])       # all-zero scalars of the longest length: the identity
    assert not big.wait_batch(0, 2).any()
    big.close()
    # a key that is not in the window-table form: plain, and the small-commitment form
    for kw in (dict(), dict(precompute=True, small_form=True)):
        other = CommitmentKey(cid, bases_of(cid)[0], **kw)
        assert other.info()["form"] != "table"
        with pytest.raises(LurkHipError) as e:
            other.submit_batch_device(0, d_s, [0], [5])
        assert e.value.code == 2 and "window-table form" in str(e.value)
        still_commits(other)
        other.close()
    # a slot still pending: a batch behind a batch, a batch behind an ordinary commitment; each wait on the other's kind - and the pending
    # commitment stays pending and waitable
    ck.submit_batch_device(3, d_s, [0, 100], [100, 50])
    refused("slot is busy", lambda: ck.submit_batch_device(3, d_s, [0], [5]))
    with pytest.raises(LurkHipError) as e:
        ck.submit_device(3, d_s, 10)
    assert "busy" in str(e.value)
    for wrong in (lambda: ck.wait(3), lambda: ck.wait_pair(3)):
        with pytest.raises(LurkHipError) as e:
            wrong()
        assert e.value.code == 2 and "lurk_hip_msm_ctx_wait_batch" in str(e.value)
    got = ck.wait_batch(3, 2)
    assert affine(cid, got[0]) == reference(cid, ints[:100]) and affine(cid, got[1]) == reference(cid, ints[100:150])
    ck.submit_device(4, d_s, 300)
    ck.submit_pair_device(5, d_s, 256, 3)
    refused("slot is busy", lambda: ck.submit_batch_device(4, d_s, [0], [5]))
    for slot in (4, 5):
        with pytest.raises(LurkHipError) as e:
            ck.wait_batch(slot, 1)
        assert e.value.code == 2 and "not a batch" in str(e.value)
    assert affine(cid, ck.wait(4)) == reference(cid, ints[:300])
    lo, hi = ck.wait_pair(5)
    want_lo = reference(cid, [s if not (i >> 3) & 1 else 0 for i, s in enumerate(ints[:256])])
    assert affine(cid, lo) == want_lo
    still_commits()
