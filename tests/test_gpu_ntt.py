"""HIP radix-2 NTT against the textbook oracle.  Parity UNPINNED: the reference has no NTT
(SURVEY.md section 0.5).  Every test but the plan-coverage one needs an MI355X.

ntt_device runs one LDS-stage pass below 2^12 and (log_n + 7) / 8 wave-resident passes from 2^12 up, each covering ns stages
(tests/ntt_cases.py: plan).  The sizes below run every plan variant on both fields; test_plan_variants_are_all_parametrised
(CPU) fails when a change to the plan adds a variant no size runs."""
import threading

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import ntt_cases as NC

HOST_SIZES = list(range(0, 21))  # through the host entry (lurk_hip_ntt)
DEV_SIZES = [21, 22, 23]          # through the device entry on device-synthesised inputs
FOUR_PASS = 25


def _dev(f, t, log_n, inverse=False, stream=None):
    """lurk_hip_ntt_dev in place on a (n, 4) int64 device tensor, on `stream` (the current one by default); synchronises."""
    import torch

    from lurk_beta_amd import _lib

    s = stream if stream is not None else torch.cuda.current_stream()
    _lib.check(_lib.load().lurk_hip_ntt_dev(f, _lib.ptr(t), log_n, int(inverse), _lib.ptr(s.cuda_stream)))
    s.synchronize()


def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def test_plan_variants_are_all_parametrised():
    """CPU: the sizes this module runs, planned with ntt_device's formula, cover the LDS path, first-pass ns in {6, 7, 8}, later-pass
    ns in {5, 6, 7, 8} and 2, 3 and 4 passes - and nothing else exists between 2^0 and 2^28 (a new variant must get a size here)."""
    def variants(sizes):
        v = set()
        for log_n in sizes:
            pl = NC.plan(log_n)
            if pl is None:
                v.add(("lds",))
                continue
            v.add(("first", pl[0]))
            v.update(("later", ns) for ns in pl[1:])
            v.add(("passes", len(pl)))
        return v

    want = {("lds",)} | {("first", ns) for ns in (6, 7, 8)} | {("later", ns) for ns in (5, 6, 7, 8)} | {("passes", k) for k in (2, 3, 4)}
    assert variants(range(0, 29)) == want
    # every variant on both fields through the every-output comparisons (test_ntt_matches_oracle, test_ntt_device_entry_2_21_to_2_23,
    # test_four_passes_2_25 runs field 0 forward and field 1 inverse)
    assert variants(HOST_SIZES + DEV_SIZES + [FOUR_PASS]) == want
    assert variants(NC.FAMILY_SIZES) >= {("lds",), ("passes", 2), ("passes", 3), ("passes", 4)}


@pytest.mark.gpu
@pytest.mark.parametrize("f", [0, 1])
@pytest.mark.parametrize("log_n", HOST_SIZES)
def test_ntt_matches_oracle(hip, f, log_n):
    """Every plan up to 2^20 (LDS path; two and three wave passes with first-pass ns 6 / 7 / 8 and later-pass ns 5..8), both fields,
    through the host entry: forward = the oracle on every output, every output canonical, the inverse of the oracle's output and of
    the kernel's own output is the input; at <= 2^6 also the textbook DFT."""
    from lurk_beta_amd import ntt

    n = 1 << log_n
    a = C.synth_scalars(f, 3, 0, n)
    fw = ntt(f, a)
    want = C.ntt(f, a)
    assert np.array_equal(fw, want)
    assert NC.below_p(fw, f)
    if log_n <= 6:
        assert C.limbs_to_ints(fw) == R.dft_naive(R.modulus(f), C.limbs_to_ints(a))
    assert np.array_equal(ntt(f, fw, inverse=True), a)
    back = ntt(f, want, inverse=True)
    assert np.array_equal(back, a)
    assert NC.below_p(back, f)


@pytest.mark.gpu
@pytest.mark.parametrize("f", [0, 1])
@pytest.mark.parametrize("log_n", DEV_SIZES)
def test_ntt_device_entry_2_21_to_2_23(hip, f, log_n):
    """Three wave passes with an 8-stage first pass (7,7,7 / 8,7,7 / 8,8,7), both fields, on device-synthesised inputs: every output
    of the forward transform = the oracle's and canonical; the inverse of the oracle's output is the input."""
    from lurk_beta_amd import synth

    n = 1 << log_n
    d = synth.scalars(f, 3, 0, n)
    host = C.synth_scalars(f, 3, 0, n)
    assert np.array_equal(_host(d[:4096]), host[:4096])
    _dev(f, d, log_n)
    got = _host(d)
    want = C.ntt(f, host)
    assert np.array_equal(got, want)
    assert NC.below_p(got, f)
    d.copy_(_to_dev(want))
    _dev(f, d, log_n, inverse=True)
    back = _host(d)
    assert np.array_equal(back, host)
    assert NC.below_p(back, f)


@pytest.mark.gpu
def test_four_passes_2_25(hip):
    """The four-pass plan (7, 6, 6, 6), never run before: all 2^25 outputs of field 0's forward transform = the oracle's and
    canonical; field 1's inverse transform of a random vector = the oracle's inverse on every output."""
    from lurk_beta_amd import synth

    log_n = FOUR_PASS
    n = 1 << log_n
    assert NC.plan(log_n) == [7, 6, 6, 6]
    d = synth.scalars(0, 5, 0, n)
    host = C.synth_scalars(0, 5, 0, n)
    assert np.array_equal(_host(d[:4096]), host[:4096])
    _dev(0, d, log_n)
    got = _host(d)
    del d
    assert np.array_equal(got, C.ntt(0, host))
    assert NC.below_p(got, 0)
    del got, host
    d = synth.scalars(1, 6, 0, n)
    host = C.synth_scalars(1, 6, 0, n)
    _dev(1, d, log_n, inverse=True)
    got = _host(d)
    del d
    assert np.array_equal(got, C.ntt(1, host, inverse=True))
    assert NC.below_p(got, 1)


def _omega(f, log_n, inverse=False):
    p = R.modulus(f)
    w = R.root_of_unity(p, log_n)
    return pow(w, p - 2, p) if inverse else w


def _sampled_positions(n, seed):
    """every j below 2^16 and 65 536 sampled j above"""
    j = np.arange(min(n, 1 << 16))
    if n > 1 << 16:
        j = np.concatenate([j, np.random.default_rng(seed).integers(1 << 16, n, 1 << 16)])
    return j


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", NC.FAMILY_SIZES)
def test_known_answers_without_the_oracle(hip, log_n):
    """Closed forms in Python integers (pyref.root_of_unity), one size per plan family, the field alternating with the size:
    delta_0 -> all ones; constant c (1, p - 1, random) -> [n c, 0, ..., 0] (the zeros: a lazy value = 0 mod p must leave the last
    pass as a canonical 0); delta_k (k = 1, n/2, n - 1, random) -> omega^(j k) at every j < 2^16 and 65 536 sampled j above
    (pins the bit reversal and the twist indices independently of the oracle); inverse of all ones -> delta_0 (the 1/n scaling)."""
    import torch

    f = log_n % 2
    p = R.modulus(f)
    n = 1 << log_n
    w = _omega(f, log_n)
    ones = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    ones[:, 0] = 1
    for name, kind, v in NC.structured_specs(f, log_n):
        d = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        if kind == "const":
            d[:] = torch.from_numpy(C.ints_to_limbs([v]).view(np.int64)).cuda()
        else:
            d[v, 0] = 1
        _dev(f, d, log_n)
        if kind == "const":
            assert C.limbs_to_ints(_host(d[:1]))[0] == n * v % p, name
            assert not torch.any(d[1:]).item(), name
            continue
        k = v
        if k == 0:
            assert torch.equal(d, ones), name
            continue
        j = _sampled_positions(n, log_n + k)
        got = C.limbs_to_ints(_host(d[torch.from_numpy(j).cuda()]))
        wk = pow(w, k, p)
        want, x = [], 1
        for jj in j[: min(n, 1 << 16)]:
            want.append(x)
            x = x * wk % p
        want += [pow(w, int(jj) * k % n, p) for jj in j[min(n, 1 << 16):]]
        assert got == want, name
    d = ones.clone()
    _dev(f, d, log_n, inverse=True)
    delta0 = torch.zeros_like(d)
    delta0[0, 0] = 1
    assert torch.equal(d, delta0)


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", NC.FAMILY_SIZES)
def test_extreme_operands_against_the_oracle(hip, log_n):
    """All p - 1, alternating 0 / p - 1, p - 1 in one half and 0 in the other (u and v of the last stage from opposite extremes),
    and a mix of p - 1 - small, 2^253 + small and high-limb-heavy values, one size per plan family, both fields alternating with
    the size: every output = the oracle's and canonical, and the inverse brings the input back.  At 2^25 the oracle would take a
    minute per vector: there the three structured vectors are checked against their closed forms on sampled outputs instead."""
    import torch

    f = (log_n + 1) % 2
    p = R.modulus(f)
    n = 1 << log_n
    for name, make in NC.extreme_inputs(f, log_n).items():
        if log_n >= FOUR_PASS and name == "mixed_extremes":
            continue
        a = make()
        d = _to_dev(a)
        _dev(f, d, log_n)
        if log_n < FOUR_PASS:
            got = _host(d)
            assert np.array_equal(got, C.ntt(f, a)), name
            assert NC.below_p(got, f), name
        else:
            c = p - 1
            w = _omega(f, log_n)
            j = _sampled_positions(n, 7)
            got = C.limbs_to_ints(_host(d[torch.from_numpy(j).cuda()]))
            for jj, g in zip(j.tolist(), got):
                if name == "all_p_minus_1":
                    want = n * c % p if jj == 0 else 0
                elif name == "alternating_0_p_minus_1":  # c (1 - (-1)^i) / 2
                    want = (n // 2) * c * (1 if jj == 0 else -1 if jj == n // 2 else 0) % p
                else:  # c sum_{i < n/2} omega^(i j): n/2 c at 0, 0 at other even j, 2 c / (1 - omega^j) at odd j
                    want = (n // 2) * c % p if jj == 0 else 0 if jj % 2 == 0 else 2 * c * pow(1 - pow(w, jj, p), p - 2, p) % p
                assert g == want, (name, jj)
        _dev(f, d, log_n, inverse=True)
        if log_n < FOUR_PASS:
            assert np.array_equal(_host(d), a), name
        else:
            assert torch.equal(d, _to_dev(a)), name


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [12, 17])
def test_convolution_theorem(hip, log_n):
    """inverse(NTT(a) * NTT(b)) = the cyclic convolution of a with a sparse b (4 non-zeros), both transforms on the GPU (two and
    three wave passes), the pointwise product and the convolution (a sum of rotated, scaled copies of a) on the host."""
    f = log_n % 2
    p = R.modulus(f)
    n = 1 << log_n
    a = C.synth_scalars(f, 8, 0, n)
    rng = np.random.default_rng(log_n)
    pos = [0, 1] + [int(x) for x in rng.choice(np.arange(2, n), 2, replace=False)]
    val = [p - 1, 1, R.uniform_fe(81, 0, p), R.uniform_fe(81, 1, p)]
    b = np.zeros((n, 4), dtype=np.uint64)
    for s, c in zip(pos, val):
        b[s] = C.ints_to_limbs([c])[0]
    want = np.zeros((n, 4), dtype=np.uint64)
    for s, c in zip(pos, val):
        want = C.axpy(f, want, np.roll(a, s, axis=0), c)  # (b * a)[j] = sum_s b_s a[j - s]
    da, db = _to_dev(a), _to_dev(b)
    _dev(f, da, log_n)
    _dev(f, db, log_n)
    prod = C.mul_canonical(f, _host(da), _host(db))
    dp = _to_dev(prod)
    _dev(f, dp, log_n, inverse=True)
    assert np.array_equal(_host(dp), want)


@pytest.mark.gpu
def test_non_default_stream_and_shared_plan_concurrency(hip):
    """On non-default torch streams: one transform alone; then, for three rounds, two streams at once on distinct buffers with the
    same (field, log_n, direction) - one cached NttPlan, one twiddle table, each its own stream-ordered scratch - and two sizes at
    once; every result exact against the oracle."""
    import torch

    f = 1
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a16 = [C.synth_scalars(f, 20 + i, 0, 1 << 16) for i in range(2)]
    w16 = [C.ntt(f, a) for a in a16]
    a18 = C.synth_scalars(f, 22, 0, 1 << 18)
    w18 = C.ntt(f, a18)
    d = _to_dev(a16[0])
    torch.cuda.synchronize()
    _dev(f, d, 16, stream=s1)
    assert np.array_equal(_host(d), w16[0])
    from lurk_beta_amd import _lib

    lib = _lib.load()
    for rnd in range(3):
        x, y = _to_dev(a16[0]), _to_dev(a16[1])
        z = _to_dev(a18)
        torch.cuda.synchronize()
        _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(x), 16, 0, _lib.ptr(s1.cuda_stream)))
        _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(y), 16, 0, _lib.ptr(s2.cuda_stream)))
        s1.synchronize()
        s2.synchronize()
        assert np.array_equal(_host(x), w16[0]) and np.array_equal(_host(y), w16[1]), rnd
        x = _to_dev(a16[1])
        torch.cuda.synchronize()
        _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(z), 18, 0, _lib.ptr(s1.cuda_stream)))
        _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(x), 16, 0, _lib.ptr(s2.cuda_stream)))
        s1.synchronize()
        s2.synchronize()
        assert np.array_equal(_host(z), w18) and np.array_equal(_host(x), w16[1]), rnd


@pytest.mark.gpu
def test_first_use_of_a_plan_from_two_threads(hip):
    """Two Python threads make the first use of a plan key no other test uses (field 0, 2^24, inverse) at the same moment, each on
    its own stream: the plan cache builds one twiddle table under its lock and both results are exact (the oracle's forward output
    comes back to the input)."""
    import torch

    from lurk_beta_amd import _lib

    f, log_n = 0, 24
    n = 1 << log_n
    host = C.synth_scalars(f, 9, 0, n)
    fw = C.ntt(f, host)
    bufs = [_to_dev(fw), _to_dev(fw)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    lib = _lib.load()
    go = threading.Barrier(2)
    rcs = [None, None]

    def run(i):
        go.wait()
        rcs[i] = lib.lurk_hip_ntt_dev(f, _lib.ptr(bufs[i]), log_n, 1, _lib.ptr(streams[i].cuda_stream))
        streams[i].synchronize()

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert rcs == [0, 0]
    want = _to_dev(host)
    assert torch.equal(bufs[0], want) and torch.equal(bufs[1], want)


@pytest.mark.gpu
def test_window_at_an_offset_leaves_its_neighbours_alone(hip):
    """A 2^14 transform of a window that starts 32 bytes into a larger tensor, both directions: the window is exact and the elements
    on either side (sentinels) are untouched - no pass reads or writes outside [ptr, ptr + n * 32)."""
    import torch

    f, log_n = 0, 14
    n = 1 << log_n
    a = C.synth_scalars(f, 11, 0, n)
    big = np.full((n + 2, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    big[1:n + 1] = a
    d = _to_dev(big)
    window = d[1:n + 1]
    assert window.data_ptr() == d.data_ptr() + 32
    _dev(f, window, log_n)
    got = _host(d)
    assert np.array_equal(got[1:n + 1], C.ntt(f, a))
    assert np.array_equal(got[0], big[0]) and np.array_equal(got[n + 1], big[n + 1])
    _dev(f, window, log_n, inverse=True)
    assert torch.equal(d, _to_dev(big))


@pytest.mark.gpu
def test_refusals_on_both_entries(hip):
    """log_n = 29, field 2 (BN254: no NTT) and a null buffer raise LurkHipError on the host and the device entry without touching
    the buffer."""
    import torch

    from lurk_beta_amd import LurkHipError, _lib, ntt

    lib = _lib.load()
    a = C.synth_scalars(1, 3, 0, 8)
    keep = a.copy()
    with pytest.raises(LurkHipError):
        ntt(2, a)  # BN254 is not offered
    for args in ((2, _lib.ptr(a), 3, 0), (1, _lib.ptr(a), 29, 0), (0, _lib.ptr(None), 3, 0), (1, _lib.ptr(None), 3, 1)):
        with pytest.raises(LurkHipError):
            _lib.check(lib.lurk_hip_ntt(*args))
    assert np.array_equal(a, keep)
    d = _to_dev(a)
    s = _lib.ptr(torch.cuda.current_stream().cuda_stream)
    for args in ((2, _lib.ptr(d), 3, 0, s), (1, _lib.ptr(d), 29, 0, s), (0, _lib.ptr(None), 3, 0, s), (1, _lib.ptr(None), 3, 1, s)):
        with pytest.raises(LurkHipError):
            _lib.check(lib.lurk_hip_ntt_dev(*args))
    torch.cuda.synchronize()
    assert np.array_equal(_host(d), keep)


@pytest.mark.gpu
def test_ntt_large_roundtrip_and_linearity(hip):
    from lurk_beta_amd import LurkHipError, ntt

    f, n = 1, 1 << 20
    a = C.synth_scalars(f, 3, 0, n)
    fw = ntt(f, a)
    assert np.array_equal(fw, C.ntt(f, a))
    assert np.array_equal(ntt(f, fw, inverse=True), a)
    with pytest.raises(LurkHipError):
        ntt(2, a[:8])  # BN254 is not offered


@pytest.mark.gpu
def test_full_size_roundtrip_and_linearity_2_24(hip):
    """2^24 elements on the device API: inverse(forward(a)) = a, and forward(a + r b) = forward(a) + r forward(b)
    (checked on the GPU with the fold kernel, then on 4096 sampled positions by the oracle)."""
    import torch

    from lurk_beta_amd import _lib, fold_vec, synth

    lib = _lib.load()
    f, log_n = 1, 24
    n = 1 << log_n
    stream = torch.cuda.current_stream().cuda_stream
    p = R.modulus(f)
    a = synth.scalars(f, 3, 0, n, mont=True)
    b = synth.scalars(f, 4, 0, n, mont=True)
    r = R.uniform_fe(75, 0, p)
    r_mont = C.to_mont(f, C.ints_to_limbs([r]))
    # the NTT takes canonical bytes; Montgomery inputs are canonical bytes of x R, and the transform is linear: fine for both properties
    c = fold_vec(f, a, b, r_mont)
    a0 = a.clone()
    for t in (a, b, c):
        _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(t), log_n, 0, _lib.ptr(stream)))
    lin = fold_vec(f, a, b, r_mont)
    assert torch.equal(lin, c)
    idx = torch.from_numpy(np.random.default_rng(6).integers(0, n, 4096)).cuda()
    ha, hb, hc = (t[idx].cpu().numpy().view(np.uint64) for t in (a, b, c))
    assert np.array_equal(C.from_mont(f, hc), C.axpy(f, C.from_mont(f, ha), C.from_mont(f, hb), r))
    _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(a), log_n, 1, _lib.ptr(stream)))
    assert torch.equal(a, a0)


@pytest.mark.gpu
def test_full_size_2_24_every_output_against_the_oracle(hip):
    """BASELINE-size transform compared DIRECTLY: all 2^24 outputs of the forward NTT equal the oracle's (a consistent error in the
    third pass would survive the round trip and the linearity check above), and the inverse of the oracle's output is the input."""
    import torch

    from lurk_beta_amd import _lib, synth

    lib = _lib.load()
    f, log_n = 1, 24
    n = 1 << log_n
    stream = torch.cuda.current_stream().cuda_stream
    d = synth.scalars(f, 3, 0, n)
    host = C.synth_scalars(f, 3, 0, n)
    assert np.array_equal(d[:4096].cpu().numpy().view(np.uint64), host[:4096])
    _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(d), log_n, 0, _lib.ptr(stream)))
    torch.cuda.synchronize()
    want = C.ntt(f, host)
    got = d.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert np.array_equal(got, want)
    assert NC.below_p(got, f)
    d.copy_(torch.from_numpy(want.view(np.int64)))
    _lib.check(lib.lurk_hip_ntt_dev(f, _lib.ptr(d), log_n, 1, _lib.ptr(stream)))
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64).reshape(-1, 4), host)
