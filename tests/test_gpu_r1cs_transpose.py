"""GPU: a resident shape transposed on the device (lurk_hip_r1cs_transpose_dev) and read back to the host (lurk_hip_r1cs_read), against
the host transpose the provers used so far (lurk_beta_amd.spartan.transpose_csr), Python integers, and the compressing provers fed with
either transpose.  Every comparison is equality."""
import ctypes

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R

pytestmark = pytest.mark.gpu
FIELDS = [0, 1, 2]
SLOT_TYPES = [4, 6, 8, 3, 1]  # (hash4, hash6, hash8, commitment, bit_decomp): LURK_SLOT_*


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _pool(f, seed, n=48):
    """n distinct coefficients: 1, p - 1, 2 and random ones; (ints, (n, 4) Montgomery)"""
    p = R.modulus(f)
    ints = [1, p - 1, 2] + C.limbs_to_ints(C.synth_scalars(f, seed, 0, n - 3))
    assert len(set(ints)) == n
    return ints, C.to_mont(f, C.ints_to_limbs(ints))


def _csr(rows, pool_mont):
    """rows: per row a list of (column, pool index) -> (indptr, indices, data Montgomery), and the same as (row, column, pool index) triples"""
    ip = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum(np.array([len(r) for r in rows], dtype=np.uint64), out=ip[1:])
    flat = [e for r in rows for e in r]
    ix = np.array([c for c, _ in flat], dtype=np.uint64)
    dv = pool_mont[np.array([k for _, k in flat], dtype=np.int64)] if flat else np.zeros((0, 4), dtype=np.uint64)
    return ip, ix, np.ascontiguousarray(dv)


def _same(got, want):
    return all(np.array_equal(np.asarray(g, dtype=np.uint64).reshape(-1), np.asarray(w, dtype=np.uint64).reshape(-1)) for g, w in zip(got, want)) and len(got) == len(want)


def _read_all(shape):
    return [shape.read(w) for w in range(3)]


def _check_transpose(shape, mats, rows_t):
    """read(transposed(shape, rows_t)) == transpose_csr of the host CSR, info() as the source's, and the same bytes on a second call"""
    from lurk_beta_amd.spartan import transpose_csr

    n_rows = rows_t if rows_t else shape.num_cols
    t = shape.transposed(rows_t)
    assert (t.field_id, t.num_cons, t.num_vars, t.num_io) == (shape.field_id, n_rows, shape.num_cons - 1, 0)
    assert t.info() == shape.info()
    got = _read_all(t)
    for w in range(3):
        assert _same(got[w], transpose_csr(*mats[w], n_rows)), (w, rows_t)
    again = shape.transposed(rows_t)
    for w in range(3):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again.read(w), got[w]))
    again.close()
    return t


def _edge(f):
    """num_cons 300, num_vars 40, num_io 2 (43 columns).  A: an entry in column 40 (u) in every row - a transposed row of 300 entries,
    beyond a wave, a 256-thread workgroup and the 32-entry bound of the lane-per-row kernels - a duplicated (7, 3) with two different
    coefficients, a row with the u entry alone.  B: column 11 with exactly 32 entries (not a long row), column 12 with 33 (a long row),
    most rows empty.  C: empty.
    Columns 5, 6, 20-29, 41 and 42 are untouched by every matrix."""
    ints, pool = _pool(f, 700 + f)
    rng = np.random.default_rng(70 + f)
    free = [c for c in range(40) if c not in (3, 5, 6, 11, 12) and not 20 <= c <= 29]
    a_rows, b_rows = [], []
    for i in range(300):
        row = [(int(c), int(rng.integers(0, len(ints)))) for c in sorted(rng.choice(free, size=int(rng.integers(0, 4)), replace=False))]
        if i == 7:
            row = [(3, 4), (3, 5)] + row  # the same (i, j) twice: both stay, in this order
        a_rows.append(sorted(row, key=lambda e: e[0]) + [(40, int(rng.integers(0, len(ints))))])
        b = []
        if i % 9 == 0 and i // 9 < 32:
            b.append((11, int(rng.integers(0, len(ints)))))
        if i % 9 == 1 and i // 9 < 33:
            b.append((12, int(rng.integers(0, len(ints)))))
        if i % 50 == 49:
            b.append((int(rng.choice(free)), 1))
        b_rows.append(sorted(b, key=lambda e: e[0]))
    a_rows[100] = [a_rows[100][-1]]
    c_rows = [[] for _ in range(300)]
    assert sum(1 for r in b_rows for c, _ in r if c == 11) == 32 and sum(1 for r in b_rows for c, _ in r if c == 12) == 33
    triples = [[(i, c, ints[k]) for i, r in enumerate(rows) for c, k in r] for rows in (a_rows, b_rows, c_rows)]
    return [_csr(rows, pool) for rows in (a_rows, b_rows, c_rows)], triples


def _frames_host(f, num_frames, counts, first, frame_len, nv, extra_cons=0):
    """the rows lurk_hip_frames_r1cs_create builds, relocated on the host from lurk_hip_slot_constraints (Montgomery data)"""
    from lurk_beta_amd import slot_constraints, slot_witness_size

    mats = [([0], [], []) for _ in range(3)]
    for fr in range(num_frames):
        base = first + fr * frame_len
        for n, t in zip(counts, SLOT_TYPES):
            if not n:
                continue
            size = slot_witness_size(f, t)
            cons = slot_constraints(f, t)
            for _k in range(n):
                for w in range(3):
                    ip, ix, dv = cons[w]
                    at = len(mats[w][1])
                    mats[w][1].extend(nv if int(col) == size else base + int(col) for col in ix)
                    mats[w][2].append(np.ascontiguousarray(dv).reshape(-1, 4))
                    mats[w][0].extend(at + int(x) for x in ip[1:])
                base += size
    out = []
    for ip, ix, dv in mats:
        ip = ip + [ip[-1]] * extra_cons
        out.append((np.array(ip, dtype=np.uint64), np.array(ix, dtype=np.uint64), np.concatenate(dv) if dv else np.zeros((0, 4), dtype=np.uint64)))
    return out


# ---- 1. read ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS)
def test_a_created_shape_reads_back_as_it_was_given(hip, f):
    from lurk_beta_amd import R1CSShape

    _, pool = _pool(f, 600 + f)
    a = [[], [(0, 0), (3, 1), (11, 2)], [], [], [(11, 7), (2, 8), (2, 9)], [(5, 1)], []]  # empty rows first, last and in between
    b = [[(1, 3)], [], [(4, 4), (10, 47)], [], [], [], [(0, 0)]]
    mats = [_csr(a, pool), _csr(b, pool), _csr([[] for _ in range(7)], pool)]  # C: all empty
    shape = R1CSShape(f, 7, 9, 2, *mats)
    for w in range(3):
        assert _same(shape.read(w), mats[w]), w
    shape.close()
    empty = [_csr([[], [], []], pool) for _ in range(3)]  # nnz = 0 in every matrix
    shape = R1CSShape(f, 3, 4, 1, *empty)
    for w in range(3):
        ip, ix, dv = shape.read(w)
        assert ip.tolist() == [0, 0, 0, 0] and ix.size == 0 and dv.shape == (0, 4)
    shape.close()


@pytest.mark.parametrize("f", FIELDS)
def test_a_frames_shape_reads_back_as_the_relocated_slot_rows(hip, f):
    """lurk_hip_frames_r1cs_create's relocation, read for the first time: two frames of all five slot types against the host's own
    relocation of lurk_hip_slot_constraints."""
    from lurk_beta_amd import R1CSShape, slot_witness_size

    counts = [2, 1, 1, 1, 2]
    shape_len = sum(n * slot_witness_size(f, t) for n, t in zip(counts, SLOT_TYPES))
    num_frames, first = 2, 3
    nv, nio = first + num_frames * shape_len + 4, 2
    shape = R1CSShape.for_frames(f, num_frames, counts, first, shape_len, nv, nio)
    want = _frames_host(f, num_frames, counts, first, shape_len, nv)
    assert shape.num_cons == want[0][0].size - 1
    for w in range(3):
        assert _same(shape.read(w), want[w]), w
    shape.close()


# ---- 2. the transpose equals the host transpose ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS)
def test_transpose_of_the_edge_shape_equals_the_host_transpose(hip, f):
    from lurk_beta_amd import R1CSShape

    mats, _ = _edge(f)
    shape = R1CSShape(f, 300, 40, 2, *mats)
    for rows_t in (0, 43, 128):
        _check_transpose(shape, mats, rows_t).close()
    for w in range(3):
        assert _same(shape.read(w), mats[w])  # the source is untouched
    shape.close()


def _random_shape(f, num_cons, num_vars, num_io, per_row, seed):
    _, pool = _pool(f, seed)
    rng = np.random.default_rng(seed)
    ncols = num_vars + 1 + num_io
    mats = []
    for w in range(3):
        ip = np.arange(num_cons + 1, dtype=np.uint64) * np.uint64(per_row[w])
        ix = rng.integers(0, ncols, num_cons * per_row[w]).astype(np.uint64)
        mats.append((ip, ix, np.ascontiguousarray(pool[rng.integers(0, len(pool), ix.size)])))
    return mats


def test_transpose_of_a_wide_shape_equals_the_host_transpose(hip):
    """5000 rows over 4096 columns, three random entries per row, 8192 output rows.  Every kernel of the transpose (key expansion, row
    pointers from the run boundaries, the long-row count and compaction) gives a 256-thread workgroup a tile of 256 entries or 256 output
    rows: 8192 rows are 32 tiles, 15 000 entries 59."""
    from lurk_beta_amd import R1CSShape

    f = 1
    mats = _random_shape(f, 5000, 4095, 0, (3, 3, 3), 811)
    shape = R1CSShape(f, 5000, 4095, 0, *mats)
    assert 8192 > 2 * 256
    _check_transpose(shape, mats, 8192).close()
    shape.close()


def test_transpose_beyond_the_sorts_size_thresholds(hip):
    """The sort the transpose leans on changes its algorithm with the number of entries (one workgroup; a merge sort up to 2^20; passes over
    the digits above): A holds 1 050 000 entries, B 700 000, C a single one; and an output of 2^21 rows gives the scan over the 256-row
    tiles' long-row counts 8193 inputs."""
    from lurk_beta_amd import R1CSShape

    f = 1
    num_cons, nv, nio = 350_000, 65_533, 2
    mats = _random_shape(f, num_cons, nv, nio, (3, 2, 0), 823)
    _, pool = _pool(f, 823)
    ip = np.zeros(num_cons + 1, dtype=np.uint64)
    ip[-1] = 1
    mats[2] = (ip, np.array([nv], dtype=np.uint64), np.ascontiguousarray(pool[5:6]))
    shape = R1CSShape(f, num_cons, nv, nio, *mats)
    assert mats[0][1].size > 1 << 20
    _check_transpose(shape, mats, 2 * nv).close()
    shape.close()
    small, _ = _edge(f)
    shape = R1CSShape(f, 300, 40, 2, *small)
    _check_transpose(shape, small, 1 << 21).close()
    shape.close()


# ---- 3. products ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FIELDS)
def test_the_transposed_shape_multiplies_as_the_transposed_matrices(hip, f):
    """M^T v in Python integers: the 300-entry row and the 33-entry row go through the wave-per-row kernel, the 32-entry row through the
    lane-per-row one - a row missing from the long-row list is left unwritten, one listed twice is caught by the read-back above."""
    from lurk_beta_amd import R1CSShape

    p = R.modulus(f)
    mats, triples = _edge(f)
    shape = R1CSShape(f, 300, 40, 2, *mats)
    v = C.synth_scalars(f, 900 + f, 0, 300)
    vi = C.limbs_to_ints(v)
    for rows_t in (0, 128):
        t = shape.transposed(rows_t)
        got = t.multiply_vec(_dev(C.to_mont(f, v)))
        n = rows_t if rows_t else 43
        for w in range(3):
            want = [0] * n
            for i, c, coef in triples[w]:
                want[c] = (want[c] + coef * vi[i]) % p
            assert C.limbs_to_ints(C.from_mont(f, _host(got[w]))) == want, (w, rows_t)
        t.close()
    shape.close()


@pytest.mark.parametrize("f", FIELDS)
def test_transposing_twice_gives_the_shape_with_columns_ascending(hip, f):
    from lurk_beta_amd import R1CSShape
    from lurk_beta_amd.spartan import transpose_csr

    mats, _ = _edge(f)
    shape = R1CSShape(f, 300, 40, 2, *mats)
    t = shape.transposed(43)
    tt = t.transposed(300)
    assert (tt.num_cons, tt.num_vars, tt.num_io) == (300, 42, 0) and tt.info() == shape.info()
    for w in range(3):
        want = transpose_csr(*transpose_csr(*mats[w], 43), 300)
        assert _same(tt.read(w), want)
        assert np.array_equal(want[0], mats[w][0])  # the same rows, each sorted by column (stable)
    for s in (tt, t, shape):
        s.close()


# ---- 4. the provers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn,c", [("pallas", 0), ("vesta", 1)])
def test_spartan_proof_from_a_resident_shape_equals_the_host_transposes(hip, cn, c):
    from lurk_beta_amd import CommitmentKey, R1CSShape
    from lurk_beta_amd.spartan import SpartanProver, SpartanVerifier
    from tests.test_gpu_spartan_verify import _instance, _mont_mats

    nc, nv = 64, 128
    I = _instance(cn, c, nc, nv, True)
    sf, q, N, B = I["sf"], I["q"], I["N"], I["B"]
    mats = _mont_mats(sf, I["mats"])
    host = SpartanProver(c, q, mats, nc, nv, len(I["X"]))
    dev = SpartanProver.from_shape(c, q, R1CSShape(sf, nc, nv, len(I["X"]), *mats), nc, nv, len(I["X"]))
    for w in range(3):
        assert _same(dev.shape_t.read(w), host.shape_t.read(w))
    key = CommitmentKey(c, B[:N])
    cw, ce = key.commit(I["W"]), key.commit(I["E"])
    args = (I["X"], I["u"], _dev(C.to_mont(sf, I["W"])), _dev(C.to_mont(sf, I["E"])), _dev(B), cw, ce)
    want = host.prove(*args, key=key, in_library=True)
    got = dev.prove(*args, key=key, in_library=True)
    assert got == want
    verifier = SpartanVerifier.from_shape(dev.shape, c, q)
    assert verifier.verify(I["X"], I["u"], cw, ce, got, key, d_ck=_dev(B)) is True and verifier.last_failed_check == 0
    bad_x = [(I["X"][0] + 1) % q] + I["X"][1:]
    assert verifier.verify(bad_x, I["u"], cw, ce, got, key, d_ck=_dev(B)) is False
    key.close()
    host.close()
    dev.close()


@pytest.mark.parametrize("nc,nv,nio", [(2, 2, 1), (8, 16, 2)])
def test_spartan_kzg_proof_from_a_resident_shape_equals_the_host_transposes(hip, nc, nv, nio):
    from lurk_beta_amd import R1CSShape, SpartanKzgProver, SpartanKzgVerifier, hyperkzg
    from tests import spartan_kzg_ref as K
    from tests.test_gpu_spartan_kzg import Q, TAU, device_instance, mats_mont

    key = hyperkzg.trapdoor_key(TAU, 64)
    it = K.make_instance(TAU, nc, nv, nio, 11 + nc + nv, True)
    mats = mats_mont(it["mats"])
    host = SpartanKzgProver(mats, nc, nv, nio)
    dev = SpartanKzgProver.from_shape(2, Q, R1CSShape(2, nc, nv, nio, *mats), nc, nv, nio)
    for w in range(3):
        assert _same(dev.shape_t.read(w), host.shape_t.read(w))
    di = device_instance(it, key)
    args = (di["X"], di["u"], di["d_W"], di["d_E"], di["comm_W"], di["comm_E"], key)
    want = host.prove(*args)
    got = dev.prove(*args)
    assert got == want
    verifier = SpartanKzgVerifier.from_shape(dev.shape)
    ok, _, _ = verifier.verify(di["X"], di["u"], di["comm_W"], di["comm_E"], got)
    assert ok and verifier.last_failed_check == 0
    bad_x = [(di["X"][0] + 1) % Q] + list(di["X"][1:])
    assert not verifier.verify(bad_x, di["u"], di["comm_W"], di["comm_E"], got)[0]
    host.close()
    dev.close()
    key.close()


# ---- 5. what was impossible before: a shape the library built, compressed without any host CSR -----------------------------------------------
def test_a_frames_shape_is_compressed_without_a_host_csr(hip):
    import torch

    from lurk_beta_amd import CommitmentKey, MultiFrameWitness, slot_constraints
    from lurk_beta_amd.spartan import SpartanProver, SpartanVerifier

    cn, c, f, nio = "pallas", 0, 1, 2
    q = R.CURVES[cn]["order"]
    counts = {"hash4": 1, "hash6": 0, "hash8": 1, "commitment": 1, "bit_decomp": 1}
    counts5 = [counts[k] for k in ("hash4", "hash6", "hash8", "commitment", "bit_decomp")]
    probe = MultiFrameWitness(f, 1, 3, 0, slot_counts=counts)
    nv = 1 << probe.w_len.bit_length()  # a power of two with room for the globals and the slot blocks
    mf = MultiFrameWitness(f, 1, 3, nv - 3 - probe.slots_len, slot_counts=counts)
    assert mf.w_len == nv
    slot_rows = sum(n * (slot_constraints(f, t)[0][0].size - 1) for n, t in zip(counts5, SLOT_TYPES))
    nc = 1 << (slot_rows - 1).bit_length()
    pad = np.zeros(nc - slot_rows + 1, dtype=np.uint64)
    no_rows = (pad, np.zeros(0, dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
    shape = mf.r1cs(nio, extra=(no_rows, no_rows, no_rows) if nc > slot_rows else None)
    assert (shape.num_cons, shape.num_vars, shape.num_io) == (nc, nv, nio)
    # W traced by the library, z = [W | 1 | X]
    pre = {name: _dev(C.to_mont(f, C.synth_scalars(f, 950 + st, 1, counts[name] * st)))
           for name, st in (("hash4", 4), ("hash8", 8), ("commitment", 3), ("bit_decomp", 1))}
    d_z = torch.zeros((nv + 1 + nio, 4), dtype=torch.int64, device="cuda")
    g = C.to_mont(f, C.synth_scalars(f, 970, 0, mf.globals_len))
    body = C.to_mont(f, C.synth_scalars(f, 971, 0, mf.body_len)).reshape(1, mf.body_len, 4)
    mf.assemble(d_z, pre, g, body, mont=True)
    X = C.limbs_to_ints(C.synth_scalars(f, 972, 0, nio))
    d_z[nv:] = _dev(C.to_mont(f, C.ints_to_limbs([1] + X)))
    torch.cuda.synchronize()
    assert shape.is_sat(d_z) == (0, nc)
    N = max(nc, nv)
    B = C.synth_bases(c, N + 1)
    key = CommitmentKey(c, B[:N])
    d_W, d_E = d_z[:nv].contiguous(), torch.zeros((nc, 4), dtype=torch.int64, device="cuda")
    cw, ce = key.commit(C.from_mont(f, _host(d_W))), key.commit(np.zeros((nc, 4), dtype=np.uint64))
    prover = SpartanProver.from_shape(c, q, shape, nc, nv, nio)  # no host CSR anywhere on this path
    proof = prover.prove(X, 1, d_W, d_E, _dev(B), cw, ce, key=key, in_library=True)
    verifier = SpartanVerifier.from_shape(prover.shape, c, q)
    assert verifier.verify(X, 1, cw, ce, proof, key, d_ck=_dev(B)) is True and verifier.last_failed_check == 0
    # the same proof through the host: the rows rebuilt from lurk_hip_slot_constraints, transposed by numpy, uploaded twice
    host_mats = _frames_host(f, 1, counts5, mf.globals_len, mf.frame_len, nv, extra_cons=nc - slot_rows)
    for w in range(3):
        assert _same(prover.shape.read(w), host_mats[w])
    host = SpartanProver(c, q, host_mats, nc, nv, nio)
    assert host.prove(X, 1, d_W, d_E, _dev(B), cw, ce, key=key, in_library=True) == proof
    key.close()
    host.close()
    prover.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_no_handle_and_the_source_intact(hip):
    import torch

    from lurk_beta_amd import R1CSShape, _lib

    f = 1
    p = R.modulus(f)
    lib = _lib.load()
    mats, triples = _edge(f)
    shape = R1CSShape(f, 300, 40, 2, *mats)
    _, pool = _pool(f, 601)
    no_rows = R1CSShape(f, 0, 4, 1, *[_csr([], pool) for _ in range(3)])

    def refused(handle, rows_t, message, with_out=True):
        out = ctypes.c_void_p(0xDEAD)
        rc = lib.lurk_hip_r1cs_transpose_dev(handle, rows_t, ctypes.byref(out) if with_out else None, None)
        assert rc == 2 and message in lib.lurk_hip_last_error().decode(), (rc, lib.lurk_hip_last_error())
        assert not with_out or out.value is None

    refused(None, 0, "null argument")
    refused(shape._h, 0, "null argument", with_out=False)
    refused(no_rows._h, 0, "num_cons = 0")
    refused(shape._h, 42, "rows_t is below the shape's num_vars + 1 + num_io columns")
    refused(shape._h, 1, "rows_t is below the shape's num_vars + 1 + num_io columns")
    refused(shape._h, 1 << 32, "rows_t must be below 2^32")
    refused(shape._h, (1 << 64) - 1, "rows_t must be below 2^32")
    if torch.cuda.device_count() > 1:  # resident on device 0, asked for from device 1
        torch.cuda.set_device(1)
        try:
            refused(shape._h, 0, "the shape is resident on another device than the current one")
            ip = np.zeros(301, dtype=np.uint64)
            assert lib.lurk_hip_r1cs_read(shape._h, 0, _lib.ptr(ip), None, None) == 2
            assert "the shape is resident on another device than the current one" in lib.lurk_hip_last_error().decode()
        finally:
            torch.cuda.set_device(0)
    ip = np.zeros(301, dtype=np.uint64)
    for which in (-1, 3):
        assert lib.lurk_hip_r1cs_read(shape._h, which, _lib.ptr(ip), None, None) == 2
        assert "unknown matrix id (0 = A, 1 = B, 2 = C)" in lib.lurk_hip_last_error().decode()
    assert lib.lurk_hip_r1cs_read(None, 0, _lib.ptr(ip), None, None) == 2 and "null shape" in lib.lurk_hip_last_error().decode()
    assert lib.lurk_hip_r1cs_read(shape._h, 0, None, None, None) == 2 and "null indptr" in lib.lurk_hip_last_error().decode()
    assert lib.lurk_hip_r1cs_read(shape._h, 0, _lib.ptr(ip), None, None) == 2 and "null indices" in lib.lurk_hip_last_error().decode()
    ix = np.zeros(mats[0][1].size, dtype=np.uint64)
    assert lib.lurk_hip_r1cs_read(shape._h, 0, _lib.ptr(ip), _lib.ptr(ix), None) == 0  # the structure alone
    assert np.array_equal(ip, mats[0][0]) and np.array_equal(ix, mats[0][1])
    # the source still multiplies
    z = C.synth_scalars(f, 990, 0, 43)
    zi = C.limbs_to_ints(z)
    got = shape.multiply_vec(_dev(C.to_mont(f, z)))
    for w in range(3):
        want = [0] * 300
        for i, c, coef in triples[w]:
            want[i] = (want[i] + coef * zi[c]) % p
        assert C.limbs_to_ints(C.from_mont(f, _host(got[w]))) == want
    shape.close()
    no_rows.close()
