"""GPU: the witness blocks of the trie coprocessor's step circuits (lurk_hip_trie_circuit_witness_dev) against the Python restatement
of Trie::synthesize_lookup / synthesize_insert (tests/trie_circuit_ref.py) and against the library's own rows
(lurk_hip_trie_circuit_r1cs_create + lurk_hip_r1cs_is_sat_dev), from proofs a DeviceTrie leaves on the device.

Kernel forms: up to 8 192 traces in a call run T lanes per hash (every test below but one); more run one hash per lane
(test_both_kernel_forms_agree: 2 731 lookups at H = 3 are 8 193 traces, 2 731 inserts 16 386)."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import trie_circuit_ref as TC

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _ints(t):
    return C.limbs_to_ints(_host(t).reshape(-1, 4))


def _filled(n):
    import torch

    return torch.full((n, 4), FILL, dtype=torch.int64, device="cuda")


def _pairs(f, height, n, seed):
    p = R.modulus(f)
    return [(R.uniform_fe(seed, i, p), R.uniform_fe(seed + 1, i, p)) for i in range(n)]


def _keys16(f, height, pairs):
    """16 keys with distinct paths: present ones, absent ones, and ones that share all but the last digit (or, at H = 1, nothing) with a
    present key"""
    p = R.modulus(f)
    mask = (1 << (3 * height)) - 1
    keys, seen = [], set()

    def add(k):
        if k & mask not in seen and k < p:
            seen.add(k & mask)
            keys.append(k)

    add(pairs[0][0])                      # present
    add(R.uniform_fe(90, 0, p))           # absent
    add(pairs[1][0] ^ 1)                  # shares its prefix with a present key
    add(pairs[2][0])
    add(pairs[0][0] ^ 5)
    add(R.uniform_fe(90, 1, p))
    i = 2
    while len(keys) < 16:
        add(R.uniform_fe(90, i, p))
        i += 1
    return keys


@lru_cache(maxsize=None)
def _small(f, height=3, m=6):
    """(trie, keys, values, proofs on the device, the restatement's aux per insert block) - computed once per field and left unchanged"""
    from lurk_beta_amd.trie import DeviceTrie, _elems

    pairs = _pairs(f, height, 9, 40 + f)
    trie = DeviceTrie.build(f, pairs, height)
    keys = _keys16(f, height, pairs)
    p = R.modulus(f)
    values = [R.uniform_fe(91, i, p) for i in range(16)]
    dk, dv = _elems(keys), _elems(values)
    old, new, old_values, new_roots = trie.prove_insert(dk, dv)
    root = trie.root
    old_i = np.array(_ints(old), dtype=object).reshape(16, height, 8)
    want = []
    for i in range(m):
        cs, result, _ = TC.trie_circuit(f, height, TC.INSERT, root, keys[i], [list(x) for x in old_i[i]], values[i])
        assert cs.unsatisfied() == [] and cs.aux[result - 1] == _ints(new_roots)[i]
        want.append(list(cs.aux))
    return dict(trie=trie, root=root, keys=keys, values=values, dk=dk, dv=dv, old=old, new=new, new_roots=new_roots, want=want)


def _witness(f, height, op, s, sel, d_w, **place):
    from lurk_beta_amd.trie import _elems
    from lurk_beta_amd.trie_circuit import trie_circuit_witness

    ins = op == TC.INSERT
    trie_circuit_witness(f, height, op, _elems([s["root"]]), s["dk"][sel].contiguous(), s["old"][sel].contiguous(), d_w,
                         new_values=s["dv"][sel].contiguous() if ins else None, new_paths=s["new"][sel].contiguous() if ins else None, **place)


@pytest.mark.parametrize("f", [0, 1, 2])
def test_every_element_equals_the_restatement_at_height_3(hip, f):
    import torch

    from lurk_beta_amd.trie_circuit import trie_circuit_size

    H, m = 3, 6
    s = _small(f)
    sel = torch.arange(m, device="cuda")
    for op in (TC.LOOKUP, TC.INSERT):
        sz = trie_circuit_size(f, H, op)
        want = [w[:sz.size] for w in s["want"]]  # the lookup's allocations open the insert's
        # once through first / stride ...
        first, stride = 3, sz.size + 5
        d_w = _filled(first + m * stride + 7)
        _witness(f, H, op, s, sel, d_w, first=first, stride=stride)
        torch.cuda.synchronize()
        got = C.limbs_to_ints(C.from_mont(f, _host(d_w)))
        raw = _host(d_w)
        for i in range(m):
            at = first + i * stride
            assert got[at:at + sz.size] == want[i], (f, op, i, next(k for k in range(sz.size) if got[at + k] != want[i][k]))
            assert (raw[at + sz.size:at + stride] == FILL).all()  # between the blocks: as filled
        assert (raw[:first] == FILL).all() and (raw[first + m * stride:] == FILL).all()
        # ... and once through shuffled offsets
        order = [4, 0, 5, 2, 1, 3]
        offs = [2 + order[i] * (sz.size + 1) for i in range(m)]
        d_w = _filled(2 + m * (sz.size + 1) + 3)
        _witness(f, H, op, s, sel, d_w, offsets=torch.tensor(offs, dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        got = C.limbs_to_ints(C.from_mont(f, _host(d_w)))
        raw = _host(d_w)
        covered = np.zeros(len(raw), dtype=bool)
        for i in range(m):
            assert got[offs[i]:offs[i] + sz.size] == want[i], (f, op, i)
            covered[offs[i]:offs[i] + sz.size] = True
        assert (raw[~covered] == FILL).all()
        # the result column: the looked-up value / the new root
        for i in range(m):
            assert want[i][sz.result_col] == (_ints(s["new_roots"])[i] if op == TC.INSERT else _ints(s["old"])[(i * H + H - 1) * 8 + (s["keys"][i] & 7)])


@pytest.mark.parametrize("f", [0, 1, 2])
def test_both_kernel_forms_agree(hip, f):
    """8 193 (lookup) and 16 386 (insert) traces take the one-hash-per-lane form, the batch of 16 the T-lanes-per-hash form: block i of the
    large batch is block i mod 16 of the small one, whose first six blocks the test above pins.  Compared on the device."""
    import torch

    from lurk_beta_amd.trie_circuit import trie_circuit_size

    H, m = 3, 2731
    s = _small(f)
    for op in (TC.LOOKUP, TC.INSERT):
        sz = trie_circuit_size(f, H, op)
        small = _filled(16 * sz.size)
        _witness(f, H, op, s, torch.arange(16, device="cuda"), small, first=0, stride=sz.size)
        got6 = C.limbs_to_ints(C.from_mont(f, _host(small[:6 * sz.size])))
        assert got6 == [x for w in s["want"] for x in w[:sz.size]]
        big = _filled(m * sz.size)
        _witness(f, H, op, s, torch.arange(m, device="cuda") % 16, big, first=0, stride=sz.size)
        torch.cuda.synchronize()
        rep = small.view(16, sz.size, 4)[torch.arange(m, device="cuda") % 16].reshape(-1, 4)
        assert torch.equal(big, rep), (f, op)


@lru_cache(maxsize=None)
def _tall(f, m=3):
    from lurk_beta_amd.trie import DeviceTrie, _elems

    H = 85
    p = R.modulus(f)
    pairs = _pairs(f, H, 6, 60 + f)
    trie = DeviceTrie.build(f, pairs, H)
    keys = [pairs[1][0], R.uniform_fe(93, 0, p), pairs[4][0] ^ (1 << 200)]  # present, absent, sharing its top levels with a present key
    values = [R.uniform_fe(94, i, p) for i in range(m)]
    dk, dv = _elems(keys), _elems(values)
    old, new, old_values, new_roots = trie.prove_insert(dk, dv)
    return dict(trie=trie, root=trie.root, keys=keys, values=values, dk=dk, dv=dv, old=old, new=new, old_values=old_values, new_roots=new_roots)


def _z(f, sh, d_w):
    """z = [W | 1 | 0 .. 0]"""
    import torch

    tail = _dev(C.to_mont(f, C.ints_to_limbs([1] + [0] * sh.num_io)))
    return torch.cat([d_w, tail])


@pytest.mark.parametrize("op", [TC.LOOKUP, TC.INSERT])
@pytest.mark.parametrize("f", [2, 1])
def test_height_85_blocks_satisfy_the_librarys_rows(hip, f, op):
    import torch

    from lurk_beta_amd import slot_witness
    from lurk_beta_amd.trie_circuit import trie_circuit_shape, trie_circuit_size

    H, m = 85, 3
    s = _tall(f)
    sz = trie_circuit_size(f, H, op)
    first, stride = 11, sz.size + 2
    num_vars = first + m * stride
    sh = trie_circuit_shape(f, H, op, m, first, stride, num_vars, 2)
    assert sh.num_cons == m * sz.num_cons
    d_w = torch.zeros((num_vars, 4), dtype=torch.int64, device="cuda")
    _witness(f, H, op, s, torch.arange(m, device="cuda"), d_w, first=first, stride=stride)
    assert sh.is_sat(_z(f, sh, d_w)) == (0, sh.num_cons)
    w = _host(d_w)
    res = C.limbs_to_ints(C.from_mont(f, w[[first + i * stride + sz.result_col for i in range(m)]]))
    assert res == (_ints(s["new_roots"]) if op == TC.INSERT else _ints(s["old_values"]))
    if op == TC.LOOKUP:
        assert res[0] != 0 and res[1] == 0  # present, absent
    # every hash sub-block is lurk_hip_slot_witness of its path preimage
    b = TC.key_block_size(f)
    blocks = slot_witness(f, 8, _host(s["old"]).reshape(m * H, 8, 4)).reshape(m, H, 396, 4)
    for i in range(m):
        got = w[first + i * stride + 1 + b:first + i * stride + 1 + b + 403 * H].reshape(H, 403, 4)[:, :396]
        assert np.array_equal(got, blocks[i]), (f, op, i)
    if op == TC.INSERT:
        blocks = slot_witness(f, 8, _host(s["new"]).reshape(m * H, 8, 4)).reshape(m, H, 396, 4)[:, ::-1]  # allocated from the leaf upward
        lk = trie_circuit_size(f, H, TC.LOOKUP).size
        for i in range(m):
            at = first + i * stride + lk + 1
            assert np.array_equal(w[at:at + 396 * H].reshape(H, 396, 4), blocks[i]), (f, i)
    sh.close()


@pytest.mark.parametrize("k", [0, 57])
def test_a_wrong_proof_fails_at_its_level(hip, k):
    """one non-selected entry of path preimage k changed: the traces and the picks still hold, `hashed * 1 = next` of level k does not"""
    import torch

    from lurk_beta_amd.trie_circuit import trie_circuit_shape, trie_circuit_size

    f, H, m = 2, 85, 3
    s = dict(_tall(f))
    sz = trie_circuit_size(f, H, TC.LOOKUP)
    sh = trie_circuit_shape(f, H, TC.LOOKUP, m, 0, sz.size, m * sz.size, 2)
    digit = (s["keys"][0] >> (3 * (H - 1 - k))) & 7
    old = s["old"].clone()
    old[0, k, (digit + 1) % 8, 0] ^= 1
    s["old"] = old
    d_w = torch.zeros((m * sz.size, 4), dtype=torch.int64, device="cuda")
    _witness(f, H, TC.LOOKUP, s, torch.arange(m, device="cuda"), d_w, first=0, stride=sz.size)
    n_unsat, first_unsat = sh.is_sat(_z(f, sh, d_w))
    assert n_unsat >= 1 and first_unsat == TC.key_block_size(f) + 396 * k + 388
    sh.close()


def test_refusals_on_the_device(hip):
    from lurk_beta_amd import LurkHipError
    from lurk_beta_amd.trie_circuit import trie_circuit_shape, trie_circuit_size, trie_circuit_witness

    f, H = 1, 3
    s = _small(f)
    sz = trie_circuit_size(f, H, TC.INSERT)
    d_w = _filled(2 * sz.size)
    args = (s["dk"][:2].contiguous(), s["old"][:2].contiguous(), d_w)
    root = s["dk"][:1]
    for kw, word in ((dict(new_values=s["dv"][:2].contiguous()), "NULL"), (dict(stride=sz.size - 1, new_values=s["dv"][:2].contiguous(), new_paths=s["new"][:2].contiguous()), "stride")):
        op = TC.LOOKUP if word == "NULL" else TC.INSERT
        with pytest.raises(LurkHipError, match=word):
            trie_circuit_witness(f, H, op, root, *args, **kw)
    with pytest.raises(LurkHipError, match="null buffer"):
        trie_circuit_witness(f, H, TC.INSERT, root, *args, stride=sz.size)
    assert (_host(d_w) == FILL).all()
    assert hip.lurk_hip_trie_circuit_witness_dev(f, H, 0, None, 0, None, None, None, None, (1 << 28) + 1, None, None, 0, 0, None) != 0 and b"2^28" in hip.lurk_hip_last_error()
    assert hip.lurk_hip_trie_circuit_witness_dev(*[0] * 3, None, 0, None, None, None, None, 0, None, None, 0, 0, None) != 0 and hip.lurk_hip_last_error() != b""
    assert hip.lurk_hip_trie_circuit_r1cs_create(None, *[0] * 9, *[None] * 9) != 0 and hip.lurk_hip_last_error() != b""
    with pytest.raises(LurkHipError, match="past num_vars"):
        trie_circuit_shape(f, H, TC.INSERT, 2, 1, sz.size, 2 * sz.size, 2)
    with pytest.raises(LurkHipError, match="stride"):
        trie_circuit_shape(f, H, TC.INSERT, 2, 0, sz.size - 1, 2 * sz.size, 2)


def test_a_chain_of_inserts_folds_step_by_step(hip):
    """The step: an insert circuit at H = 3 on Pallas with two public values tied to the root column and the result column, four DEPENDENT
    inserts from insert_chain_dev (a repeated key among them), their four witnesses from ONE witness call, folded one after the other."""
    import torch

    from lurk_beta_amd import CommitmentKey, FoldingContext
    from lurk_beta_amd.trie import DeviceTrie, _elems
    from lurk_beta_amd.trie_circuit import trie_circuit_shape, trie_circuit_size, trie_circuit_witness

    f, curve, H, m, nio = 1, 0, 3, 4, 2
    p = R.modulus(f)
    sz = trie_circuit_size(f, H, TC.INSERT)
    first = 2
    num_vars = first + sz.size + 3
    one = C.to_mont(f, C.ints_to_limbs([1]))
    csr = lambda cols: (np.array([0] + list(np.cumsum([len(c) for c in cols])), dtype=np.uint64), np.array([x for c in cols for x in c], dtype=np.uint64),
                        np.repeat(one, sum(len(c) for c in cols), axis=0).reshape(-1, 4))
    # X0 * ONE = root, X1 * ONE = result
    extra = (csr([[num_vars + 1], [num_vars + 2]]), csr([[num_vars], [num_vars]]), csr([[first], [first + sz.result_col]]))
    sh = trie_circuit_shape(f, H, TC.INSERT, 1, first, 0, num_vars, nio, extra=extra)
    n = sh.num_cons
    assert n == sz.num_cons + 2

    trie = DeviceTrie.build(f, _pairs(f, H, 5, 80), H)
    a, b, c = (R.uniform_fe(95, i, p) for i in range(3))
    keys = [a, b, a, (c & ~0x1C0) | (a & 0x1C0)]  # a repeated key, and one that shares a's top digit
    values = [R.uniform_fe(96, i, p) for i in range(m)]
    dk, dv = _elems(keys), _elems(values)
    old, new, old_values, roots, grown = trie.insert_chain(dk, dv)
    roots_in = torch.cat([_elems([trie.root]), roots[:m - 1]])  # block i opens on the root of T_i
    d_w = torch.zeros((m, num_vars, 4), dtype=torch.int64, device="cuda")
    trie_circuit_witness(f, H, TC.INSERT, roots_in, dk, old, d_w, new_values=dv, new_paths=new, first=first, stride=num_vars)
    torch.cuda.synchronize()
    xs = [torch.stack([d_w[i, first], d_w[i, first + sz.result_col]]) for i in range(m)]
    assert C.limbs_to_ints(C.from_mont(f, _host(xs[0][0]).reshape(1, 4))) == [trie.root]
    assert C.limbs_to_ints(C.from_mont(f, _host(xs[m - 1][1]).reshape(1, 4))) == [grown.root]
    for i in range(m - 1):
        assert torch.equal(xs[i][1], xs[i + 1][0])  # X1 of step i is X0 of step i + 1

    key = CommitmentKey(curve, C.synth_bases(curve, max(n, num_vars)))
    ctx = FoldingContext(curve, sh, key)
    for i in range(m):
        z2 = torch.cat([d_w[i], _dev(one), xs[i]])
        assert sh.is_sat(z2) == (0, n)
        ctx.begin(d_w[i], _host(xs[i]), stream=torch.cuda.current_stream().cuda_stream)
        ctx.finish(C.to_mont(f, C.ints_to_limbs([R.uniform_fe(97, i, p) >> 128])))
        z_ptr, e_ptr, stream = ctx.running_device()
        n_unsat, first_unsat = ctypes.c_uint64(), ctypes.c_uint64()
        assert hip.lurk_hip_r1cs_is_sat_dev(sh._h, ctypes.c_void_p(z_ptr), ctypes.c_void_p(e_ptr), ctypes.byref(n_unsat), ctypes.byref(first_unsat),
                                            ctypes.c_void_p(stream)) == 0, hip.lurk_hip_last_error()
        assert (n_unsat.value, first_unsat.value) == (0, n), i
    ctx.close()
    key.close()
    sh.close()
    grown.close()
    trie.close()
