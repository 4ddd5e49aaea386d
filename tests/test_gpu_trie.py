"""GPU: the device-resident trie (lurk_hip_trie_*, lurk_beta_amd.trie.DeviceTrie) against the Python restatement of the reference
(tests/trie_ref.py): roots after sequential inserts, refusals, lookup and insert proofs element for element, the verifiers' codes on honest
and tampered proofs, and two streams on one handle."""
import functools
import random

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import kat
from tests import trie_ref as T

pytestmark = pytest.mark.gpu

BN = kat.BN


def _with_digit(key: int, height: int, d: int, digit: int, low: int = 0) -> int:
    """key with digit d replaced and everything below it set to the low bits of `low`"""
    sh = 3 * (height - 1 - d)
    return (key >> (sh + 3) << (sh + 3)) | (digit << sh) | (low & ((1 << sh) - 1))


def _key0(height: int) -> int:
    return 0x0123456789ABCDEFFEDCBA98765432100F1E2D3C4B5A69788796A5B4C3D2E1 & ((1 << (3 * height - 3)) - 1)  # top digit 0


@functools.lru_cache(maxsize=None)
def key_set(field_id: int, height: int, n: int):
    """n (key, value) pairs in insertion order (shuffled).  Between them the sets hold: eight keys filling one leaf node and a ninth that
    diverges from them at depth 0 (n = 9); keys 0 and p - 1 (n = 2, n = 200); a chain in which key j shares exactly j digits with key 0, the
    last of them diverging only at the last digit, which makes the build run one launch for every depth (n = 200); a value of 0 (n >= 9).
    Every key of the n = 200 set but p - 1 has top digit 0."""
    p = R.modulus(field_id)
    rng = random.Random(1000 * height + n + field_id)
    k0 = _key0(height)
    if n == 0:
        pairs = []
    elif n == 1:
        pairs = [(123, 456)]
    elif n == 2:
        pairs = [(0, 7), (p - 1, 9)]
    elif n == 9:
        leaf = [(_with_digit(k0, height, height - 1, c), 100 + c) for c in range(8)]
        leaf[3] = (leaf[3][0], 0)
        pairs = leaf + [(_with_digit(k0, height, 0, 2, rng.getrandbits(255)), 5)]
    else:
        keys = [k0] + [_with_digit(k0, height, j, (((k0 >> (3 * (height - 1 - j))) & 7) + 1) % 8, rng.getrandbits(255)) for j in range(1, height)]
        keys += [0, p - 1]
        while len(keys) < n:
            keys.append(rng.getrandbits(255) & ((1 << (3 * height - 3)) - 1))
        pairs = [(k, rng.randrange(1, p)) for k in keys[:n]]
        pairs[5 % len(pairs)] = (pairs[5 % len(pairs)][0], 0)
    assert all(k < p for k, _ in pairs)
    rng.shuffle(pairs)
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def ref_trie(field_id: int, height: int, n: int) -> T.RefTrie:
    """the reference after sequential inserts; shared by the tests and never modified (copy() before inserting)"""
    t = T.RefTrie(field_id, height)
    for k, v in key_set(field_id, height, n):
        t.insert(k, v)
    return t


def _build(field_id, height, n):
    from lurk_beta_amd.trie import DeviceTrie

    return DeviceTrie.build(field_id, key_set(field_id, height, n), height)


def _ints(t) -> list[int]:
    return C.limbs_to_ints(t.cpu().numpy().view(np.uint64))


def _paths_np(paths) -> np.ndarray:
    """a list of proofs (H preimages of 8 ints) -> (m, H, 8, 4) uint64"""
    flat = [x for proof in paths for pre in proof for x in pre]
    return C.ints_to_limbs(flat).reshape(len(paths), -1, 8, 4)


@pytest.mark.parametrize("n", [0, 1, 2, 9, 200])
@pytest.mark.parametrize("height", [1, 3, 5, 85])
def test_root_equals_sequential_inserts(hip, height, n):
    with _build(BN, height, n) as t:
        assert t.root == ref_trie(BN, height, n).root
        if height == 85 and n == 1:
            assert t.root == kat.golden_int("trie_insert_123_456")
        if height == 85 and n == 0:
            assert t.root == kat.golden_int("empty_root_85")


@pytest.mark.parametrize("field_id", [0, 1])
def test_root_on_the_pasta_fields(hip, field_id):
    for height, n in ((5, 9), (3, 200)):
        with _build(field_id, height, n) as t:
            assert t.root == ref_trie(field_id, height, n).root


def test_the_chain_set_shares_every_depth():
    """the n = 200 set is what it is meant to be: key j of the chain shares exactly j digits with key 0"""
    H = 85
    keys = {k for k, _ in key_set(BN, H, 200)}
    k0 = _key0(H)
    d0 = T.path(BN, k0, H)
    shared = set()
    for k in keys - {k0}:
        d = T.path(BN, k, H)
        shared.add(next(i for i in range(H) if d[i] != d0[i]))
    assert shared >= set(range(H))


def test_build_refusals_name_index_and_kind(hip):
    from lurk_beta_amd import LurkHipError
    from lurk_beta_amd.trie import DeviceTrie

    H, p = 3, R.modulus(BN)
    with pytest.raises(LurkHipError, match=r"key 2 is out of order") as e:
        DeviceTrie.build_sorted(BN, [1, 5, 3, 7], [1, 1, 1, 1], H)
    assert e.value.code == 2
    with pytest.raises(LurkHipError, match=r"key 1 has a duplicate path"):
        DeviceTrie.build_sorted(BN, [1, 1 + (1 << (3 * H)), 2], [1, 1, 1], H)  # equal below bit 3 H, different above
    with pytest.raises(LurkHipError, match=r"key 2 is not reduced"):
        DeviceTrie.build_sorted(BN, [1, 2, p + 3], [1, 1, 1], H)
    with pytest.raises(LurkHipError, match=r"key 0 is not reduced"):
        DeviceTrie.build_sorted(BN, [p], [1], H)
    for h in (0, 86):
        with pytest.raises(LurkHipError, match="height"):
            DeviceTrie.build_sorted(BN, [1], [1], h)
    with pytest.raises(LurkHipError, match="unknown field id"):
        DeviceTrie.build_sorted(3, [1], [1], H)
    # a following valid build on the same stream succeeds
    ref = T.RefTrie(BN, H)
    for k in (1, 3, 5, 7):
        ref.insert(k, k + 10)
    with DeviceTrie.build_sorted(BN, [1, 3, 5, 7], [11, 13, 15, 17], H) as t:
        assert t.root == ref.root
    # DeviceTrie.build: of two pairs with one path the last stays, as sequential inserts leave it
    ref = T.RefTrie(BN, H)
    pairs = [(1, 10), (6, 5), (1 + (1 << (3 * H)), 20)]
    for k, v in pairs:
        ref.insert(k, v)
    with DeviceTrie.build(BN, pairs, H) as t:
        assert t.root == ref.root and t.n == 2


def _lookup_queries(field_id, height, n):
    """present keys, and absent ones whose path leaves the populated trie at depth 0, in between and at depth H - 1"""
    pairs = key_set(field_id, height, n)
    present = [k for k, _ in pairs[:6]] + [_key0(height)]
    k0 = _key0(height)
    used_last = {T.path(field_id, k, height)[-1] for k, _ in pairs if k >> 3 == k0 >> 3}
    free_last = next((c for c in range(8) if c not in used_last), None)
    if free_last is not None:
        deep = _with_digit(k0, height, height - 1, free_last)
    else:  # the leaf node is full (n = 9): leave one level above it
        deep = _with_digit(k0, height, height - 2, ((k0 >> 3) & 7) ^ 1, 3)
    absent = [_with_digit(k0, height, 0, 1, 12345), deep]
    if height > 2:
        d = height // 2
        used = {T.path(field_id, k, height)[d] for k, _ in pairs if k >> (3 * (height - d)) == k0 >> (3 * (height - d))}
        free = next((c for c in range(8) if c not in used), None)
        if free is not None:
            absent.append(_with_digit(k0, height, d, free, 999))
    return present, absent


@pytest.mark.parametrize("field_id,height,n", [(BN, 85, 200), (BN, 5, 9), (0, 5, 9), (1, 5, 200), (BN, 1, 2), (BN, 3, 0)])
def test_lookup_proofs_equal_the_reference(hip, field_id, height, n):
    ref = ref_trie(field_id, height, n)
    if n:
        present, absent = _lookup_queries(field_id, height, n)
    else:
        present, absent = [], [0, 5, 300]
    if height == 85 and n == 200:  # the walk leaves the populated part at depth 0, not at all (the leaf node exists), and in between
        assert [sum(1 for pre in ref.prove_lookup(k) if len(set(pre)) > 1) for k in absent] == [1, 85, 85 // 2 + 1]
    keys = present + absent
    with _build(field_id, height, n) as t:
        paths, values = t.prove_lookup(keys)
        want_values = [ref.lookup(k) or 0 for k in keys]
        assert _ints(values) == want_values
        assert all(v == 0 for v in want_values[len(present):])
        assert np.array_equal(paths.cpu().numpy().view(np.uint64), _paths_np([ref.prove_lookup(k) for k in keys]))
        codes, failed = t.verify_lookup(keys, values, paths)
        assert failed == 0 and not codes.any()


def test_lookup_tampering_codes(hip):
    H, n = 85, 200
    ref = ref_trie(BN, H, n)
    p = R.modulus(BN)
    key, value = next((k, v) for k, v in key_set(BN, H, n) if v)
    digits = ref.path(key)
    honest = ref.prove_lookup(key)

    def bump(level, pos):
        out = [list(x) for x in honest]
        out[level][pos] = (out[level][pos] + 1) % p
        return [tuple(x) for x in out]

    cases = [(ref.root, value, honest, 0)]
    for k in (0, H // 2, H - 1):
        cases.append((ref.root, value, bump(k, (digits[k] + 1) % 8), k + 1))  # off the path
        cases.append((ref.root, value, bump(k, digits[k]), None))             # on the path: the helper decides, k + 1 or k + 2
    cases.append((ref.root, (value + 1) % p, honest, H + 1))
    cases.append(((ref.root + 1) % p, value, honest, 1))
    from lurk_beta_amd.trie import verify_lookup_batch

    want = [T.verify_lookup(BN, H, r, key, v, pth) for r, v, pth, _ in cases]
    for (r, v, pth, fixed), w in zip(cases, want):
        assert fixed is None or w == fixed
    on_path = [w for (_, _, _, fixed), w in zip(cases, want) if fixed is None]
    assert all(w in (k + 1, k + 2) for w, k in zip(on_path, (0, H // 2, H - 1)))
    codes, failed = verify_lookup_batch(BN, H, [r for r, _, _, _ in cases], [key] * len(cases), [v for _, v, _, _ in cases], _paths_np([pth for _, _, pth, _ in cases]))
    assert list(codes) == want and failed == sum(1 for w in want if w)
    # a batch of 130 (two full waves and a partial one): n_failed counts exactly the tampered proofs
    m, bad = 130, {0, 63, 64, 127, 128, 129}
    batch = _paths_np([bump(H - 1, (digits[H - 1] + 1) % 8) if i in bad else honest for i in range(m)])
    codes, failed = verify_lookup_batch(BN, H, [ref.root], [key] * m, [value] * m, batch)
    assert failed == len(bad) and {i for i in range(m) if codes[i]} == bad and all(codes[i] == H for i in bad)
    # keys and values that are not reduced are refused
    from lurk_beta_amd import LurkHipError

    with pytest.raises(LurkHipError, match="key 1 is not reduced"):
        verify_lookup_batch(BN, H, [ref.root], [key, p + 1], [value, value], batch[:2])
    with pytest.raises(LurkHipError, match="value 0 is not reduced"):
        verify_lookup_batch(BN, H, [ref.root], [key, key], [p, value], batch[:2])


@pytest.mark.parametrize("field_id,height,n", [(BN, 85, 200), (0, 5, 9), (1, 5, 9)])
def test_insert_proofs_equal_the_reference(hip, field_id, height, n):
    from lurk_beta_amd.trie import verify_insert_batch

    ref = ref_trie(field_id, height, n)
    p = R.modulus(field_id)
    present, absent = _lookup_queries(field_id, height, n)
    keys = absent + present[:3]  # fresh keys, and existing keys with new values
    new_values = [1000 + i for i in range(len(keys))]
    want = []
    for k, v in zip(keys, new_values):
        t = ref.copy()
        old, new, _ = t.prove_insert(k, v)
        want.append((old, new, t.root))
    with _build(field_id, height, n) as t:
        old_paths, new_paths, old_values, new_roots = t.prove_insert(keys, new_values)
        assert t.root == ref.root  # the handle is not modified
        assert np.array_equal(old_paths.cpu().numpy().view(np.uint64), _paths_np([w[0] for w in want]))
        assert np.array_equal(new_paths.cpu().numpy().view(np.uint64), _paths_np([w[1] for w in want]))
        assert _ints(new_roots) == [w[2] for w in want]
        assert _ints(old_values) == [ref.lookup(k) or 0 for k in keys]
        codes, failed = t.verify_insert(keys, old_values, new_values, old_paths, new_paths, new_roots)
        assert failed == 0 and not codes.any()
        # a new path that differs from the old in two positions at level k; a new root that belongs to another key
        key, (old, new, root) = keys[0], want[0]
        digits = ref.path(key)
        cases = []
        for k in (0, height // 2, height - 1):
            bad = [list(x) for x in new]
            off = (digits[k] + 1) % 8
            bad[k][off] = (bad[k][off] + 1) % p
            cases.append((old, [tuple(x) for x in bad], root, 0x100 + k + 1))
        cases.append((old, new, want[1][2], 0x201))
        cases.append((old, new, root, 0))
        m = len(cases)
        codes, failed = verify_insert_batch(field_id, height, [ref.root] * m, [c[2] for c in cases], [key] * m, [0] * m, [new_values[0]] * m,
                                            _paths_np([c[0] for c in cases]), _paths_np([c[1] for c in cases]))
        assert list(codes) == [c[3] for c in cases] and failed == m - 1
        assert list(codes) == [T.verify_insert(field_id, height, ref.root, c[2], key, None, new_values[0], c[0], c[1]) for c in cases]


def test_two_streams_one_handle(hip):
    import torch

    from lurk_beta_amd.trie import _elems

    H, n = 85, 200
    present, absent = _lookup_queries(BN, H, n)
    a, b = _elems((present + absent) * 8), _elems((absent + present) * 8)
    with _build(BN, H, n) as t:
        alone = [t.prove_lookup(a), t.prove_lookup(b)]
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        both = [t.prove_lookup(a, stream=s1.cuda_stream), t.prove_lookup(b, stream=s2.cuda_stream)]
        s1.synchronize()
        s2.synchronize()
        for (p0, v0), (p1, v1) in zip(alone, both):
            assert torch.equal(p0, p1) and torch.equal(v0, v1)
