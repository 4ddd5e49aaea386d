"""CPU-only: the Python restatement of the reference's trie (tests/trie_ref.py) against the golden vectors and the oracle, its two
verifiers on honest and tampered proofs, and the library's host-only path function."""
import random

import numpy as np
import pytest

from oracle import pyref as R
from tests import kat
from tests import trie_ref as T

BN = kat.BN


def test_helper_reproduces_the_golden_vectors():
    assert T.path(BN, 500, 3) == kat.GOLDEN["trie_path_500_h3"]
    t = T.RefTrie(BN, 85)
    assert t.root == kat.golden_int("empty_root_85")
    assert t.lookup(123) is None
    assert t.insert(123, 456) is True
    assert t.root == kat.golden_int("trie_insert_123_456")
    assert t.lookup(123) == 456 and t.lookup(124) is None


def test_helper_hash_is_the_oracle_hash():
    t = T.RefTrie(1, 3)
    t.insert(5, 77)
    nodes = [t.children[t.root], t.children[t.empty_roots[0]], (1, 2, 3, 4, 5, 6, 7, R.modulus(1) - 1)]
    for pre in nodes:
        assert T.hash8(1, pre) == R.poseidon_hash(1, list(pre))
    assert t.root == R.trie_insert_root(1, 3, 5, 77)


def test_path_matches_pyref():
    rng = random.Random(5)
    for f in (0, 1, 2):
        for h in (1, 3, 85):
            for key in (0, 1, 500, R.modulus(f) - 1, rng.randrange(R.modulus(f))):
                assert T.path(f, key, h) == R.trie_path(f, key, h)


def test_insertion_order_does_not_change_the_root():
    rng = random.Random(11)
    pairs = [(rng.randrange(R.modulus(BN)), rng.randrange(1, R.modulus(BN))) for _ in range(12)]
    roots = set()
    for seed in range(3):
        order = list(pairs)
        random.Random(seed).shuffle(order)
        t = T.RefTrie(BN, 5)
        for k, v in order:
            t.insert(k, v)
        roots.add(t.root)
        assert all(t.lookup(k) == v for k, v in dict((k & (8 ** 5 - 1), (k, v)) for k, v in order).values())
    assert len(roots) == 1


def _bump(path, level, pos):
    out = [list(p) for p in path]
    out[level][pos] = (out[level][pos] + 1) % R.modulus(BN)
    return [tuple(p) for p in out]


def test_lookup_verifier_accepts_honest_and_rejects_each_tamper():
    H = 5
    t = T.RefTrie(BN, H)
    for k, v in ((3, 30), (3 + 8, 31), (9000, 32), (20000, 33)):
        t.insert(k, v)
    for key, value in ((3, 30), (9000, 32), (4, 0), (31000, 0)):  # present and absent
        proof = t.prove_lookup(key)
        assert T.verify_lookup(BN, H, t.root, key, value, proof) == 0
        digits = t.path(key)
        for k in (0, H // 2, H - 1):
            off = (digits[k] + 1) % 8
            assert T.verify_lookup(BN, H, t.root, key, value, _bump(proof, k, off)) == k + 1
            assert T.verify_lookup(BN, H, t.root, key, value, _bump(proof, k, digits[k])) == k + 1  # the hash of preimage k moved too
        assert T.verify_lookup(BN, H, t.root, key, value + 1, proof) == H + 1
        assert T.verify_lookup(BN, H, t.root + 1, key, value, proof) == 1


def test_insert_verifier_accepts_honest_and_rejects_each_tamper():
    H = 5
    base = T.RefTrie(BN, H)
    for k, v in ((3, 30), (3 + 8, 31), (9000, 32)):
        base.insert(k, v)
    results = {}
    for key, old_value, new_value in ((4, None, 44), (3, 30, 55), (20000, None, 66)):  # fresh, existing, fresh
        t = base.copy()
        old, new, inserted = t.prove_insert(key, new_value)
        assert inserted
        results[key] = t.root
        assert T.verify_insert(BN, H, base.root, t.root, key, old_value, new_value, old, new) == 0
        digits = base.path(key)
        for k in (0, H // 2, H - 1):
            off = (digits[k] + 1) % 8
            assert T.verify_insert(BN, H, base.root, t.root, key, old_value, new_value, old, _bump(new, k, off)) == 0x100 + k + 1
            assert T.verify_insert(BN, H, base.root, t.root, key, old_value, new_value, _bump(old, k, off), new) == k + 1
        assert T.verify_insert(BN, H, base.root, t.root, key, (old_value or 0) + 1, new_value, old, new) == H + 1
        assert T.verify_insert(BN, H, base.root, t.root, key, old_value, new_value + 1, old, new) == 0x200 + H + 1
    assert T.verify_insert(BN, H, base.root, results[3], 4, None, 44, *base.copy().prove_insert(4, 44)[:2]) == 0x201  # another key's new root


def test_library_path_digits_match_pyref():
    """lurk_hip_trie_path_digits is host code: the same digits as the oracle's trie_path on every field, at the extremes of the key range."""
    from lurk_beta_amd import LurkHipError
    from lurk_beta_amd import trie as LT

    for f in (0, 1, 2):
        for h in (1, 3, 85):
            keys = [0, 1, 500, R.modulus(f) - 1, (1 << (3 * h)) - 1]
            got = LT.path_digits(f, h, keys)
            assert got.shape == (len(keys), h) and got.dtype == np.uint8
            for row, key in zip(got, keys):
                assert list(row) == R.trie_path(f, key, h), (f, h, hex(key))
    with pytest.raises(LurkHipError, match="unknown field id"):
        LT.path_digits(3, 3, [1])
    for h in (0, 86):
        with pytest.raises(LurkHipError, match="height"):
            LT.path_digits(2, h, [1])
