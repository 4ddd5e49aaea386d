"""CPU-only: the level-synchronous statement of a chain of dependent trie inserts (tests/trie_chain_ref.py) equals the reference's
sequential inserts (tests/trie_ref.py: RefTrie.prove_insert one after the other) - every old preimage, new preimage, old value and root
- and the new entry point is declared, bound with the header's arity and added under the unchanged ABI revision."""
import hashlib
import os
import random
import re

import pytest

from oracle import pyref as R
from tests import kat
from tests import trie_chain_ref as CH
from tests import trie_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN = kat.BN


@pytest.mark.parametrize("height", [1, 2, 3, 5])
@pytest.mark.parametrize("populated", [False, True])
def test_level_synchronous_chain_equals_sequential_inserts(height, populated):
    pairs = CH.base_pairs(BN, height, populated)
    base = CH.base_trie(BN, height, pairs)
    root0 = base.root
    for name, updates in CH.families(BN, height, pairs):
        assert 0 < len(updates) <= 200
        want = CH.sequential(base, updates)
        for short in (False, True):
            assert CH.level_synchronous(base, updates, short=short) == want, (name, short)
    assert base.root == root0  # the checker works on copies


@pytest.mark.parametrize("field_id", [0, 1])
def test_the_other_fields(field_id):
    pairs = CH.base_pairs(field_id, 3, True)
    base = CH.base_trie(field_id, 3, pairs)
    for name, updates in CH.families(field_id, 3, pairs):
        assert CH.level_synchronous(base, updates, short=True) == CH.sequential(base, updates), name


def test_random_chains_with_a_stand_in_hash():
    """300 random chains, the hash replaced by SHA-256 in both the checker and the formulation (the statement is about which entries a
    preimage holds, not about Poseidon; a LINEAR stand-in will not do: the checker's child map is addressed by hash, and a node with one
    leaf hash in one position then collides with its mirror image): repeated keys, a key pool, values of 0, empty and populated bases."""
    p = R.modulus(BN)

    def fake(pre):
        return int.from_bytes(hashlib.sha256(b"".join(int(x).to_bytes(32, "little") for x in pre)).digest(), "little") % p

    class FakeTrie(T.RefTrie):
        def register_hash(self, preimage):
            h = fake(preimage)
            self.children[h] = tuple(preimage)
            return h

        def copy(self):
            t = object.__new__(FakeTrie)
            t.field_id, t.height, t.children, t.empty_roots, t.root = self.field_id, self.height, dict(self.children), self.empty_roots, self.root
            return t

    rng = random.Random(2024)
    for case in range(300):
        height = (1, 2, 3, 5)[case % 4]
        base = FakeTrie(BN, height)
        space = rng.choice([4, 8, 8 ** height])
        for _ in range(rng.choice([0, 0, 3, 12])):
            base.insert(rng.randrange(space), rng.randrange(1, p))
        pool = [rng.randrange(space) for _ in range(rng.choice([1, 2, 5, 40]))]
        updates = [(rng.choice(pool), rng.choice([0, 7, rng.randrange(p)])) for _ in range(rng.randrange(1, 60))]
        want = CH.sequential(base, updates)
        for short in (False, True):
            assert CH.level_synchronous(base, updates, short=short, hash8=fake) == want, (case, short)


def test_final_pairs_are_the_pairs_of_the_last_trie():
    pairs = CH.base_pairs(BN, 3, True)
    base = CH.base_trie(BN, 3, pairs)
    for name, updates in CH.families(BN, 3, pairs):
        final = CH.final_pairs(pairs, updates, 3)
        assert [k & 511 for k, _ in final] == sorted({k & 511 for k, _ in final})
        assert CH.base_trie(BN, 3, final).root == CH.sequential(base, updates)[3][-1], name


def test_the_entry_point_is_declared_and_bound_under_abi_4():
    from lurk_beta_amd import _lib
    from lurk_beta_amd.trie import DeviceTrie

    hdr = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    assert re.search(r"^#define LURK_HIP_ABI_VERSION 4$", hdr, flags=re.M)  # an addition
    decl = re.search(r"\bint\s+lurk_hip_trie_insert_chain_dev\s*\(([^)]*)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert decl, "include/lurk_hip.h does not declare lurk_hip_trie_insert_chain_dev"
    params = [a.strip() for a in decl.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in params] == ["t", "d_keys32", "d_values32", "m", "d_old_paths", "d_new_paths", "d_old_values32", "d_roots32",
                                                           "out_trie", "stream"]
    restype, argtypes = _lib.SIGNATURES["lurk_hip_trie_insert_chain_dev"]
    assert len(argtypes) == len(params) == 10
    lib = _lib.load()
    assert hasattr(lib, "lurk_hip_trie_insert_chain_dev") and lib.lurk_hip_abi_version() == 4
    assert callable(DeviceTrie.insert_chain)
