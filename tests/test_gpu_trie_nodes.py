"""GPU: root-addressed tries - the trie's child map resident on the device (lurk_hip_trie_nodes_*, DeviceTrieNodes) against the reference's
map (tests/trie_ref.py: RefTrie.children is InversePoseidonCache::a8, setting RefTrie.root is Trie::new_with_root) and against the
handle-based trie calls, byte for byte.  Everything is bit-exact; every count is exact."""
import ctypes
import functools
import random

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyref as R
from tests import kat
from tests import trie_chain_ref as CH
from tests import trie_ref as T

pytestmark = pytest.mark.gpu

BN = kat.BN
SHAPES = [(BN, 1), (BN, 2), (BN, 3), (BN, 85), (0, 2), (0, 85), (1, 2), (1, 85)]


def _u64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _ints(t) -> list[int]:
    return C.limbs_to_ints(_u64(t).reshape(-1, 4))


def _paths_np(paths, height) -> np.ndarray:
    flat = [x for proof in paths for pre in proof for x in pre]
    return C.ints_to_limbs(flat).reshape(len(paths), height, 8, 4)


def _pre_np(pres) -> np.ndarray:
    return C.ints_to_limbs([x for pre in pres for x in pre]).reshape(len(pres), 8, 4)


def _from_digits(digits) -> int:
    v = 0
    for d in digits:
        v = v * 8 + d
    return v


def _pairs(field_id: int, height: int, n: int, seed: int = 0):
    """min(n, 8^height) pairs with distinct path values (a trie of height 1 has 8 leaves, one of height 2 has 64).  The first keys share
    0, 1, H - 2 and H - 1 (all but the last) digits with key 0; one value in five is 0.  The top digit stays below 3, so that at H = 85 every path
    value is below every modulus."""
    rng = random.Random(1009 * seed + 17 * height + field_id)
    p = R.modulus(field_id)
    top = 3 if height == 85 else 8
    a = [rng.randrange(top)] + [rng.randrange(8) for _ in range(height - 1)]
    variants = [a]
    for pos in (0, 1, height - 2, height - 1):
        if 0 <= pos < height:
            b = list(a)
            b[pos] = (b[pos] + 1) % (top if pos == 0 else 8)
            variants.append(b)
    pvs = []
    for d in variants:
        if _from_digits(d) not in pvs:
            pvs.append(_from_digits(d))
    n = min(n, 8 ** height)
    while len(pvs) < n:
        pv = _from_digits([rng.randrange(top)] + [rng.randrange(8) for _ in range(height - 1)])
        if pv not in pvs:
            pvs.append(pv)
    pairs = [(pv, 0 if i % 5 == 3 else rng.randrange(1, p)) for i, pv in enumerate(pvs[:n])]
    assert all(k < p for k, _ in pairs)
    return pairs


def _absent_keys(field_id, height, pairs, count, seed=5):
    rng = random.Random(seed)
    have = {k for k, _ in pairs}
    top = 3 if height == 85 else 8
    out = []
    while len(out) < count and len(have) + len(out) < 8 ** height:
        pv = _from_digits([rng.randrange(top)] + [rng.randrange(8) for _ in range(height - 1)])
        if pv not in have and pv not in out:
            out.append(pv)
    return out


def _twin(field_id, height, key):
    """another key with the same path value (carry bits above the path), or None where the field has no room for one"""
    k = key + (5 << (3 * height))
    return k if 3 * height < 200 and k < R.modulus(field_id) else None


def _ref_with(field_id, height, pairs) -> T.RefTrie:
    t = T.RefTrie(field_id, height)
    for k, v in pairs:
        t.insert(k, v)
    return t


def _reachable(ref: T.RefTrie, root: int) -> set:
    """the digests of the nodes of the trie named by root"""
    seen, level = set(), {root}
    for _ in range(ref.height):
        seen |= level
        level = {c for node in level for c in ref.children[node]}
    return seen


def _assert_store_holds(ns, ref: T.RefTrie, digests):
    digests = sorted(digests)
    pre, found = ns.get(digests)
    assert found.cpu().numpy().all()
    assert np.array_equal(_u64(pre), _pre_np([ref.children[d] for d in digests]))


def _lookup_all(ns, ref: T.RefTrie, roots, keys):
    """one root-addressed lookup per (root, key), against new_with_root + prove_lookup of the reference; returns the device outputs"""
    assert len(roots) == len(keys)
    paths, values, status, missing = ns.prove_lookup(roots, keys)
    want_paths, want_values = [], []
    for r, k in zip(roots, keys):
        v = ref.copy()
        v.root = r
        proof = v.prove_lookup(k)
        want_paths.append(proof)
        want_values.append(proof[-1][v.path(k)[-1]])
    assert missing == 0 and not status.cpu().numpy().any()
    assert _ints(values) == want_values
    assert np.array_equal(_u64(paths), _paths_np(want_paths, ref.height))
    return paths, values


# ---- 1. a fresh store ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id,height", SHAPES)
def test_fresh_store_holds_the_empty_chain(hip, field_id, height):
    from lurk_beta_amd.trie import DeviceTrieNodes

    ref = T.RefTrie(field_id, height)
    keys = [0, 1, 7, 8] + [k for k, _ in _pairs(field_id, height, 6)]
    with DeviceTrieNodes.create(field_id, height) as ns:
        info = ns.info()
        assert info["n_nodes"] == height and info["field_id"] == field_id and info["height"] == height
        assert info["slots"] >= 2 * height and info["slots"] & (info["slots"] - 1) == 0
        _, values = _lookup_all(ns, ref, [ref.root] * len(keys), keys)
        assert not _u64(values).any()
        pre, found = ns.get(ref.empty_roots)
        assert found.cpu().numpy().tolist() == [1] * height
        below = [0] + ref.empty_roots[:-1]
        assert np.array_equal(_u64(pre), _pre_np([[b] * 8 for b in below]))
        assert ns.n_nodes == height  # reads do not register


# ---- 2. add_trie -----------------------------------------------------------------------------------------------------------------------
def _check_add_trie(field_id, height, n):
    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes

    pairs = _pairs(field_id, height, n)
    ref = _ref_with(field_id, height, pairs)
    want = _reachable(ref, ref.root) | set(ref.empty_roots)
    with DeviceTrie.build(field_id, pairs, height) as t, DeviceTrieNodes.create(field_id, height) as ns:
        assert t.root == ref.root
        ns.add_trie(t)
        assert ns.n_nodes == len(want)
        _assert_store_holds(ns, ref, want)
        ns.add_trie(t)
        assert ns.n_nodes == len(want)
        _assert_store_holds(ns, ref, want)
        keys = [k for k, _ in pairs] + _absent_keys(field_id, height, pairs, 5)
        if keys:
            _lookup_all(ns, ref, [ref.root] * len(keys), keys)


# n = 300 where the trie has that many leaves and the reference (one host hash per node) stays within seconds: 900 items, four workgroups
@pytest.mark.parametrize("height,n", [(h, n) for h in (1, 2, 3, 85) for n in (0, 1, 2, 9, 300) if n <= 9 or h == 3])
def test_add_trie_registers_every_node_once(hip, height, n):
    _check_add_trie(BN, height, n)


@pytest.mark.parametrize("field_id,height", [(0, 2), (0, 85), (1, 2), (1, 85)])
def test_add_trie_the_other_fields(hip, field_id, height):
    _check_add_trie(field_id, height, 9)


def test_add_trie_300_keys_at_the_standard_height(hip):
    """25 500 items, a hundred workgroups, no host hash: with no value 0 every node key i opens is a new digest, so the count is H (the
    empty chain) + H (key 0) + H - 1 - shared[i] for every further key in path order; the content is checked through the lookups, which
    must be the handle's byte for byte."""
    import torch

    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, _elems

    H = 85
    pairs = sorted((k, v or 1000 + i) for i, (k, v) in enumerate(_pairs(BN, H, 300, seed=3)))  # distinct values: no two subtrees alike
    nodes = 2 * H
    for (a, _), (b, _) in zip(pairs, pairs[1:]):
        pa, pb = T.path(BN, a, H), T.path(BN, b, H)
        shared = next(d for d in range(H) if pa[d] != pb[d])
        nodes += H - 1 - shared
    dk = _elems([k for k, _ in pairs] + _absent_keys(BN, H, pairs, 40))
    with DeviceTrie.build(BN, pairs, H) as t, DeviceTrieNodes.create(BN, H) as ns:
        ns.add_trie(t)
        assert ns.n_nodes == nodes
        ns.add_trie(t)
        assert ns.n_nodes == nodes
        paths, values, status, missing = ns.prove_lookup([t.root], dk)
        want = t.prove_lookup(dk)
        assert missing == 0 and torch.equal(paths, want[0]) and torch.equal(values, want[1])


# ---- 3. the root-addressed lookup is the handle-based one, byte for byte ------------------------------------------------------------------
@pytest.mark.parametrize("field_id,height", SHAPES)
def test_prove_lookup_equals_the_handle_based_call(hip, field_id, height):
    import torch

    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, _elems

    a, b = _pairs(field_id, height, 9, seed=1), _pairs(field_id, height, 7, seed=2)
    keys = [k for k, _ in a] + [k for k, _ in b] + _absent_keys(field_id, height, a + b, 6)
    twin = _twin(field_id, height, a[0][0])
    if twin is not None:
        keys.append(twin)  # two keys with one path value
    dk = _elems(keys)
    m = len(keys)
    with DeviceTrie.build(field_id, a, height) as ta, DeviceTrie.build(field_id, b, height) as tb, DeviceTrie.build(field_id, [], height) as te, \
            DeviceTrieNodes.create(field_id, height) as ns:
        for t in (ta, tb, te):
            ns.add_trie(t)
        handles = [ta, tb, te]
        want = [t.prove_lookup(dk) for t in handles]
        # one root for the whole batch
        for t, (wp, wv) in zip(handles, want):
            paths, values, status, missing = ns.prove_lookup([t.root], dk)
            assert missing == 0 and not status.cpu().numpy().any()
            assert torch.equal(paths, wp) and torch.equal(values, wv)
        # one root per query, the three versions mixed
        which = [j % 3 for j in range(m)]
        paths, values, status, missing = ns.prove_lookup([handles[w].root for w in which], dk)
        assert missing == 0 and not status.cpu().numpy().any()
        for j, w in enumerate(which):
            assert torch.equal(paths[j], want[w][0][j]) and torch.equal(values[j], want[w][1][j])
        if twin is not None:
            assert torch.equal(paths[-1], ns.prove_lookup([handles[which[-1]].root], [a[0][0]])[0][0])


# ---- 4. versions -----------------------------------------------------------------------------------------------------------------------
def _chain_case(field_id, height, m=40, seed=4):
    """base pairs, and m updates with repeated keys, present and absent, values of 0"""
    pairs = _pairs(field_id, height, 9, seed=seed)
    rng = random.Random(seed)
    p = R.modulus(field_id)
    pool = [k for k, _ in pairs[:4]] + _absent_keys(field_id, height, pairs, 4, seed=seed)
    twin = _twin(field_id, height, pool[0])
    if twin is not None:
        pool.append(twin)
    updates = [(rng.choice(pool), rng.choice([0, rng.randrange(1, p), rng.randrange(1, p)])) for _ in range(m)]
    return pairs, updates


def _check_versions(field_id, height):
    import torch

    from lurk_beta_amd import poseidon_batch
    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes

    pairs, updates = _chain_case(field_id, height)
    m = len(updates)
    base = _ref_with(field_id, height, pairs)
    _, news, _, roots = CH.sequential(base, updates)
    ref, versions = base.copy(), []
    for k, v in updates:
        ref.prove_insert(k, v)
        versions.append(ref.root)
    assert versions == roots
    new_nodes = {T.hash8(field_id, pre) for proof in news for pre in proof}
    want = _reachable(base, base.root) | set(base.empty_roots) | new_nodes
    with DeviceTrie.build(field_id, pairs, height) as t, DeviceTrieNodes.create(field_id, height) as ns:
        _, new, _, got_roots, _ = t.insert_chain([k for k, _ in updates], [v for _, v in updates], trie=False)
        assert _ints(got_roots) == roots
        ns.add_trie(t)
        batch = new.reshape(m * height, 8, 4)
        digests = ns.register(batch)
        assert ns.n_nodes == len(want)
        assert np.array_equal(_u64(digests), poseidon_batch(field_id, 8, _u64(batch)))
        again = ns.register(batch)
        assert ns.n_nodes == len(want) and torch.equal(again, digests)
        twice = torch.stack([batch, batch], dim=1).reshape(2 * m * height, 8, 4).contiguous()  # every preimage twice, side by side
        ns.register(twice)
        assert ns.n_nodes == len(want)
        _assert_store_holds(ns, ref, want)
        # every version is addressable: all keys at every root
        keys = sorted({k for k, _ in pairs} | {k for k, _ in updates})
        all_roots = [base.root] + roots
        _lookup_all(ns, ref, [r for r in all_roots for _ in keys], keys * len(all_roots))


@pytest.mark.parametrize("field_id,height", [(BN, 3), (BN, 85), (0, 2), (1, 2)])
def test_every_version_of_a_chain_is_addressable(hip, field_id, height):
    _check_versions(field_id, height)


# ---- 5. missing preimages --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height,k", [(1, 0), (3, 1), (3, 2), (85, 40), (85, 84)])
def test_missing_preimages_are_reported_by_level(hip, height, k):
    from lurk_beta_amd.trie import DeviceTrieNodes

    pairs = _pairs(BN, height, 9, seed=6)
    ref = _ref_with(BN, height, pairs)
    key = pairs[0][0]  # present, its value is not 0: no node on its path is an empty subtree
    assert pairs[0][1] != 0
    proof = ref.prove_lookup(key)
    rng = random.Random(5)
    stranger = rng.randrange(R.modulus(BN))
    with DeviceTrieNodes.create(BN, height) as ns:
        if k:
            ns.register(_pre_np(proof[:k]))  # the path down to level k - 1
        assert ns.n_nodes == height + k
        empty = ref.empty_roots[-1]
        paths, values, status, missing = ns.prove_lookup([ref.root, empty, stranger, ref.root], [key, key, key, key])
        assert status.cpu().numpy().tolist() == [k + 1, 0, 1, k + 1] and missing == 3
        got = _u64(paths)
        assert np.array_equal(got[0, :k], _paths_np([proof[:k]], k)[0]) and not got[0, k:].any()
        assert not got[2].any() and np.array_equal(got[3], got[0])
        assert _ints(values) == [0, 0, 0, 0]
        assert np.array_equal(got[1], _paths_np([T.RefTrie(BN, height).prove_lookup(key)], height)[0])
        assert ns.n_nodes == height + k


# ---- 6. prove_insert at mixed version roots --------------------------------------------------------------------------------------------
def _insert_case(field_id, height):
    pairs, updates = _chain_case(field_id, height, m=12)
    base = _ref_with(field_id, height, pairs)
    ref, roots = base.copy(), [base.root]
    for k, v in updates:
        ref.prove_insert(k, v)
        roots.append(ref.root)
    rng = random.Random(9)
    p = R.modulus(field_id)
    pool = sorted({k for k, _ in pairs} | {k for k, _ in updates}) + _absent_keys(field_id, height, pairs, 3, seed=10)
    queries = [(rng.choice(roots), rng.choice(pool), rng.randrange(1, p)) for _ in range(30)]
    queries.append((roots[3], pool[0], 0))
    want = []
    for r, k, v in queries:
        c = ref.copy()
        c.root = r
        old, new, _ = c.prove_insert(k, v)
        want.append((old, new, old[-1][c.path(k)[-1]], c.root))
    return pairs, updates, ref, queries, want


@pytest.mark.parametrize("field_id,height", [(BN, 1), (BN, 3), (BN, 85), (0, 2), (1, 85)])
def test_prove_insert_at_mixed_roots_equals_the_reference(hip, field_id, height):
    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, verify_insert_batch

    pairs, updates, ref, queries, want = _insert_case(field_id, height)
    roots, keys, values = ([q[j] for q in queries] for j in range(3))
    with DeviceTrie.build(field_id, pairs, height) as t, DeviceTrieNodes.create(field_id, height) as ns:
        ns.add_trie(t)
        ns.insert_chain(t.root, [k for k, _ in updates], [v for _, v in updates])
        n0 = ns.n_nodes

        def check(got):
            old, new, old_values, new_roots, status, missing = got
            assert missing == 0 and not status.cpu().numpy().any()
            assert np.array_equal(_u64(old), _paths_np([w[0] for w in want], height))
            assert np.array_equal(_u64(new), _paths_np([w[1] for w in want], height))
            assert _ints(old_values) == [w[2] for w in want] and _ints(new_roots) == [w[3] for w in want]
            codes, failed = verify_insert_batch(field_id, height, roots, new_roots, keys, old_values, values, old, new)
            assert failed == 0 and not codes.any()

        check(ns.prove_insert(roots, keys, values, register_new=False))
        assert ns.n_nodes == n0
        fresh = [j for j, w in enumerate(want) if w[3] not in set(roots)]
        assert len(fresh) >= 20
        _, _, status, missing = ns.prove_lookup([want[j][3] for j in fresh], [keys[j] for j in fresh])
        assert status.cpu().numpy().tolist() == [1] * len(fresh) and missing == len(fresh)
        check(ns.prove_insert(roots, keys, values, register_new=True))
        after = ref.copy()
        for r, k, v in queries:
            c = after.copy()
            c.root = r
            c.prove_insert(k, v)
            after.children.update(c.children)
        assert ns.n_nodes == n0 + len({T.hash8(field_id, pre) for w in want for pre in w[1]} - _all_registered(ref, pairs, updates))
        _, got_values = _lookup_all(ns, after, [w[3] for w in want], keys)
        assert _ints(got_values) == values


def _all_registered(ref, pairs, updates):
    """what the store of the insert test holds before the inserts: the base trie, the empty chain, every node the chain left"""
    base = _ref_with(ref.field_id, ref.height, pairs)
    _, news, _, _ = CH.sequential(base, updates)
    return _reachable(base, base.root) | set(base.empty_roots) | {T.hash8(ref.field_id, pre) for proof in news for pre in proof}


# ---- 7. a chain that starts at a root ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_id,height", [(BN, 1), (BN, 2), (BN, 3), (BN, 85), (0, 85), (1, 2)])
def test_insert_chain_at_a_root(hip, field_id, height):
    import torch

    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, verify_insert_batch

    pairs, updates = _chain_case(field_id, height, m=40)
    base = _ref_with(field_id, height, pairs)
    olds, news, old_values, roots = CH.sequential(base, updates)
    keys, values = [k for k, _ in updates], [v for _, v in updates]
    with DeviceTrie.build(field_id, pairs, height) as t, DeviceTrieNodes.create(field_id, height) as ns:
        ns.add_trie(t)
        n0 = ns.n_nodes
        want = t.insert_chain(keys, values, trie=False)
        got = ns.insert_chain(t.root, keys, values)
        for a, b in zip(want[:4], got):
            assert torch.equal(a, b)
        assert _ints(got[3]) == roots and _ints(got[2]) == old_values
        assert np.array_equal(_u64(got[0]), _paths_np(olds, height)) and np.array_equal(_u64(got[1]), _paths_np(news, height))
        assert ns.n_nodes == len(_all_registered(base, pairs, updates)) >= n0
        codes, failed = verify_insert_batch(field_id, height, [base.root] + roots[:-1], got[3], keys, got[2], values, got[0], got[1])
        assert failed == 0 and not codes.any()
        # all m roots are addressable: every update's key at the root it left, and a second chain from a root in the middle
        ref = base.copy()
        for k, v in updates:
            ref.prove_insert(k, v)
        _, vals = _lookup_all(ns, ref, roots, keys)
        assert _ints(vals) == values
        mid = ref.copy()
        mid.root = roots[17]
        want2 = CH.sequential(mid, updates[:9])
        got2 = ns.insert_chain(roots[17], keys[:9], values[:9], paths=False)
        assert got2[0] is None and _ints(got2[3]) == want2[3] and _ints(got2[2]) == want2[2]


def test_a_chain_whose_third_key_misses_is_refused_by_name(hip):
    from lurk_beta_amd import LurkHipError
    from lurk_beta_amd.trie import DeviceTrieNodes

    height, k = 3, 2
    pairs = [p for p in _pairs(BN, height, 9, seed=12) if p[1] != 0]
    ref = _ref_with(BN, height, pairs)
    keys = [p[0] for p in pairs[:4]]
    with DeviceTrieNodes.create(BN, height) as ns:
        for j, key in enumerate(keys):
            proof = ref.prove_lookup(key)
            ns.register(_pre_np(proof[:k] if j == 2 else proof))
        hole = ref.prove_lookup(keys[2])[k - 1][ref.path(keys[2])[k - 1]]
        _, found = ns.get([hole])
        assert found.cpu().numpy().tolist() == [0]  # no other key's path goes through the node left out
        n0 = ns.n_nodes
        with pytest.raises(LurkHipError, match=rf"update 2: missing preimage at level {k}") as e:
            ns.insert_chain(ref.root, keys, [5, 6, 7, 8])
        assert e.value.code == 2 and ns.n_nodes == n0
        got = ns.insert_chain(ref.root, keys[:2], [5, 6])  # the store still works
        assert _ints(got[3]) == CH.sequential(ref, [(keys[0], 5), (keys[1], 6)])[3]


# ---- 8. growth -------------------------------------------------------------------------------------------------------------------------
def _check_growth(height=3):
    from lurk_beta_amd.trie import DeviceTrieNodes, _elems

    rng = random.Random(13)
    p = R.modulus(BN)
    with DeviceTrieNodes.create(BN, height, reserve_nodes=1) as ns:
        slots = [ns.info()["slots"]]
        assert slots[0] == 8  # the next power of two that keeps H = 3 nodes under half
        seen = {}
        for size in (3, 9, 40, 150, 600):
            pres = [[rng.randrange(p) for _ in range(8)] for _ in range(size)]
            pres[-1] = pres[0]  # one duplicate inside the batch
            if seen:
                pres[1] = next(iter(seen.values()))  # and one from an earlier batch
            digests = _ints(ns.register(_elems([x for pre in pres for x in pre])))
            seen.update({d: tuple(pre) for d, pre in zip(digests, pres)})
            assert digests == [T.hash8(BN, pre) for pre in pres]
            info = ns.info()
            slots.append(info["slots"])
            assert info["n_nodes"] == height + len(seen) and 2 * info["n_nodes"] <= info["slots"]
            order = sorted(seen)
            got, found = ns.get(order)
            assert found.cpu().numpy().all() and np.array_equal(_u64(got), _pre_np([seen[d] for d in order]))
        assert len(set(slots)) >= 4 and slots == sorted(slots)  # at least three rebuilds
        pre, found = ns.get(T.RefTrie(BN, height).empty_roots)
        assert found.cpu().numpy().all()


def test_growth_keeps_every_node(hip):
    _check_growth()


# ---- 9. one tag, many digests ----------------------------------------------------------------------------------------------------------
def test_tag_collisions(hip, monkeypatch):
    """two tag bits: three tags for hundreds of digests.  Every probe meets foreign nodes under its own tag; distinct digests must all be
    stored and duplicates stored once (the checks of 2, 4 and 8 again, at H = 3)"""
    monkeypatch.setenv("LURK_TRIE_NODES_TAG_BITS", "2")
    for n in (0, 1, 2, 9, 300):
        _check_add_trie(BN, 3, n)
    _check_versions(BN, 3)
    _check_growth(3)


# ---- 10. the independent check: by hash, and by the lookup circuit ------------------------------------------------------------------------
@pytest.mark.parametrize("field_id,height", [(BN, 3), (BN, 85), (1, 85)])
def test_the_verifiers_accept_root_addressed_lookups(hip, field_id, height):
    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, verify_lookup_batch

    pairs, updates = _chain_case(field_id, height, m=20)
    keys = sorted({k for k, _ in pairs} | {k for k, _ in updates})
    with DeviceTrie.build(field_id, pairs, height) as t, DeviceTrieNodes.create(field_id, height) as ns:
        ns.add_trie(t)
        roots = _ints(ns.insert_chain(t.root, [k for k, _ in updates], [v for _, v in updates], paths=False)[3])
        qr = [r for r in [t.root] + roots for _ in keys]
        qk = keys * (len(roots) + 1)
        paths, values, status, missing = ns.prove_lookup(qr, qk)
        assert missing == 0
        codes, failed = verify_lookup_batch(field_id, height, qr, qk, values, paths)
        assert failed == 0 and not codes.any()
        paths[5, height - 1, 0, 0] ^= 1  # and the verifier is awake
        assert verify_lookup_batch(field_id, height, qr, qk, values, paths)[1] == 1


def test_a_lookup_circuit_witness_from_a_root_addressed_proof_is_satisfied(hip):
    import torch

    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, _elems
    from lurk_beta_amd.trie_circuit import trie_circuit_shape, trie_circuit_size, trie_circuit_witness

    f, H, LOOKUP = BN, 3, 0
    pairs, updates = _chain_case(f, H, m=6)
    with DeviceTrie.build(f, pairs, H) as t, DeviceTrieNodes.create(f, H) as ns:
        ns.add_trie(t)
        roots = _ints(ns.insert_chain(t.root, [k for k, _ in updates], [v for _, v in updates], paths=False)[3])
        keys = [updates[-1][0], pairs[0][0], _absent_keys(f, H, pairs, 1)[0]]
        m = len(keys)
        d_roots, dk = _elems([roots[-1], roots[2], t.root]), _elems(keys)
        paths, values, status, missing = ns.prove_lookup(d_roots, dk)
        assert missing == 0
        sz = trie_circuit_size(f, H, LOOKUP)
        first, stride = 3, sz.size + 1
        num_vars = first + m * stride
        sh = trie_circuit_shape(f, H, LOOKUP, m, first, stride, num_vars, 2)
        d_w = torch.zeros((num_vars, 4), dtype=torch.int64, device="cuda")
        trie_circuit_witness(f, H, LOOKUP, d_roots, dk, paths, d_w, first=first, stride=stride)
        tail = torch.from_numpy(np.ascontiguousarray(C.to_mont(f, C.ints_to_limbs([1, 0, 0])), dtype=np.uint64).view(np.int64)).cuda()
        assert sh.is_sat(torch.cat([d_w, tail])) == (0, sh.num_cons)
        w = _u64(d_w)
        assert C.limbs_to_ints(C.from_mont(f, w[[first + i * stride + sz.result_col for i in range(m)]])) == _ints(values)


# ---- 11. refusals: nothing launched, the store unchanged -------------------------------------------------------------------------------
def test_refusals_leave_the_store_alone(hip):
    import torch

    from lurk_beta_amd import LurkHipError, _lib
    from lurk_beta_amd.trie import DeviceTrie, DeviceTrieNodes, _elems

    H, p = 3, R.modulus(BN)
    h = ctypes.c_void_p(0x5A5A)
    for field_id, height, match in ((3, H, "field"), (7, H, "field"), (BN, 0, "height"), (BN, 86, "height")):
        with pytest.raises(LurkHipError, match=match) as e:
            _lib.check(hip.lurk_hip_trie_nodes_create(ctypes.byref(h), field_id, height, 0))
        assert e.value.code == 2 and not h.value
        h = ctypes.c_void_p(0x5A5A)
    with pytest.raises(LurkHipError, match="null"):
        _lib.check(hip.lurk_hip_trie_nodes_create(None, BN, H, 0))
    with pytest.raises(LurkHipError, match="null"):
        _lib.check(hip.lurk_hip_trie_nodes_info(None, None, None, None, None, None))

    pairs = _pairs(BN, H, 9, seed=16)
    keys = [k for k, _ in pairs[:4]]
    m = len(keys)
    with DeviceTrie.build(BN, pairs, H) as t, DeviceTrie.build(0, [], H) as other_field, DeviceTrie.build(BN, pairs, 2) as other_height, \
            DeviceTrieNodes.create(BN, H) as ns:
        ns.add_trie(t)
        n0, slots0 = ns.n_nodes, ns.info()["slots"]
        root = t.root
        proof0 = [x.clone() for x in ns.prove_lookup([root], keys)[:3]]
        dk, dv, dr = _elems(keys), _elems([5, 6, 7, 8]), _elems([root] * m)
        buf = lambda: torch.zeros((m, H, 8, 4), dtype=torch.int64, device="cuda")
        row = lambda: torch.zeros((m, 4), dtype=torch.int64, device="cuda")
        o, n_, v, r, st = buf(), buf(), row(), row(), torch.zeros(m, dtype=torch.int32, device="cuda")
        pre = _elems([1] * 16)
        dig, found = torch.zeros((2, 4), dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        miss = ctypes.c_uint64()
        P = _lib.ptr

        def refused(match, fn, *args):
            with pytest.raises(LurkHipError, match=match) as e:
                _lib.check(fn(*args))
            assert e.value.code == 2
            for x in (o, n_, v, r, st, dig, found):
                assert not x.any()  # nothing was launched
            info = ns.info()
            assert info["n_nodes"] == n0 and info["slots"] == slots0
            for a, b in zip(ns.prove_lookup([root], keys)[:3], proof0):
                assert torch.equal(a, b)

        reg, add, get = hip.lurk_hip_trie_nodes_register_dev, hip.lurk_hip_trie_nodes_add_trie, hip.lurk_hip_trie_nodes_get_dev
        look, ins, chain = hip.lurk_hip_trie_nodes_prove_lookup_dev, hip.lurk_hip_trie_nodes_prove_insert_dev, hip.lurk_hip_trie_nodes_insert_chain_dev
        root32 = C.ints_to_limbs([root])
        # NULLs
        refused("null", reg, None, P(pre), 2, P(dig), None)
        refused("null", reg, ns._h, None, 2, P(dig), None)
        refused("null", add, ns._h, None, None)
        refused("null", add, None, t._h, None)
        refused("null", get, ns._h, None, 2, P(o), P(found), None)
        refused("null", get, ns._h, P(dig), 2, P(o), None, None)
        refused("null", look, None, P(dr), 1, P(dk), m, P(o), P(v), P(st), ctypes.byref(miss), None)
        refused("null", look, ns._h, P(dr), 1, P(dk), m, P(o), P(v), None, ctypes.byref(miss), None)
        refused("null", look, ns._h, None, 1, P(dk), m, P(o), P(v), P(st), None, None)
        refused("null", ins, ns._h, P(dr), 1, P(dk), P(dv), m, P(o), None, P(v), P(r), P(st), None, 1, None)
        refused("null", ins, ns._h, P(dr), 1, P(dk), None, m, P(o), P(n_), P(v), P(r), P(st), None, 1, None)
        refused("null", chain, ns._h, None, P(dk), P(dv), m, P(o), P(n_), P(v), P(r), None)
        refused("null", chain, ns._h, P(root32), None, P(dv), m, P(o), P(n_), P(v), P(r), None)
        # a trie of another field or height
        refused("another field", add, ns._h, other_field._h, None)
        refused("another height", add, ns._h, other_height._h, None)
        # root_stride
        refused("root_stride", look, ns._h, P(dr), 2, P(dk), m, P(o), P(v), P(st), None, None)
        refused("root_stride", ins, ns._h, P(dr), 2, P(dk), P(dv), m, P(o), P(n_), P(v), P(r), P(st), None, 1, None)
        refused("overlap", ins, ns._h, P(dr), 1, P(dk), P(dv), m, P(o), o.data_ptr() + 256 * H * (m - 1), P(v), P(r), P(st), None, 1, None)
        # elements that are not reduced, the first one named
        bad_k, bad_v, bad_r = _elems(keys[:2] + [p + 1, p]), _elems([5, p, 7, p + 3]), _elems([root, root, root, p])
        refused("key 2 is not reduced", look, ns._h, P(dr), 1, P(bad_k), m, P(o), P(v), P(st), None, None)
        refused("root 3 is not reduced", look, ns._h, P(bad_r), 1, P(dk), m, P(o), P(v), P(st), None, None)
        refused("root 0 is not reduced", look, ns._h, P(bad_r[3:]), 0, P(dk), m, P(o), P(v), P(st), None, None)
        refused("key 2 is not reduced", ins, ns._h, P(dr), 1, P(bad_k), P(dv), m, P(o), P(n_), P(v), P(r), P(st), None, 1, None)
        refused("new value 1 is not reduced", ins, ns._h, P(dr), 1, P(dk), P(bad_v), m, P(o), P(n_), P(v), P(r), P(st), None, 1, None)
        refused("root 3 is not reduced", ins, ns._h, P(bad_r), 1, P(dk), P(dv), m, P(o), P(n_), P(v), P(r), P(st), None, 1, None)
        refused("key 2 is not reduced", chain, ns._h, P(root32), P(bad_k), P(dv), m, P(o), P(n_), P(v), P(r), None)
        refused("value 1 is not reduced", chain, ns._h, P(root32), P(dk), P(bad_v), m, P(o), P(n_), P(v), P(r), None)
        refused("root is not reduced", chain, ns._h, P(C.ints_to_limbs([p])), P(dk), P(dv), m, P(o), P(n_), P(v), P(r), None)
        bad_pre = _elems([1] * 11 + [p + 2, 3, p, 1, 1])
        refused("preimage element 11 is not reduced", reg, ns._h, P(bad_pre), 2, P(dig), None)
        # and the calls do work with the good arguments
        if torch.cuda.device_count() > 1:  # a store resident on device 0, asked from device 1
            try:
                torch.cuda.set_device(1)
                elsewhere = torch.zeros((2, 4), dtype=torch.int64, device="cuda:1")
                refused("another device", get, ns._h, P(elsewhere), 2, P(elsewhere), P(elsewhere), None)
            finally:
                torch.cuda.set_device(0)
        _lib.check(look(ns._h, P(dr), 1, P(dk), m, P(o), P(v), P(st), ctypes.byref(miss), None))
        assert miss.value == 0 and torch.equal(o, proof0[0])
