"""A chain of dependent trie inserts, stated level by level in Python integers: the independent statement of what
lurk_hip_trie_insert_chain_dev computes, and the cases both its CPU and its GPU tests run.

Update i = (key_i, value_i) is applied to T_i and leaves T_{i+1} (the reference's ``insert_at_path``, src/coprocessor/trie/mod.rs:760-776,
restated as ``tests.trie_ref.RefTrie.prove_insert``).  Sequentially that is m * H dependent hashes.  Level-synchronously it is H rounds:

* at the node that update i passes at depth d, the preimage it FINDS is the node's preimage in T_0 with every child entry c replaced by
  the new hash (one level down) of the latest EARLIER update that went through child c; the preimage it LEAVES has its own child's new
  hash put in as well; its new hash at depth d is the hash of the preimage it leaves.  So depth d needs depth d + 1 only.
* "the latest earlier update through child c" is a search, not a scan over the node's updates: ``order[e]`` keeps the updates sorted by
  (top-e-digit prefix, sequence index) - one stable 8-way split per depth of the order above it - and ``skey[e][q]`` = 8 * (start of the
  depth e - 1 node in the order) + digit e - 1 is non-decreasing along it.  The updates through child c of a node are one run of
  ``skey[d + 1]``, sorted by sequence index: two binary searches find the run, a third the last entry before i.
* once every node of a depth holds the updates of ONE path value the orders below are all the same, and only an update's own child has
  earlier setters: its predecessor in the run (``short=True`` stops splitting there, as the device code does).

Nothing here imports the library."""
from __future__ import annotations

import random
from bisect import bisect_left

from oracle import pyref as R
from tests import trie_ref as T


def sequential(base: T.RefTrie, updates):
    """The checker: RefTrie.prove_insert applied in sequence to a copy of ``base`` -> (old paths, new paths, old values, roots)"""
    t = base.copy()
    olds, news, old_values, roots = [], [], [], []
    for key, value in updates:
        old, new, _ = t.prove_insert(key, value)
        olds.append(old)
        news.append(new)
        old_values.append(old[-1][t.path(key)[-1]])
        roots.append(t.root)
    return olds, news, old_values, roots


def split_orders(digits, height: int, short: bool):
    """-> (order, skey, depth): order[e], skey[e] for e = 1 .. depth; below ``depth`` (< height only when ``short``) the order is
    order[depth] and a node's updates are the run that starts at label[q]"""
    m = len(digits)
    order, label = list(range(m)), [0] * m
    orders, skeys = {0: order}, {}
    e = 0
    while e < height:
        if short and not any(label[q] == label[q - 1] and digits[order[q]] != digits[order[q - 1]] for q in range(1, m)):
            break
        keyed = sorted(((label[q] * 8 + digits[order[q]][e], q) for q in range(m)))  # (key, position): stable
        e += 1
        skeys[e] = [k for k, _ in keyed]
        order = [order[q] for _, q in keyed]
        orders[e] = order
        label = [bisect_left(skeys[e], k) for k in skeys[e]]
    return orders, skeys, e, label


def level_synchronous(base: T.RefTrie, updates, short: bool = False, hash8=None):
    """The chain in H rounds, bottom-up -> (old paths, new paths, old values, roots), shaped as ``sequential`` gives them."""
    H, m = base.height, len(updates)
    hash8 = hash8 or (lambda pre: T.hash8(base.field_id, pre))
    digits = [base.path(k) for k, _ in updates]
    t0 = [base.prove_lookup(k) for k, _ in updates]  # the preimages of T_0 along every update's path
    orders, skeys, depth, label = split_orders(digits, H, short)
    olds = [[None] * H for _ in range(m)]
    news = [[None] * H for _ in range(m)]
    below = [v for _, v in updates]  # the new hash one level down: at the leaf level, the value
    for d in range(H - 1, -1, -1):
        here = [None] * m
        e = min(d + 1, depth)
        order = orders[e]
        for q, i in enumerate(order):
            pre, own = list(t0[i][d]), digits[i][d]
            if d + 1 <= depth:
                node = skeys[e][q] >> 3
                for c in range(8):
                    a, b = bisect_left(skeys[e], node * 8 + c), bisect_left(skeys[e], node * 8 + c + 1)
                    r = bisect_left(order, i, a, b) - 1  # the run is sorted by sequence index
                    if r >= a:
                        pre[c] = below[order[r]]
            elif q > label[q]:
                pre[own] = below[order[q - 1]]
            olds[i][d] = tuple(pre)
            pre[own] = below[i]
            news[i][d] = tuple(pre)
            here[i] = hash8(pre)
        below = here
    old_values = [olds[i][H - 1][digits[i][H - 1]] for i in range(m)]
    return olds, news, old_values, below


def final_pairs(base_pairs, updates, height: int):
    """What T_m holds: the base pairs, then the last update per path value, sorted by path value (a value of 0 stays a pair)."""
    mask = (1 << (3 * height)) - 1
    last = {}
    for k, v in list(base_pairs) + list(updates):
        last[k & mask] = (k, v)
    return [last[p] for p in sorted(last)]


def base_trie(field_id: int, height: int, pairs) -> T.RefTrie:
    t = T.RefTrie(field_id, height)
    for k, v in pairs:
        t.insert(k, v)
    return t


def base_pairs(field_id: int, height: int, populated: bool, seed: int = 1):
    """no key, or about ten (fewer where the trie has fewer leaves) with distinct path values, one of them with the value 0"""
    if not populated:
        return []
    rng = random.Random(1000 * seed + 10 * height + field_id)
    p, leaves = R.modulus(field_id), 8 ** height
    n = min(10, leaves - 3)
    pvs = rng.sample(range(leaves), n) if leaves < 1 << 20 else [rng.getrandbits(3 * height) % p for _ in range(n)]
    pairs = [(pv, rng.randrange(1, p)) for pv in pvs]
    pairs[-1] = (pairs[-1][0], 0)
    return pairs


def families(field_id: int, height: int, base, seed: int = 0):
    """-> [(name, updates)], at most 200 updates each: the case list of the chain's tests.  ``base``: the pairs of T_0."""
    rng = random.Random(7919 * seed + 31 * height + field_id + 101 * len(base))
    p, bits = R.modulus(field_id), 3 * height
    top = 7 << (bits - 3)

    def val():
        return rng.randrange(1, p)

    def key():  # a reduced key; below 255 path bits some carry bits above the path, which select the same leaf
        k = rng.getrandbits(bits)
        if bits < 200 and rng.random() < 0.5:
            k |= rng.getrandbits(20) << bits
        return k % p

    have = {k & ((1 << bits) - 1) for k, _ in base}
    absent = []
    while len(absent) < 6 and len(absent) + len(have) < 8 ** height:
        k = key()
        if k & ((1 << bits) - 1) not in have | {a & ((1 << bits) - 1) for a in absent}:
            absent.append(k)
    present = [k for k, _ in base]
    k0 = key()
    out = [("one key 64 times", [(k0, val()) for _ in range(64)])]
    out.append(("last digit alternating", [(k0 ^ (j & 1), val()) for j in range(40)]))
    k1 = k0 & ~top & ((1 << bits) - 1)  # below the top digit, so that flipping it keeps the key reduced
    out.append(("first digit alternating", [(k1 | ((j & 1) << (bits - 3)), val()) for j in range(40)]))
    pool = [key() for _ in range(min(24, 8 ** height))]
    out.append(("colliding random keys", [(rng.choice(pool), val()) for _ in range(150)]))
    mix = (present + absent) or pool
    out.append(("present and absent", [(rng.choice(mix), val()) for _ in range(60)]))
    zk = [absent[0] if absent else k0] + present[:2]
    out.append(("to zero and back", [(k, v) for k in zk for v in (val(), 0)] + [(k, val()) for k in zk] + [(zk[0], 0), (zk[0], 0)]))
    same = [(k0, 5), (k0, 5), (absent[-1] if absent else k0 ^ 1, 0)] + [(k, v) for k, v in base[:3]] + [(k0, 5)]
    out.append(("repeats the current value", same))
    multiset = [(rng.choice(pool[:6]), val()) for _ in range(48)]
    for tag in ("a", "b"):
        shuffled = list(multiset)
        random.Random(tag).shuffle(shuffled)
        out.append(("one multiset, order " + tag, shuffled))
    return out
