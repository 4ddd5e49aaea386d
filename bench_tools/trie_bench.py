#!/usr/bin/env python3
"""The device-resident Poseidon trie (lurk_hip_trie_*) on one device: BN254 Fr, height 85 (lurk-beta's StandardTrie).

  build     n = 2^12, 2^16, 2^20 random keys, sorted on the host beforehand (the sort is not timed): lurk_hip_trie_build_dev
  proofs    2^16 lookup proofs of the 2^16-key trie (half the keys present, half absent): lurk_hip_trie_prove_lookup_dev, then
            lurk_hip_trie_verify_lookup_dev over them
  baseline  the same trie by sequential inserts on ONE host core through lurk_hip_poseidon_hash_host (85 hashes per insert), measured at
            n = 2^12 and EXTRAPOLATED linearly above that (labelled so); the per-node GPU mirror (lurk_beta_amd.trie.Trie: 85 one-hash
            launches per insert) at n = 64

Method: HIP events on the null stream, the median of five after one warm-up.  Checked in every run: the device root against the
baseline's where both exist (2^12 against the host inserts, 64 keys against the mirror), and every proof against the verify kernel
(n_failed == 0).  Writes the result as JSON (default profiles/r10_trie_bench.json) and prints it as one line.

    python bench_tools/trie_bench.py [--out profiles/r10_trie_bench.json] [--max-log-n 20] [--skip-baseline]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELD, HEIGHT = 2, 85


def random_pairs(n, seed):
    """n distinct keys below 2^253 (< p) sorted by path value (= by value: 3 * 85 = 255 bits) and non-zero values, as (n, 4) uint64"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    keys[:, 3] &= np.uint64((1 << 61) - 1)
    keys = keys[np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2], keys[:, 3]))]
    assert not (keys[1:] == keys[:-1]).all(axis=1).any()
    values = rng.integers(1, 1 << 62, size=(n, 4), dtype=np.uint64)
    values[:, 3] &= np.uint64((1 << 61) - 1)
    return keys, values


def timed(fn, reps=5):
    import torch

    fn()  # warm-up
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def host_sequential_root(lib, keys, values):
    """coprocessor::trie::Trie::insert for every pair, one host hash per node (lurk_hip_poseidon_hash_host) -> (root, seconds)"""
    from lurk_beta_amd import _lib
    from lurk_beta_amd.poseidon import _ints

    pre = np.zeros((8, 4), dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint64)
    children = {}

    def hash8(p):
        for j, x in enumerate(p):
            for w in range(4):
                pre[j, w] = (x >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
        _lib.check(lib.lurk_hip_poseidon_hash_host(FIELD, 8, _lib.ptr(pre), 1, _lib.ptr(out)))
        h = int(out[0]) | int(out[1]) << 64 | int(out[2]) << 128 | int(out[3]) << 192
        children[h] = tuple(p)
        return h

    cur, empty = 0, [0]
    for _ in range(HEIGHT):
        cur = hash8([cur] * 8)
        empty.append(cur)
    root = empty[HEIGHT]
    t0 = time.perf_counter()
    for k, v in zip(_ints(keys), _ints(values)):
        digits = [(k >> (3 * (HEIGHT - 1 - d))) & 7 for d in range(HEIGHT)]
        pres, node = [], root
        for d in digits:
            p = children[node]
            pres.append(p)
            node = p[d]
        cur = v
        for p, d in zip(reversed(pres), reversed(digits)):
            q = list(p)
            q[d] = cur
            cur = hash8(q)
        root = cur
    return root, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_trie_bench.json"))
    ap.add_argument("--max-log-n", type=int, default=20)
    ap.add_argument("--skip-baseline", action="store_true")
    args = ap.parse_args()
    import torch

    from lurk_beta_amd import _lib
    from lurk_beta_amd.poseidon import _ints
    from lurk_beta_amd.trie import DeviceTrie, Trie, _dev

    lib = _lib.load()
    torch.cuda.set_device(0)
    res = {"field": "bn254_fr", "height": HEIGHT, "device": torch.cuda.get_device_name(0), "method": "HIP events, median of 5 after 1 warm-up", "build": {}}

    roots = {}
    for log_n in (12, 16, 20):
        if log_n > args.max_log_n:
            continue
        n = 1 << log_n
        keys, values = random_pairs(n, log_n)
        dk, dv = _dev(keys), _dev(values)

        def build():
            with DeviceTrie.build_sorted(FIELD, dk, dv, HEIGHT) as t:
                roots[log_n] = t.root

        med, all_ms = timed(build)
        res["build"][f"2^{log_n}"] = {"ms": round(med, 3), "all_ms": [round(x, 3) for x in all_ms], "keys_per_s": round(n / med * 1e3), "node_hash_bytes": HEIGHT * n * 32}

    # 2^16 lookup proofs against the 2^16-key trie: even queries present, odd ones absent (a present key with its low 128 bits flipped)
    log_m = min(16, args.max_log_n)
    m = 1 << log_m
    keys, values = random_pairs(m, log_m)
    queries = keys.copy()
    queries[1::2, 0] ^= np.uint64(0xFFFFFFFFFFFFFFFF)
    queries[1::2, 1] ^= np.uint64(0xFFFFFFFFFFFFFFFF)
    with DeviceTrie.build_sorted(FIELD, _dev(keys), _dev(values), HEIGHT) as t:
        dq = _dev(queries)
        out = {}

        def prove():
            out["p"], out["v"] = t.prove_lookup(dq)

        p_med, p_all = timed(prove)
        got = out["v"].cpu().numpy().view(np.uint64)
        assert np.array_equal(got[0::2], values[0::2]) and not got[1::2].any(), "looked-up values"
        verdict = {}

        def verify():
            verdict["codes"], verdict["failed"] = t.verify_lookup(dq, out["v"], out["p"])

        v_med, v_all = timed(verify)
        assert verdict["failed"] == 0 and not verdict["codes"].any(), "the verify kernel rejects the library's own proofs"
        res["lookup_proofs"] = {"proofs": m, "trie_keys": m, "prove_ms": round(p_med, 3), "prove_all_ms": [round(x, 3) for x in p_all], "verify_ms": round(v_med, 3),
                                "verify_all_ms": [round(x, 3) for x in v_all], "proof_bytes": HEIGHT * 256, "all_verified": True,
                                "verify_hashes_per_s": round(m * HEIGHT / v_med * 1e3)}

    if not args.skip_baseline:
        # one host core, sequential inserts, 2^12 keys; the same root as the device build
        keys, values = random_pairs(1 << 12, 12)
        root, secs = host_sequential_root(lib, keys, values)
        assert root == roots[12], "device root != sequential host inserts at 2^12"
        per_insert = secs / (1 << 12)
        res["baseline_host_sequential"] = {"n": 1 << 12, "seconds": round(secs, 3), "us_per_insert": round(per_insert * 1e6, 1), "root_matches_device": True,
                                           "extrapolated_seconds": {f"2^{k}": round(per_insert * (1 << k), 1) for k in (16, 20)},
                                           "note": "2^16 and 2^20 are linear extrapolations of the 2^12 measurement, not measurements"}
        # the per-node GPU mirror: 85 one-hash launches per insert
        k64, v64 = random_pairs(64, 64)
        mirror = Trie(FIELD)
        t0 = time.perf_counter()
        for k, v in zip(_ints(k64), _ints(v64)):
            mirror.insert(k, v)
        secs = time.perf_counter() - t0
        with DeviceTrie.build_sorted(FIELD, _dev(k64), _dev(v64), HEIGHT) as t:
            assert t.root == mirror.root, "device root != the mirror's at 64 keys"
        res["baseline_mirror_per_node_launches"] = {"n": 64, "seconds": round(secs, 3), "ms_per_insert": round(secs / 64 * 1e3, 2), "root_matches_device": True}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
