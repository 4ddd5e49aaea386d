#!/usr/bin/env python3
"""The trie coprocessor circuits' witness on one device: lurk_hip_trie_circuit_witness_dev at H = 85 (lurk-beta's StandardTrie), lookup and
insert, m = 1, 16, 256, 4096 blocks, on BN254 Fr and Pallas Fq - and, in the same run, what the library could do for the same hashes before
that call existed: lurk_hip_slot_witness_dev on the m H (insert: 2 m H) hash8 preimages of the same proofs plus lurk_hip_slot_witness_dev
on the m keys' bit decompositions, into packed blocks.  The new call does that work plus the picks, the root / value columns and the
placement inside a circuit block.

Method: proofs of m random keys against a 2^12-key trie (lurk_hip_trie_prove_insert_dev; not timed).  Per configuration one warm-up of
both, then `--reps` rounds that ALTERNATE the two, each timed with HIP events on the null stream; medians, and min / max as the spread.
Checked in every run: block 0's hash sub-blocks of the new call equal the baseline's blocks bit for bit.  Not part of bench.py; no pass
mark.  Writes JSON (default profiles/r18_trie_circuit_bench.json) and prints it as one line.

    python bench_tools/trie_circuit_bench.py [--out profiles/r18_trie_circuit_bench.json] [--max-m 4096] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEIGHT = 85
FIELDS = ((2, "bn254_fr"), (1, "pallas_fq"))


def random_elems(n, seed, sort=False):
    """n distinct elements below 2^253 as (n, 4) uint64, optionally sorted by value (= by path value at H = 85)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 61) - 1)
    if sort:
        a = a[np.lexsort((a[:, 0], a[:, 1], a[:, 2], a[:, 3]))]
    return a


def event_ms(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_trie_circuit_bench.json"))
    ap.add_argument("--max-m", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch

    from lurk_beta_amd import _lib, slot_witness_size
    from lurk_beta_amd.trie import DeviceTrie, _dev
    from lurk_beta_amd.trie_circuit import INSERT, LOOKUP, trie_circuit_size, trie_circuit_witness

    lib = _lib.load()
    torch.cuda.set_device(0)
    res = {"height": HEIGHT, "device": torch.cuda.get_device_name(0),
           "method": f"HIP events, null stream, 1 warm-up then {args.reps} alternating rounds; median (min, max)", "rows": []}
    for f, fname in FIELDS:
        kb = slot_witness_size(f, 1)
        with DeviceTrie.build_sorted(f, _dev(random_elems(1 << 12, 12, sort=True)), _dev(random_elems(1 << 12, 13)), HEIGHT) as trie:
            root = _dev(np.array([[(trie.root >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]], dtype=np.uint64))
            for m in (1, 16, 256, 4096):
                if m > args.max_m:
                    continue
                dk, dv = _dev(random_elems(m, 100 + m)), _dev(random_elems(m, 200 + m))
                old, new, _, _ = trie.prove_insert(dk, dv)
                both = torch.cat([old.reshape(m * HEIGHT, 8, 4), new.reshape(m * HEIGHT, 8, 4)])
                for op, oname in ((LOOKUP, "lookup"), (INSERT, "insert")):
                    sz = trie_circuit_size(f, HEIGHT, op)
                    n_hash = m * HEIGHT * (2 if op == INSERT else 1)
                    d_w = torch.empty((m * sz.size, 4), dtype=torch.int64, device="cuda")
                    d_b = torch.empty((n_hash * 396 + m * kb, 4), dtype=torch.int64, device="cuda")
                    pre = both if op == INSERT else both[:m * HEIGHT]

                    def new_call():
                        trie_circuit_witness(f, HEIGHT, op, root, dk, old, d_w, new_values=dv if op == INSERT else None, new_paths=new if op == INSERT else None,
                                             first=0, stride=sz.size)

                    def baseline():
                        _lib.check(lib.lurk_hip_slot_witness_dev(f, 8, _lib.ptr(pre), n_hash, 0, _lib.ptr(d_b), None, 0, 396, None))
                        _lib.check(lib.lurk_hip_slot_witness_dev(f, 1, _lib.ptr(dk), m, 0, _lib.ptr(d_b), None, n_hash * 396, kb, None))

                    new_call()
                    baseline()
                    torch.cuda.synchronize()
                    lvl = d_w[1 + kb:1 + kb + 403 * HEIGHT].view(HEIGHT, 403, 4)[:, :396]
                    assert torch.equal(lvl, d_b[:396 * HEIGHT].view(HEIGHT, 396, 4)), "the new call's hash blocks differ from lurk_hip_slot_witness_dev's"
                    t_new, t_base = [], []
                    for _ in range(args.reps):
                        t_new.append(event_ms(new_call))
                        t_base.append(event_ms(baseline))
                    mn, mb = statistics.median(t_new), statistics.median(t_base)
                    res["rows"].append({"field": fname, "op": oname, "m": m, "hash8_traces": n_hash, "form": "T lanes per hash" if n_hash <= 8192 else "one hash per lane",
                                        "w_bytes": m * sz.size * 32,
                                        "new_ms": round(mn, 4), "new_min_max_ms": [round(min(t_new), 4), round(max(t_new), 4)], "new_blocks_per_s": round(m / mn * 1e3, 1),
                                        "baseline_ms": round(mb, 4), "baseline_min_max_ms": [round(min(t_base), 4), round(max(t_base), 4)],
                                        "baseline_blocks_per_s": round(m / mb * 1e3, 1), "new_over_baseline_time": round(mn / mb, 3)})
                    del d_w, d_b
                del old, new, both
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
