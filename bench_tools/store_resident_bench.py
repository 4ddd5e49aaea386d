#!/usr/bin/env python3
"""The device-resident store (lurk_hip_store) against the one-shot hydration (lurk_hip_store_hydrate) on one device, Pallas Fq, on
store_hasher.wide_dag(12000) (~4 x 10^5 nodes, ~30 levels) and list_dag(400) (409 levels, a 400-cell spine), all in one process:

  (a) one_shot        lurk_hip_store_hydrate on the whole DAG: every record and value up, every node hashed, every digest down
  (b) append_all      ONE append of the whole DAG into a fresh store of sufficient capacity, with the digests coming back (the traffic of
                      (a)) and without (new_digests32 = NULL)
  (c) append_tail     the append of the LAST 1 % of the nodes after the first 99 % are resident, no digests back - set beside what a caller
                      has to do today for the same growth, which is (a) again
  (d) slot_preimages  lurk_hip_store_slot_preimages_dev for 2^16 hash8 slots of four pointers each to random nodes of the wide DAG
                      (descriptors resident, and with their upload), canonical - set against building the same preimages on the host
                      from downloaded digests (lurk_hip_store_digests of the distinct nodes) and uploading them

Method: a host clock around calls that end in a device synchronisation (the appends and the one-shot call synchronise themselves; (d) is
followed by torch.cuda.synchronize()), two warm-ups, the median of seven repetitions with their minimum and maximum.  Checked on the way:
the store's digests after (b) and after (c) are the one-shot call's, and the two sides of (d) are equal.  Prints one JSON line and writes it.

    python bench_tools/store_resident_bench.py [--out profiles/store_resident_bench.json] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELD = 1  # LURK_FIELD_PALLAS_FQ


def timed(fn, reps, warmup=2, setup=None):
    """-> {"median_ms", "min_ms", "max_ms", "all_ms"} of fn(setup()) over `reps` runs after `warmup`; only fn is on the clock"""
    import torch

    out = []
    for k in range(warmup + reps):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg) if setup else fn()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(out)), 3), "min_ms": round(min(out), 3), "max_ms": round(max(out), 3), "all_ms": [round(x, 3) for x in out]}


def bench_dag(name, nodes, reps):
    from lurk_beta_amd import DeviceStore
    from lurk_beta_amd import store_hasher as SH

    rec, vals = SH.encode(nodes)
    n = rec.shape[0]
    cut = n - max(1, n // 100)
    rec_head, vals_head = SH.encode(nodes[:cut])
    rec_tail, vals_tail = SH.encode(nodes[cut:])
    res = {"nodes": n, "hashed_nodes": int(np.count_nonzero(rec[:, 0])), "tail_nodes": n - cut, "tail_hashed_nodes": int(np.count_nonzero(rec_tail[:, 0]))}
    keep = {}

    def one_shot():
        keep["want"], keep["levels"] = SH.hydrate_records(FIELD, rec, vals)

    res["one_shot"] = timed(one_shot, reps)
    res["levels"] = keep["levels"]
    want = keep["want"]
    stores = []

    def fresh(head=False):
        for s in stores:
            s.close()
        stores[:] = [DeviceStore(FIELD, reserve_nodes=n)]
        if head:
            stores[0].append_records(rec_head, vals_head)
        return stores[0]

    res["append_all_digests_back"] = timed(lambda s: keep.__setitem__("got", s.append_records(rec, vals, digests=True)[1]), reps, setup=fresh)
    assert np.array_equal(keep["got"], want), "append (digests back) != one shot"
    res["append_all"] = timed(lambda s: s.append_records(rec, vals), reps, setup=fresh)
    assert np.array_equal(stores[0].digests(np.arange(n)), want), "append != one shot"
    res["append_tail_1pct"] = timed(lambda s: s.append_records(rec_tail, vals_tail), reps, setup=lambda: fresh(head=True))
    info = stores[0].info()
    assert info["n_nodes"] == n and info["hashes_done"] == res["hashed_nodes"] and info["levels"] == res["levels"]
    assert np.array_equal(stores[0].digests(np.arange(n)), want), "head + tail != one shot"
    res["tail_over_one_shot"] = round(res["append_tail_1pct"]["median_ms"] / res["one_shot"]["median_ms"], 4)
    res["append_all_over_one_shot"] = round(res["append_all_digests_back"]["median_ms"] / res["one_shot"]["median_ms"], 3)
    return res, stores[0], rec


def bench_slots(store, rec, reps, log_slots=16):
    import torch

    from lurk_beta_amd import _lib
    from lurk_beta_amd.store_resident import SLOT_ELEM_DIGEST, SLOT_ELEM_TAG

    lib = _lib.load()
    n, m = rec.shape[0], (1 << log_slots) * 4  # pointers
    ids = np.random.default_rng(5).integers(0, n, size=m, dtype=np.uint32)
    elems = np.empty((2 * m, 2), dtype=np.uint32)
    elems[0::2, 0], elems[1::2, 0] = SLOT_ELEM_TAG, SLOT_ELEM_DIGEST
    elems[0::2, 1] = elems[1::2, 1] = ids
    out = torch.empty((2 * m, 4), dtype=torch.int64, device="cuda")
    d_elems = torch.from_numpy(elems.view(np.int32)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def device(d):
        _lib.check(lib.lurk_hip_store_slot_preimages_dev(store._h, _lib.ptr(d), 2 * m, 0, _lib.ptr(out), _lib.ptr(stream)))

    res = {"slots": 1 << log_slots, "elements": 2 * m, "preimage_bytes": 2 * m * 32, "descriptor_bytes": 2 * m * 8}
    res["device_descriptors_resident"] = timed(lambda: device(d_elems), reps)
    res["device_with_descriptor_upload"] = timed(lambda: device(torch.from_numpy(elems.view(np.int32)).cuda()), reps)
    got = out.cpu().numpy().view(np.uint64)
    tags = rec[:, 1].astype(np.uint64)
    keep = {}

    def host():
        uniq, inv = np.unique(ids, return_inverse=True)
        dig = store.digests(uniq)  # the download
        pre = np.zeros((2 * m, 4), dtype=np.uint64)
        pre[0::2, 0] = tags[ids]
        pre[1::2] = dig[inv]
        keep["dev"] = torch.from_numpy(pre.view(np.int64)).cuda()  # the upload

    res["host_round_trip"] = timed(host, reps)
    assert np.array_equal(keep["dev"].cpu().numpy().view(np.uint64), got), "device-built preimages != host-built"
    res["distinct_nodes_downloaded"] = int(np.unique(ids).size)
    res["host_over_device"] = round(res["host_round_trip"]["median_ms"] / res["device_with_descriptor_upload"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "store_resident_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--wide", type=int, default=12000)
    ap.add_argument("--deep", type=int, default=400)
    args = ap.parse_args()
    assert args.reps >= 5, "the median of at least five repetitions"
    import torch

    from lurk_beta_amd import store_hasher as SH

    assert torch.cuda.is_available(), "needs a device: there is nothing to measure without one"
    torch.cuda.set_device(0)
    res = {"tool": "store_resident_bench", "device": torch.cuda.get_device_name(0), "field": "pallas_fq",
           "method": "host clock around synchronising calls, 2 warm-ups, median (min, max) of %d" % args.reps}
    res["wide_dag_%d" % args.wide], store, rec = bench_dag("wide", SH.wide_dag(args.wide), args.reps)
    res["slot_preimages"] = bench_slots(store, rec, args.reps)
    store.close()
    res["list_dag_%d" % args.deep], store, _ = bench_dag("deep", SH.list_dag(args.deep), args.reps)
    store.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
