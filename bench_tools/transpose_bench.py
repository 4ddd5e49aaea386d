#!/usr/bin/env python3
"""Times the two ways to the transposed shape the compressing provers need, in one process, on two shapes:
    python bench_tools/transpose_bench.py [--log-n 20] [--rc 100] [--reps 5]
(a) the host path as SpartanProver.__init__ runs it: lurk_beta_amd.spartan.transpose_csr of the three host CSR matrices (numpy), then a second
    R1CSShape(...) creation (lurk_hip_r1cs_create: every coefficient hashed into the dictionary, 8 B per entry uploaded) - the two parts
    timed apart with the host clock (the creation ends in synchronous copies);
(b) R1CSShape.transposed(2 * num_vars) (lurk_hip_r1cs_transpose_dev) - HIP events on the stream around the call, and the host clock
    around it (the call synchronises once).
Shapes: the compressing benchmark's 2^log_n x 2^log_n instance (bench_workloads/compress.py's matrices, same seed) and the slot shape of
rc frames at eval_step's slot counts (lurk_hip_frames_r1cs_create; its host CSR is read back with lurk_hip_r1cs_read).  One warm-up of
each path, then the median of --reps.  The two results are compared entry for entry before anything is timed.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lurk_beta_amd as L
from lurk_beta_amd import _lib
from lurk_beta_amd.spartan import transpose_csr

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, default=20)
ap.add_argument("--rc", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
F, q = L.FIELD_PALLAS_FQ, 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
lib = _lib.load()


def compress_mats(log_n):
    """bench_workloads/compress.py's A, B, C"""
    nc = nv = 1 << log_n
    nfree, nio = nv - nc // 2, 6
    rng = np.random.default_rng(11)
    R = (1 << 256) % q
    tab = np.array([[(v * R % q) >> (64 * w) & 0xFFFFFFFFFFFFFFFF for w in range(4)] for v in (1, q - 1, 2, 3, 1 << 16, q - 7)], dtype=np.uint64)
    rows_p = nc // 2

    def rand_mat():
        cnt = np.zeros(nc, dtype=np.uint64)
        cnt[:rows_p] = rng.integers(2, 5, rows_p)
        indptr = np.zeros(nc + 1, dtype=np.uint64)
        np.cumsum(cnt, out=indptr[1:])
        nnz = int(indptr[-1])
        cols = rng.integers(0, nfree + 1 + nio, nnz)
        cols = np.where(cols >= nfree, cols - nfree + nv, cols).astype(np.uint64)
        return indptr, cols, np.ascontiguousarray(tab[rng.integers(0, len(tab), nnz)])

    A, B = rand_mat(), rand_mat()
    ip = np.zeros(nc + 1, dtype=np.uint64)
    ip[1:rows_p + 1] = np.arange(1, rows_p + 1, dtype=np.uint64)
    ip[rows_p + 1:] = rows_p
    Cm = (ip, (nfree + np.arange(rows_p)).astype(np.uint64), np.tile(tab[0], (rows_p, 1)))
    return [A, B, Cm], nc, nv, nio


def median(xs):
    return sorted(xs)[len(xs) // 2]


def bench(label, shape, mats):
    nc, nv = shape.num_cons, shape.num_vars
    rows_t = 2 * nv
    nnz = shape.info()["nnz"]
    # both paths once: the warm-up, and the check that they agree
    host_t = [transpose_csr(*m, rows_t) for m in mats]
    up = L.R1CSShape(F, rows_t, nc - 1, 0, *host_t)
    dev = shape.transposed(rows_t)
    assert dev.info() == up.info()
    for w in range(3):
        for a, b in zip(dev.read(w), up.read(w)):
            assert np.array_equal(a, b), (label, w)
    up.close()
    dev.close()
    t_csr, t_create, t_dev_ev, t_dev_wall = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        host_t = [transpose_csr(*m, rows_t) for m in mats]
        t1 = time.perf_counter()
        up = L.R1CSShape(F, rows_t, nc - 1, 0, *host_t)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        t_csr.append((t1 - t0) * 1e3)
        t_create.append((t2 - t1) * 1e3)
        up.close()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        dev = shape.transposed(rows_t)
        b.record()
        torch.cuda.synchronize()
        t_dev_wall.append((time.perf_counter() - t0) * 1e3)
        t_dev_ev.append(a.elapsed_time(b))
        dev.close()
    released = ctypes.c_size_t()
    _lib.check(lib.lurk_hip_scratch_trim(ctypes.byref(released)))
    out = {"shape": label, "num_cons": nc, "num_vars": nv, "rows_t": rows_t, "nnz": list(nnz), "distinct_coefficients": shape.info()["distinct_coefficients"],
           "host_transpose_csr_ms": round(median(t_csr), 3), "host_r1cs_create_ms": round(median(t_create), 3),
           "device_transpose_ms_events": round(median(t_dev_ev), 3), "device_transpose_ms_wall": round(median(t_dev_wall), 3),
           "create_over_device": round(median(t_create) / median(t_dev_ev), 1), "host_path_over_device": round((median(t_csr) + median(t_create)) / median(t_dev_ev), 1),
           "entry_bytes_largest_matrix": 8 * max(nnz), "scratch_arena_bytes": released.value, "all_device_ms_events": [round(x, 3) for x in t_dev_ev]}
    print(f"{label}: transpose_csr {out['host_transpose_csr_ms']} ms + r1cs_create {out['host_r1cs_create_ms']} ms on the host path; "
          f"transposed() {out['device_transpose_ms_events']} ms (events), {out['device_transpose_ms_wall']} ms (host clock)", flush=True)
    return out


results = []
mats, nc, nv, nio = compress_mats(args.log_n)
shape = L.R1CSShape(F, nc, nv, nio, *mats)
results.append(bench(f"compress 2^{args.log_n} x 2^{args.log_n}", shape, mats))
shape.close()
del mats

from lurk_beta_amd.witness import MultiFrameWitness

mf = MultiFrameWitness(F, args.rc, 64, 1311)
shape = mf.r1cs(6)
mats = [shape.read(w) for w in range(3)]
results.append(bench(f"slot rows, rc = {args.rc}", shape, mats))
shape.close()
print(json.dumps({"transpose_bench": results, "reps": args.reps, "device": torch.cuda.get_device_name(0)}))
