#!/usr/bin/env python3
"""The sixteen halving vectors 2^16 .. 2 of a 2^20 HyperKZG opening's first stage under a 2^20-point window-table key, on BN254 and Pallas:
as ONE batch (lurk_hip_msm_ctx_submit_batch_dev) and as sixteen lurk_hip_msm_ctx_submit_dev calls, six in flight.  One process, one device.

Method of msm_curve_bench.py: warm-up, then the median of five regions (synchronize, `steps` rounds, synchronize), the two forms
alternating region by region.  The results of the two forms are compared byte for byte in every round.  Prints one JSON line; --out
writes the same record to a file.

    python bench_tools/msm_batch_bench.py [--log-n 20] [--steps 5] [--regions 5] [--warmup 2] [--out profiles/rNN_msm_batch.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOTS = 6
CURVES = {"bn254": (2, 2), "pallas": (0, 1)}  # curve id, scalar field id


def bench_curve(name, args):
    import torch

    from lurk_beta_amd import CommitmentKey, synth

    curve, field = CURVES[name]
    n = 1 << args.log_n
    key = CommitmentKey(curve, synth.bases(curve, n), n=n, precompute=True, device=True)
    key.reserve(1 << 16, SLOTS)
    lens = [(1 << 16) >> k for k in range(16)]
    offs = [sum(lens[:k]) for k in range(16)]
    d_s = synth.scalars(field, 17, 0, sum(lens), mont=True)
    torch.cuda.synchronize()

    def batch():
        key.submit_batch_device(0, d_s, offs, lens, is_mont=True)
        return key.wait_batch(0, 16)

    def one_by_one():
        out = np.zeros((16, 12), dtype=np.uint64)
        for k in range(16):
            slot = k % SLOTS
            if k >= SLOTS:
                out[k - SLOTS] = key.wait(slot)
            key.submit_device(slot, d_s[offs[k]:], lens[k], is_mont=True)
        for k in range(16 - SLOTS, 16):
            out[k] = key.wait(k % SLOTS)
        return out

    def region(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = [fn() for _ in range(steps)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps, got

    want = one_by_one()
    region(batch, args.warmup)
    region(one_by_one, args.warmup)
    t_batch, t_single = [], []
    for _ in range(args.regions):
        dt, got = region(batch, args.steps)
        assert all(np.array_equal(g, want) for g in got), "the batch differs from the sixteen commitments"
        t_batch.append(dt)
        dt, got = region(one_by_one, args.steps)
        assert all(np.array_equal(g, want) for g in got)
        t_single.append(dt)
    # the two accumulation forms of the batch, each forced (LURK_MSM_BATCH_PLANNED is read at each call), alternating
    forms = {"0": [], "1": []}
    for form in forms:
        os.environ["LURK_MSM_BATCH_PLANNED"] = form
        region(batch, args.warmup)
    for _ in range(args.regions):
        for form, ts in forms.items():
            os.environ["LURK_MSM_BATCH_PLANNED"] = form
            dt, got = region(batch, args.steps)
            assert all(np.array_equal(g, want) for g in got), "the batch differs from the sixteen commitments"
            ts.append(dt)
    os.environ.pop("LURK_MSM_BATCH_PLANNED")
    info = key.info()
    key.close()
    return {"window_bits": info["window_bits"], "key_form": info["form"], "batch_ms": round(statistics.median(t_batch), 4),
            "batch_ms_by_region": [round(v, 4) for v in t_batch], "sixteen_submits_ms": round(statistics.median(t_single), 4),
            "sixteen_submits_ms_by_region": [round(v, 4) for v in t_single],
            "batch_direct_ms": round(statistics.median(forms["0"]), 4), "batch_direct_ms_by_region": [round(v, 4) for v in forms["0"]],
            "batch_planned_ms": round(statistics.median(forms["1"]), 4), "batch_planned_ms_by_region": [round(v, 4) for v in forms["1"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    out = {"tool": "msm_batch_bench", "device": torch.cuda.get_device_name(0), "log_n": args.log_n, "vectors": "2^16 .. 2 (sixteen)", "steps": args.steps,
           "regions": args.regions, "warmup": args.warmup, "results_equal": "every round, byte for byte"}
    for name in CURVES:
        out[name] = bench_curve(name, args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
