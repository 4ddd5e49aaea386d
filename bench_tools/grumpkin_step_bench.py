#!/usr/bin/env python3
"""ms per folding step on Grumpkin at the secondary circuit's size, beside a Vesta context on a shape of the same dimensions and row
lengths, in one process on one MI355X:
    python bench_tools/grumpkin_step_bench.py [--steps 20] [--regions 3] [--out FILE]
A step is begin (commit W2, cross term, commit T) + finish(r) with the caller's r and a host witness, as the secondary half of
prove_step runs it; the two curves alternate region by region, the figure per curve is the median of the regions.  Both contexts fold
the SAME structure (M = 10 240 rows, 9 000 variables, 2 IO, every 64th row long) with coefficients and witnesses drawn from their own
field; keys are lurk_hip_synth_bases_dev's bases.  The first step's commitments are checked by the dlog checksum on Grumpkin."""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import lurk_beta_amd as L
from lurk_beta_amd import synth
from tests import bn254_ref as B

M, NV, NIO = 10240, 9000, 2
PALLAS_P = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001  # Vesta's scalar field (field id 0)


def structure(rng):
    """indptr / indices of A, B, C: 1-3 entries per row, every 64th row 40 entries in A"""
    ncols = NV + 1 + NIO
    out = []
    for w in range(3):
        indptr, indices = [0], []
        for i in range(M):
            k = 40 if (w == 0 and i % 64 == 0) else rng.randrange(1, 4)
            indices += sorted(rng.sample(range(ncols), k))
            indptr.append(len(indices))
        out.append((indptr, indices))
    return out


def to_mont(p, xs):
    return B.ints_to_limbs([(x << 256) % p for x in xs])


def make(curve, p, struct, rng):
    mats = [(ip, ix, to_mont(p, [rng.choice([1, 1, 2, p - 1, rng.randrange(1, p)]) for _ in ix])) for ip, ix in struct]
    shape = L.R1CSShape.for_curve(curve, M, NV, NIO, *mats)
    n = max(M, NV)
    key = L.CommitmentKey(curve, synth.bases(curve, n), n=n, device=True)
    return shape, key, L.FoldingContext(curve, shape, key)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = random.Random("grumpkin-step-bench")
    struct = structure(rng)
    sides = {}
    for name, curve, p in (("grumpkin", L.CURVE_GRUMPKIN, B.BN254_P), ("vesta", L.CURVE_VESTA, PALLAS_P)):
        shape, key, ctx = make(curve, p, struct, rng)
        w2 = [to_mont(p, [rng.randrange(p) for _ in range(NV)]) for _ in range(4)]  # four witnesses in turn
        x2 = to_mont(p, [rng.randrange(p) for _ in range(NIO)])
        r = to_mont(p, [rng.randrange(1 << 128)])
        sides[name] = dict(curve=curve, p=p, shape=shape, key=key, ctx=ctx, w2=w2, x2=x2, r=r, ms=[])
    g = sides["grumpkin"]
    cw, _ = g["ctx"].begin(g["w2"][0], g["x2"])
    g["ctx"].finish(g["r"])
    want = B.dlog_checksum_np(B.GRUMPKIN, B.ints_to_limbs(B.from_mont(g["p"], g["w2"][0])))
    assert B.from_xy(L.point_to_affine(L.CURVE_GRUMPKIN, cw)) == want, "commit(W2) on Grumpkin differs from the dlog checksum"

    def run(s, steps):
        for k in range(steps):
            s["ctx"].begin(s["w2"][k % 4], s["x2"])
            s["ctx"].finish(s["r"])
        s["ctx"].read()  # the folds of the last step are through

    for s in sides.values():
        run(s, a.warmup)
    for _ in range(a.regions):
        for s in sides.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(s, a.steps)
            s["ms"].append((time.perf_counter() - t0) * 1e3 / a.steps)
    med = {k: sorted(s["ms"])[len(s["ms"]) // 2] for k, s in sides.items()}
    res = {"rows": M, "num_vars": NV, "num_io": NIO, "steps": a.steps, "regions": a.regions, "device": torch.cuda.get_device_name(0),
           "grumpkin_ms_per_step": round(med["grumpkin"], 4), "vesta_ms_per_step": round(med["vesta"], 4),
           "ratio": round(med["grumpkin"] / med["vesta"], 3), "grumpkin_regions_ms": [round(x, 4) for x in sides["grumpkin"]["ms"]],
           "vesta_regions_ms": [round(x, 4) for x in sides["vesta"]["ms"]]}
    # where a step's time goes: the library's profiler over one more region per curve (kernel time by name)
    from lurk_beta_amd import _lib
    import ctypes

    lib = _lib.load()
    for k, s in sides.items():
        lib.lurk_hip_profile_enable(1)
        lib.lurk_hip_profile_reset()
        run(s, a.steps)
        prof = {}
        for prefix in (b"r1cs_cross_term", b"fold_vec", b"msm"):
            ms, n = ctypes.c_double(), ctypes.c_uint64()
            lib.lurk_hip_profile_get(prefix, ctypes.byref(ms), ctypes.byref(n))
            prof[prefix.decode()] = {"ms_per_step": round(ms.value / a.steps, 4), "launches_per_step": n.value / a.steps}
        lib.lurk_hip_profile_enable(0)
        res[k + "_kernel_ms"] = prof
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
