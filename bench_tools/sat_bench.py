#!/usr/bin/env python3
"""Times the satisfiability check and the existing R1CS kernels on the slot gadgets' real rows and on the synthetic step shape:
    python bench_tools/sat_bench.py [--rc 100] [--export DIR] [--variants]
    python bench_tools/sat_bench.py --import DIR [--rc 100]
Default mode builds the slot shape of `rc` frames at eval_step's slot counts on Pallas Fq (lurk_hip_frames_r1cs_create), traces a W for
it (lurk_hip_frames_witness_dev) and times lurk_hip_r1cs_is_sat_dev beside multiply_vec, cross_term and cross_term_cached, on that shape
and on bench_workloads/fold_step.py's synthetic one.  HIP events around each call, median of 30 after 3 warm-ups, three repetitions.
--export DIR writes the slot shape's CSR (coefficients as a dictionary + ids) and the traced z as .npy.
--import DIR creates the shape from those files through plain lurk_hip_r1cs_create and times only multiply_vec, cross_term and
cross_term_cached: in that mode the script touches nothing newer than those calls, so a copy of it runs unchanged inside a checkout of an
older commit with that commit's own build (the A/B of is_sat against multiply_vec + the host's own comparison).
--variants also times is_sat's measurement switches (LURK_SAT_GROUP / LURK_SAT_LDS / LURK_SAT_LANE_MAX).
HBM fractions are of COMPULSORY bytes (8 B per non-zero, the per-row vectors, z once) over 8 TB/s."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lurk_beta_amd as L
from bench_workloads.fold_step import synth_r1cs_shape
from lurk_beta_amd import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--rc", type=int, default=100)
ap.add_argument("--export", dest="export_dir")
ap.add_argument("--import", dest="import_dir")
ap.add_argument("--variants", action="store_true")
args = ap.parse_args()
rc = args.rc
F = L.FIELD_PALLAS_FQ
q = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
NIO, GLOBALS, BODY = 6, 64, 1311
lib = _lib.load()


def timed(fn):
    """three repetitions of: 3 warm-ups, then the median of 30 HIP-event timings"""
    meds = []
    for _ in range(3):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        meds.append(ms[15])
    return meds


def report(label, name, meds, nnz, comp_bytes):
    med = sorted(meds)[1]
    print(f"{label:10s} {name:28s} medians {' '.join(f'{m:7.3f}' for m in meds)} ms   {med / nnz * 1e6:6.2f} ns per non-zero x 1e-3   "
          f"{comp_bytes / med / 8e7:5.1f} % of 8 TB/s on compulsory bytes", flush=True)


def describe(label, shape, lens):
    info = shape.info()
    nnz = sum(info["nnz"])
    print(f"{label}: {shape.num_cons} rows, {nnz} non-zeros ({nnz / max(shape.num_cons, 1):.1f} per row), longest row {int(lens.max()) if lens.size else 0}, "
          f"dictionary {info['distinct_coefficients']} coefficients, z {shape.num_cols} columns", flush=True)
    return nnz


def bench_parent_calls(label, shape, d_z, d_z2, nnz):
    """the calls every build has"""
    n, ncols = shape.num_cons, shape.num_cols
    s = torch.cuda.current_stream().cuda_stream
    out = [torch.empty((n, 4), dtype=torch.int64, device="cuda") for _ in range(3)]
    mv = lambda: _lib.check(lib.lurk_hip_r1cs_multiply_vec_dev(shape._h, _lib.ptr(d_z), *[_lib.ptr(o) for o in out], _lib.ptr(s)))
    report(label, "multiply_vec", timed(mv), nnz, nnz * 8.0 + n * (12 + 96.0) + ncols * 32.0)
    d_t = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    report(label, "cross_term", timed(lambda: shape.cross_term(d_z, d_z2, out=d_t)), nnz, nnz * 8.0 + n * (12 + 32.0) + 2 * ncols * 32.0)
    abc1 = shape.multiply_vec(d_z)
    u1 = d_z[shape.num_vars:shape.num_vars + 1].cpu().numpy().view(np.uint64)
    t_c, _ = shape.cross_term_cached(d_z2, abc1, u1)
    assert torch.equal(t_c, shape.cross_term(d_z, d_z2)), "cached and six-gather cross terms differ"
    report(label, "cross_term_cached", timed(lambda: shape.cross_term_cached(d_z2, abc1, u1)), nnz, nnz * 8.0 + n * (12 + 7 * 32.0) + ncols * 32.0)


def row_lens(mats):
    return np.maximum.reduce([np.diff(m[0].astype(np.int64)) for m in mats])


if args.import_dir:
    d = args.import_dir
    coeffs = np.load(os.path.join(d, "coeffs.npy"))
    mats = [(np.load(os.path.join(d, f"{w}_indptr.npy")), np.load(os.path.join(d, f"{w}_indices.npy")).astype(np.uint64), coeffs[np.load(os.path.join(d, f"{w}_ids.npy"))])
            for w in "abc"]
    dims = np.load(os.path.join(d, "dims.npy"))
    shape = L.R1CSShape(F, int(dims[0]), int(dims[1]), int(dims[2]), *mats)
    nnz = describe("slot shape (imported)", shape, row_lens(mats))
    del mats
    d_z = torch.from_numpy(np.load(os.path.join(d, "z.npy")).view(np.int64)).cuda()
    d_z2 = torch.from_numpy(np.load(os.path.join(d, "z2.npy")).view(np.int64)).cuda()
    bench_parent_calls("slot", shape, d_z, d_z2, nnz)
    shape.close()
else:
    from lurk_beta_amd.witness import SLOT_ORDER, STEP_SLOT_COUNTS, MultiFrameWitness, slot_constraints

    mf = MultiFrameWitness(F, rc, GLOBALS, BODY)
    shape = mf.r1cs(NIO)

    def traced(seed):
        pre = {name: synth.scalars(F, seed + st, 1, rc * STEP_SLOT_COUNTS[name] * st, mont=True) for name, st in SLOT_ORDER if STEP_SLOT_COUNTS[name]}
        d = synth.scalars(F, seed + 20, 1, mf.w_len + 1 + NIO, mont=True)
        mf.assemble(d, pre, mont=True)
        one = (1 << 256) % q  # u = 1, Montgomery
        d[mf.w_len] = torch.from_numpy(np.array([(one >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64).view(np.int64)).cuda()
        torch.cuda.synchronize()
        return d

    d_z, d_z2 = traced(40), traced(70)
    # the same matrix on the host (one frame's rows relocated frame by frame), for the row statistics and --export
    frame = []
    for w in range(3):
        ip, ix, ids, at = [np.zeros(1, np.uint64)], [], [], 0
        for name, st in SLOT_ORDER:
            m = slot_constraints(F, st)[w]
            size = mf.sizes[name]
            for _ in range(STEP_SLOT_COUNTS[name]):
                ix.append(np.where(m[1] == size, np.uint64(1 << 40), m[1] + np.uint64(at)))
                ids.append(m[2])
                ip.append(m[0][1:] + ip[-1][-1])
                at += size
        frame.append((np.concatenate(ip), np.concatenate(ix), np.concatenate(ids)))
    lens = np.tile(np.maximum.reduce([np.diff(m[0].astype(np.int64)) for m in frame]), rc)
    nnz = describe("slot shape", shape, lens)
    hist = np.bincount(np.minimum(lens, 256), minlength=257)
    print(f"rows by their longest combination: <= 8: {int(hist[:9].sum())}, 9-32: {int(hist[9:33].sum())}, 33-96: {int(hist[33:97].sum())}, > 96: {int(hist[97:].sum())}", flush=True)
    got = shape.is_sat(d_z)
    assert got == (0, shape.num_cons), got
    if args.export_dir:
        os.makedirs(args.export_dir, exist_ok=True)
        allc = np.concatenate([m[2] for m in frame])
        coeffs, inv = np.unique(allc, axis=0, return_inverse=True)
        inv = inv.reshape(-1).astype(np.uint32)
        np.save(os.path.join(args.export_dir, "coeffs.npy"), coeffs)
        at = 0
        for w, (ip, ix, dv) in zip("abc", frame):
            k = ix.size
            one = ix == np.uint64(1 << 40)
            cols = (GLOBALS + np.arange(rc, dtype=np.uint64)[:, None] * np.uint64(mf.frame_len) + ix[None, :])
            cols[:, one] = mf.w_len
            np.save(os.path.join(args.export_dir, f"{w}_indices.npy"), cols.reshape(-1).astype(np.uint32))
            np.save(os.path.join(args.export_dir, f"{w}_ids.npy"), np.tile(inv[at:at + k], rc))
            np.save(os.path.join(args.export_dir, f"{w}_indptr.npy"), np.concatenate([np.zeros(1, np.uint64), (np.arange(rc, dtype=np.uint64)[:, None] * np.uint64(k) + ip[None, 1:]).reshape(-1)]))
            at += k
        np.save(os.path.join(args.export_dir, "dims.npy"), np.array([shape.num_cons, shape.num_vars, shape.num_io], dtype=np.uint64))
        np.save(os.path.join(args.export_dir, "z.npy"), d_z.cpu().numpy().view(np.uint64))
        np.save(os.path.join(args.export_dir, "z2.npy"), d_z2.cpu().numpy().view(np.uint64))
        print("exported to", args.export_dir, flush=True)

    def bench_is_sat(label, sh, z, e, n_nnz, tag=""):
        comp = n_nnz * 8.0 + sh.num_cons * (16 + (32.0 if e is not None else 0)) + sh.num_cols * 32.0
        report(label, "is_sat" + (" (relaxed, E)" if e is not None else "") + tag, timed(lambda: sh.is_sat(z, e)), n_nnz, comp)

    d_e = torch.zeros((shape.num_cons, 4), dtype=torch.int64, device="cuda")
    bench_is_sat("slot", shape, d_z, None, nnz)
    bench_is_sat("slot", shape, d_z, d_e, nnz)
    bench_parent_calls("slot", shape, d_z, d_z2, nnz)
    if args.variants:
        for env in ({"LURK_SAT_GROUP": "8"}, {"LURK_SAT_GROUP": "16"}, {"LURK_SAT_LDS": "1"}, {"LURK_SAT_LDS": "1", "LURK_SAT_GROUP": "8"}, {"LURK_SAT_LANE_MAX": "4"},
                    {"LURK_SAT_LANE_MAX": "16"}, {"LURK_SAT_LANE_MAX": "96"}, {"LURK_SAT_MID_MAX": "32"}):
            os.environ.update(env)
            assert shape.is_sat(d_z) == (0, shape.num_cons)
            bench_is_sat("slot", shape, d_z, None, nnz, " " + ",".join(f"{k[9:]}={v}" for k, v in env.items()))
            for k in env:
                del os.environ[k]
    shape.close()
    del d_z, d_z2, d_e
# today's synthetic shape (bench_tools/fold_bench.py's), in both modes
n_w, n_t = 8951 * rc + 64, 10973 * rc
mats = synth_r1cs_shape(F, q, n_t, n_w, NIO)
shape = L.R1CSShape(F, n_t, n_w, NIO, *mats)
nnz = describe("synthetic shape", shape, row_lens(mats))
del mats
d_z = synth.scalars(F, 1, 1, n_w + 1 + NIO, mont=True)
d_z2 = synth.scalars(F, 6, 1, n_w + 1 + NIO, mont=True)
if not args.import_dir:
    # a random z satisfies nothing: E := A z o B z - u C z makes it a satisfied relaxed instance (cross_term(z, z) = 2 E, folded with 1 / 2)
    half = pow(2, -1, q) * (1 << 256) % q
    d_e = L.fold_vec(F, torch.zeros((n_t, 4), dtype=torch.int64, device="cuda"), shape.cross_term(d_z, d_z),
                     np.array([(half >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64))
    assert shape.is_sat(d_z, d_e) == (0, n_t)
    bench_is_sat("synthetic", shape, d_z, d_e, nnz)
    assert shape.is_sat(d_z)[0] > n_t // 2
    bench_is_sat("synthetic", shape, d_z, None, nnz, " EVERY ROW FAILING")
bench_parent_calls("synthetic", shape, d_z, d_z2, nnz)
if args.variants and not args.import_dir:
    os.environ["LURK_SAT_LDS"] = "1"
    bench_is_sat("synthetic", shape, d_z, d_e, nnz, " LDS=1")
    del os.environ["LURK_SAT_LDS"]
shape.close()
