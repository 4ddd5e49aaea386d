"""Shared by the workloads: paths, the library profiler's per-kernel times, the cgroup CPU quota."""
from __future__ import annotations

import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def kernel_profile(lib, prefix):
    """(total ms, launches) of the profiler scopes whose name starts with `prefix` (HIP events on the launch stream, runtime.hip)"""
    from lurk_beta_amd import _lib

    tot, cnt = ctypes.c_double(), ctypes.c_uint64()
    _lib.check(lib.lurk_hip_profile_get(prefix.encode(), ctypes.byref(tot), ctypes.byref(cnt)))
    return tot.value, cnt.value


DUMP_LIMIT_BYTES = 64 << 20
DUMP_SAMPLE_ROWS = 1 << 16  # a larger output is dumped as this many rows at fixed, seeded positions


def field_limbs(values):
    """Field elements (ints < 2^256) -> float64 array (len, 8) of their 32-bit little-endian limbs (exact: every limb < 2^53)."""
    import numpy as np

    return np.array([[(int(v) >> (32 * k)) & 0xFFFFFFFF for k in range(8)] for v in values], dtype=np.float64).reshape(-1, 8)


def point_limbs(curve, jac):
    """A 96-byte Jacobian point -> (2, 8) float64: canonical affine x and y as 32-bit limbs (the identity is (0, 0)).  The Jacobian
    Z depends on the order of the additions, the point does not."""
    import lurk_beta_amd as L

    return field_limbs(L.point_to_affine(curve, jac))


def ints_flat(v):
    """A value made of field elements and affine points (ints, (x, y) tuples, None for the identity point, nested lists) -> flat list of ints"""
    if v is None:
        return [0, 0]
    if hasattr(v, "tolist"):  # numpy scalars and arrays
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        return [x for e in v for x in ints_flat(e)]
    return [int(v)]


def limb_rows(name, rows):
    """(m, 4) uint64 field elements (a torch tensor or numpy array) -> {name: (m, 8) float64 32-bit limbs}; above DUMP_SAMPLE_ROWS rows,
    the rows at DUMP_SAMPLE_ROWS fixed positions (seed 0, sorted) and those positions as {name}_index."""
    import numpy as np

    if hasattr(rows, "cpu"):
        rows = rows.cpu().numpy()
    rows = np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 4)
    out = {}
    if len(rows) > DUMP_SAMPLE_ROWS:
        idx = np.sort(np.random.default_rng(0).choice(len(rows), DUMP_SAMPLE_ROWS, replace=False))
        rows = rows[idx]
        out[name + "_index"] = idx.astype(np.float64)
    out[name] = rows.view(np.uint32).reshape(-1, 8).astype(np.float64)
    return out


def dump_outputs(dirname, arrays):
    """`--dump-outputs DIR`: write every {name: float32 / float64 array} to DIR/<name>.npy (at most DUMP_LIMIT_BYTES in all)."""
    import numpy as np

    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(dirname, name + ".npy"), a)


def cpu_quota_cores():
    """CPUs the cgroup lets this container use (cpu.max / cfs quota), or None."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fh:
            q = float(fh.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
            per = float(fh.read())
        return None if q <= 0 else q / per
    except Exception:
        return None


def cpu_leg_threads():
    """The thread count a cpu_baseline leg runs with, and the three numbers every leg reports beside its value (round 6: one helper
    for the headline and every sub-record).  A cgroup CPU quota caps the useful thread count whatever the host has (the GPU boxes
    show 256 logical CPUs under a 16-CPU quota): the OpenMP legs run with ceil(quota) threads, or every logical CPU without a quota.
    -> (threads, {"threads_used", "cpu_quota_cores", "host_cores"})"""
    import math

    quota = cpu_quota_cores()
    logical = os.cpu_count() or 1
    threads = max(1, min(logical, math.ceil(quota))) if quota else logical
    return threads, {"threads_used": threads, "cpu_quota_cores": quota, "host_cores": logical}


def cpu_leg_omp(threads):
    """Pin the oracle's OpenMP regions (oracle/oracle.c) to `threads` for a cpu_baseline leg."""
    from oracle import coracle as C

    C.lib().orc_set_num_threads(int(threads))
