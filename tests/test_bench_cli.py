"""bench.py's command line: the launcher contract (`--gpus N` must either find N ranks or make them), the argument checks and `--dump-outputs`."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_a_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stdout + out.stderr)


def test_bench_gpus_flag_is_read():
    """With --gpus 2 and no WORLD_SIZE the script re-executes itself under torch.distributed.run (two ranks); here,
    without a GPU, those ranks fail - but they must have been started."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--log-n", "10", "--steps", "1",
                          "--warmup", "0", "--no-cpu-baseline", "--pmc", "off"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    import torch

    if not torch.cuda.is_available():
        assert out.returncode != 0
        assert "local_rank" in out.stderr or "rank" in out.stderr.lower()  # torch.distributed.run's failure report names the ranks


def test_bench_refuses_zero_steps():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode != 0 and "--steps must be at least 1" in out.stderr, out.stderr


def test_dumped_field_limbs_are_exact():
    import numpy as np

    from bench_workloads.common import DUMP_SAMPLE_ROWS, field_limbs, ints_flat, limb_rows

    vals = [0, 1, (1 << 255) - 19, 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001]
    a = field_limbs(vals)
    assert a.dtype.name == "float64" and a.shape == (4, 8)
    assert [sum(int(x) << (32 * k) for k, x in enumerate(row)) for row in a] == vals
    assert ints_flat([[5, 6], None, (7, 8), np.uint64(9)]) == [5, 6, 0, 0, 7, 8, 9]
    rows = np.array([[v >> (64 * k) & ((1 << 64) - 1) for k in range(4)] for v in vals], dtype=np.uint64)
    assert np.array_equal(limb_rows("x", rows)["x"], a)
    # above the sample size: the same seeded positions on every call, the rows at those positions, the positions beside them
    big = np.arange(4 * (DUMP_SAMPLE_ROWS + 5), dtype=np.uint64).reshape(-1, 4)
    s1, s2 = limb_rows("y", big), limb_rows("y", big)
    idx = s1["y_index"].astype(np.int64)
    assert np.array_equal(s1["y_index"], s2["y_index"]) and len(idx) == DUMP_SAMPLE_ROWS and np.all(np.diff(idx) > 0)
    assert np.array_equal(s1["y"], big[idx].view(np.uint32).reshape(-1, 8).astype(np.float64))


@pytest.mark.gpu
def test_bench_dumps_the_last_commitment(tmp_path):
    """`--dump-outputs DIR` writes the commitment of the last timed step: the oracle's MSM of the same synthetic inputs, and the
    same bytes from a second run."""
    import numpy as np

    from bench_workloads.common import field_limbs
    from oracle import coracle as C

    log_n = 12
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--log-n", str(log_n), "--steps", "3", "--warmup", "1", "--reps", "1",
                              "--no-cpu-baseline", "--pmc", "off", "--sub-records", "off", "--no-plain-leg", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        assert sorted(os.listdir(d)) == ["commitment.npy"]
        dumps.append(np.load(d / "commitment.npy"))
    n = 1 << log_n
    want = C.jac_to_affine(0, C.msm_pippenger(0, C.synth_bases(0, n), C.synth_scalars(1, 1, 0, n)))
    assert np.array_equal(dumps[0], field_limbs(want)) and np.array_equal(dumps[0], dumps[1])


@pytest.mark.gpu
@pytest.mark.parametrize("workload, extra", [("ntt", ["--log-n", "10"]), ("poseidon_tree", ["--log-n", "12"]), ("store_hydrate", []),
                                             ("fold_step", ["--rc", "100", "--secondary", "0"]), ("compress", ["--log-n", "14"])])
def test_bench_dumps_every_workload(tmp_path, workload, extra):
    """`--dump-outputs DIR` on the other workloads: the same files and bytes from two runs; the NTT (in place, so the last of
    warmup + steps transforms) and the tree root against the oracle."""
    import numpy as np

    from bench_workloads.common import limb_rows
    from oracle import coracle as C

    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                              "--pmc", "off", "--sub-records", "off", "--dump-outputs", str(d)] + extra, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    want_names = {"ntt": ["ntt"], "poseidon_tree": ["tree_nodes", "tree_root"], "store_hydrate": ["digests_deep", "digests_wide", "digests_wide_index"],
                  "fold_step": ["challenge", "comm_T", "comm_W2"]}.get(workload)
    names = sorted(dumps[0])
    assert names == want_names if want_names else names and all(n.startswith("proof_") for n in names), names
    assert sorted(dumps[1]) == names and all(np.array_equal(dumps[0][n], dumps[1][n]) and dumps[0][n].dtype == np.float64 for n in names)
    if workload == "ntt":
        x = C.synth_scalars(1, 3, 0, 1 << 10)
        for _ in range(3):
            x = C.ntt(1, x)
        assert np.array_equal(dumps[0]["ntt"], limb_rows("ntt", x)["ntt"])
    if workload == "poseidon_tree":
        root = np.asarray(C.poseidon_tree8(1, C.synth_scalars(1, 2, 0, 1 << 12))).reshape(-1)[:4]
        assert np.array_equal(dumps[0]["tree_root"], limb_rows("tree_root", root)["tree_root"])
