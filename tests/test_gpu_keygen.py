"""f4: commitment-key generation on the device (SHAKE256 on the host, BLAKE2b / SWU / isogeny per lane) against the oracle's
restatement of arecibo's from_label + pasta_curves' hash_to_curve (oracle/keygen_ref.py; constants pinned mathematically, primitives
by hashlib; no key bytes exist upstream)."""
import numpy as np
import pytest

from oracle import coracle as C
from oracle import keygen_ref as K
from oracle import pyref as R

pytestmark = pytest.mark.gpu
CURVES = [("pallas", 0), ("vesta", 1)]


def _pts(c, arr):
    bf = 0 if c == 0 else 1
    out = []
    for row in np.ascontiguousarray(arr).reshape(-1, 8):
        x, y = C.limbs_to_ints(C.from_mont(bf, row.reshape(2, 4)))
        out.append(None if (x, y) == (0, 0) else (x, y))
    return out


@pytest.mark.parametrize("cn,c", CURVES)
def test_from_label_matches_the_oracle(hip, cn, c):
    from lurk_beta_amd.msm import ck_from_label

    n = 300
    got = _pts(c, ck_from_label(c, b"ck", n).cpu().numpy().view(np.uint64))
    assert got == K.from_label(cn, b"ck", n)
    other = _pts(c, ck_from_label(c, b"other label", 5).cpu().numpy().view(np.uint64))
    assert other == K.from_label(cn, b"other label", 5) and other[0] != got[0]
    assert ck_from_label(c, b"ck", 0).shape[0] == 0


@pytest.mark.parametrize("cn,c", CURVES)
def test_hash_to_curve_with_another_domain_and_edge_strings(hip, cn, c):
    import torch

    from lurk_beta_amd import _lib

    msgs = [bytes(32), b"\xff" * 32, bytes(range(32))] + [bytes([i]) * 32 for i in range(1, 30)]
    d_in = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).cuda()
    out = torch.empty((len(msgs), 8), dtype=torch.int64, device="cuda")
    _lib.check(_lib.load().lurk_hip_ck_hash_to_curve_dev(c, b"z.cash:test", _lib.ptr(d_in), len(msgs), _lib.ptr(out), None))
    torch.cuda.synchronize()
    assert _pts(c, out.cpu().numpy().view(np.uint64)) == [K.hash_to_curve(cn, b"z.cash:test", m) for m in msgs]


def test_generated_key_commits(hip):
    """A key generated in place (no host copy) commits to the same point as the oracle's MSM over the oracle's key; 2^16 generated
    points all lie on the curve; the table form agrees."""
    from lurk_beta_amd import CommitmentKey, point_to_affine
    from lurk_beta_amd.msm import ck_from_label

    n = 200
    key = K.from_label("pallas", b"ck", n)
    s = C.limbs_to_ints(C.synth_scalars(1, 180, 1, n))
    want = R.msm_naive("pallas", s, key)
    for pre in (False, True):
        ck = CommitmentKey.from_label(0, b"ck", n, precompute=pre)
        assert point_to_affine(0, ck.commit(C.ints_to_limbs(s))) == want
        ck.close()
    big = ck_from_label(0, b"ck", 1 << 16).cpu().numpy().view(np.uint64)
    assert C.on_curve(0, big) and _pts(0, big[:n]) == key


# ---- the device entry points under moved parameter blocks ---------------------------------------------------------------------
# tests/test_params.py moves lurk_hip_ck_params through the host compilation of the per-point map only; here the device compilation
# runs under the same moves.  The longest tag ck_params_validate admits is 62 bytes; with 62 bytes per point the first BLAKE2b
# message is exactly 256 bytes (two full blocks) and the other two exactly 128 (one full block).
CK_MOVES_DEV = [dict(bytes_per_point=1), dict(bytes_per_point=31), dict(bytes_per_point=33), dict(bytes_per_point=64), dict(xof=1),
                dict(curve_name_pallas="Pallas", curve_name_vesta="Vesta")]
CK_MOVE_REFUSED = dict(domain_prefix="p" * 31, suite="s" * 30)  # the from_label tag would be 31 + 1 + 6 + 30 = 68 bytes

MOVES_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from lurk_beta_amd import LurkHipError, params as P
from lurk_beta_amd.msm import ck_from_label
from oracle import coracle as C
from oracle import keygen_ref as K

def pts(c, arr):
    out = []
    for row in np.ascontiguousarray(arr).reshape(-1, 8):
        x, y = C.limbs_to_ints(C.from_mont(c, row.reshape(2, 4)))
        out.append(None if (x, y) == (0, 0) else (x, y))
    return out

n = 130
P.ck_params_set()
try:
    P.ck_params_set(**%(refused)r)
    print("ACCEPTED the 68-byte tag")
except LurkHipError as e:
    assert "do not fit two BLAKE2b blocks" in str(e), e
    assert P.ck_params_get() == K.CK_DEFAULTS
    print("REFUSED")
for mv in %(moves)r:
    P.ck_params_set()
    assert P.ck_params_set(**mv) == {**K.CK_DEFAULTS, **mv}
    for cn, c in (("pallas", 0), ("vesta", 1)):
        dev = pts(c, ck_from_label(c, b"ck", n).cpu().numpy().view(np.uint64))
        host = pts(c, P.ck_from_label_host(c, b"ck", n))
        want = K.from_label(cn, b"ck", n, params=mv)
        assert len(dev) == len(host) == len(want) == n
        assert dev == want, ("device", mv, cn, [i for i in range(n) if dev[i] != want[i]][:4])
        assert host == want, ("host", mv, cn, [i for i in range(n) if host[i] != want[i]][:4])
        print("AGREE", cn, sorted(mv.items()), flush=True)
print("DONE", flush=True)
"""


def test_from_label_on_the_device_under_moved_parameter_blocks(hip):
    """In a child process (the block is process-wide): under every admissible move lurk_hip_ck_from_label_dev,
    lurk_hip_ck_from_label_host and the oracle agree on 130 points of both curves; the move whose tag is too long is refused."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = MOVES_CHILD % dict(root=root, moves=CK_MOVES_DEV, refused=CK_MOVE_REFUSED)
    r = subprocess.run([sys.executable, "-c", child], cwd=root, capture_output=True, text=True, timeout=300)
    lines = r.stdout.strip().splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "DONE", f"child rc {r.returncode}\n{r.stdout[-600:]}\n{r.stderr[-1200:]}"
    assert lines[0] == "REFUSED"
    assert len([ln for ln in lines if ln.startswith("AGREE")]) == 2 * len(CK_MOVES_DEV)


def _longest_prefix(cn):
    prefix = "L" * (62 - 1 - len(cn) - len(K.CK_DEFAULTS["suite"]))
    assert len(prefix + "-" + cn + K.CK_DEFAULTS["suite"]) == 62
    return prefix.encode()


@pytest.mark.parametrize("cn,c", CURVES)
def test_hash_to_curve_dev_at_the_longest_tag_in_a_window_on_another_stream(hip, cn, c):
    """62-byte tag, 62 bytes per point: hashes of exactly 256 and exactly 128 bytes.  n around the 128-thread block, on a non-default
    stream, into a window that starts 64 bytes into a larger zeroed tensor: the points are the oracle's and the 64 bytes on either
    side of the window are still zero."""
    import random

    import torch

    from lurk_beta_amd import _lib
    from lurk_beta_amd import params as P

    sizes = [0, 1, 127, 128, 129, 300]
    rng = random.Random("longest tag " + cn)
    msgs = [bytes(62), b"\xff" * 62] + [rng.randbytes(62) for _ in range(max(sizes) - 2)]
    prefix = _longest_prefix(cn)
    want = [K.hash_to_curve(cn, prefix, m) for m in msgs]
    stream = torch.cuda.Stream()
    compared = 0
    with P.ck_params(bytes_per_point=62):
        for n in sizes:
            d_in = torch.frombuffer(bytearray(b"".join(msgs[:n]) or b"\0"), dtype=torch.uint8).cuda()
            buf = torch.zeros(64 + 64 * n + 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _lib.check(_lib.load().lurk_hip_ck_hash_to_curve_dev(c, prefix, _lib.ptr(d_in), n, _lib.ptr(buf.data_ptr() + 64), _lib.ptr(stream.cuda_stream)))
            stream.synchronize()
            raw = buf.cpu().numpy()
            assert not raw[:64].any() and not raw[64 + 64 * n:].any(), n
            got = _pts(c, raw[64:64 + 64 * n].copy().view(np.uint64))
            assert len(got) == n and got == want[:n], (n, [i for i in range(n) if got[i] != want[i]][:4])
            compared += n
    assert compared == sum(sizes)
    assert P.ck_params_get() == K.CK_DEFAULTS


@pytest.mark.parametrize("cn,c", CURVES)
def test_a_tag_one_byte_too_long_is_refused_and_the_next_call_works(hip, cn, c):
    import torch

    from lurk_beta_amd import LurkHipError, _lib
    from lurk_beta_amd import params as P
    from lurk_beta_amd.msm import ck_from_label

    prefix = _longest_prefix(cn) + b"L"
    d_in = torch.zeros(62, dtype=torch.uint8, device="cuda")
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    with P.ck_params(bytes_per_point=62):
        with pytest.raises(LurkHipError, match="do not fit two BLAKE2b blocks|too long"):
            _lib.check(_lib.load().lurk_hip_ck_hash_to_curve_dev(c, prefix, _lib.ptr(d_in), 1, _lib.ptr(out), None))
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()  # nothing ran
    assert _pts(c, ck_from_label(c, b"ck", 3).cpu().numpy().view(np.uint64)) == K.from_label(cn, b"ck", 3)
