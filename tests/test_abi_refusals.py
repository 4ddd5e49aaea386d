"""Refusals behind the C ABI, pinned row by row to recorded answers (tests/abi_refusals.py, tests/golden/abi_refusals_*.json): an unknown
field or curve id, a field or curve the entry point does not serve, a canonical scalar that is not reduced, and which of several bad
arguments is named.  The rows were recorded from the build before the entry points moved to the shared dispatch and error boundary
(dispatch.hpp, host_guarded); the library must answer with the same return code, message and outputs."""
import json

import pytest

from tests import abi_refusals as T


def _check(which, cases):
    from lurk_beta_amd import _lib

    lib = _lib.load()
    golden = T.load_golden(which)
    assert len(golden) == len(cases), "the recorded rows and the table of cases have drifted apart"
    wrong = []
    for name, args in cases:
        want = golden[(name, json.dumps(T._jsonable(args)))]
        got = T.replay(lib, name, args)
        if got != want:
            wrong.append((want, got))
    assert not wrong, "\n".join(f"recorded {w}\n     got {g}" for w, g in wrong)


def test_host_entry_points_refuse_as_recorded():
    """CPU-only: every host-only entry point, lurk_hip_sumcheck_verify, lurk_hip_hyperkzg_pairing_inputs, the slot circuits' sizes and the
    transcript calls."""
    assert all(r["rc"] != 0 or 0 in r["outs"] for r in T.load_golden("host").values())  # the table holds refusals only
    _check("host", T.HOST_CASES)


@pytest.mark.gpu
def test_device_entry_points_refuse_as_recorded():
    """With a device: the entry points whose field / curve dispatch is shared, NULL or tiny host buffers only; every row is refused before
    a kernel is launched."""
    assert all(r["rc"] != 0 for r in T.load_golden("device").values())
    _check("device", T.DEVICE_CASES)
