"""CPU-only: the slot-descriptor rule of the resident store (``store_resident.slot_elems`` = allocate_slot's rule,
/root/reference/src/lem/circuit.rs:265-308) against hand-written expectations for every slot type, the new entry points declared and bound
under the unchanged ABI revision, and - without a device - the handle's constructor failing loudly."""
import ctypes
import os
import re

import numpy as np
import pytest

from lurk_beta_amd import store_resident as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, T, D, K = SR.SLOT_ELEM_ZERO, SR.SLOT_ELEM_TAG, SR.SLOT_ELEM_DIGEST, SR.SLOT_ELEM_CONST


def _rows(*pairs):
    return np.array(pairs, dtype=np.uint32).reshape(-1, 2)


def test_slot_elems_every_slot_type_by_hand():
    # hash4: two pointers; then a dummy slot; then pointer + num + boolean (tag, digest | digest | const)
    got = SR.slot_elems("hash4", [[("ptr", 5), ("ptr", 9)], None, [("ptr", 2), ("num", 7), ("bool", True)]])
    assert got.dtype == np.uint32 and got.shape == (12, 2)
    assert np.array_equal(got, _rows((T, 5), (D, 5), (T, 9), (D, 9), (Z, 0), (Z, 0), (Z, 0), (Z, 0), (T, 2), (D, 2), (D, 7), (K, 1)))
    # hash6: three pointers
    assert np.array_equal(SR.slot_elems("hash6", [[("ptr", 1), ("ptr", 0), ("ptr", 4)]]), _rows((T, 1), (D, 1), (T, 0), (D, 0), (T, 4), (D, 4)))
    # hash8: four pointers, and a mix that fills eight elements: ptr, num, bool(False), bool, ptr, num
    assert np.array_equal(SR.slot_elems("hash8", [[("ptr", k) for k in (3, 2, 1, 0)]]), _rows((T, 3), (D, 3), (T, 2), (D, 2), (T, 1), (D, 1), (T, 0), (D, 0)))
    assert np.array_equal(SR.slot_elems(8, [[("ptr", 6), ("num", 6), ("bool", 0), ("bool", 1), ("ptr", 8), ("num", 1)]]),
                          _rows((T, 6), (D, 6), (D, 6), (K, 0), (K, 1), (T, 8), (D, 8), (D, 1)))
    # commitment: the secret as a num, then the payload pointer; a dummy commitment slot is three zeros
    assert np.array_equal(SR.slot_elems("commitment", [[("num", 11), ("ptr", 12)], None]), _rows((D, 11), (T, 12), (D, 12), (Z, 0), (Z, 0), (Z, 0)))
    # bit_decomp: one num; its dummy is one zero
    assert np.array_equal(SR.slot_elems("bit_decomp", [[("num", 4)], None, [("bool", True)]]), _rows((D, 4), (Z, 0), (K, 1)))
    # no slots at all
    assert SR.slot_elems("hash4", []).shape == (0, 2)
    # the class offers the same function
    assert np.array_equal(SR.DeviceStore.slot_elems("hash6", [None]), _rows(*[(Z, 0)] * 6))


def test_slot_elems_refuses_a_wrong_element_count_and_unknown_things():
    with pytest.raises(ValueError, match="slot 1: 3 preimage elements, a hash4 slot takes 4"):
        SR.slot_elems("hash4", [None, [("ptr", 1), ("num", 2)]])
    with pytest.raises(ValueError, match="slot 0: 6 preimage elements"):
        SR.slot_elems("hash4", [[("ptr", 1), ("ptr", 2), ("ptr", 3)]])
    with pytest.raises(ValueError, match="slot 0: 2 preimage elements, a bit_decomp slot takes 1"):
        SR.slot_elems("bit_decomp", [[("ptr", 1)]])
    with pytest.raises(ValueError, match="unknown value kind"):
        SR.slot_elems("hash4", [[("sym", 1)]])
    with pytest.raises(ValueError, match="unknown slot type"):
        SR.slot_elems("hash5", [])
    with pytest.raises(ValueError, match="32 bits"):
        SR.slot_elems("bit_decomp", [[("num", 1 << 32)]])


def test_the_entry_points_are_declared_and_bound_under_abi_4():
    from lurk_beta_amd import DeviceStore, _lib

    assert DeviceStore is SR.DeviceStore
    hdr = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    assert re.search(r"#define LURK_HIP_ABI_VERSION 4\b", hdr)
    lib = _lib.load()
    assert lib.lurk_hip_abi_version() == 4
    for name, nargs in (("lurk_hip_store_create", 3), ("lurk_hip_store_destroy", 1), ("lurk_hip_store_info", 7), ("lurk_hip_store_append", 7),
                        ("lurk_hip_store_digests_dev", 5), ("lurk_hip_store_digests", 4), ("lurk_hip_store_slot_preimages_dev", 6)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    # the descriptor is two 32-bit words, as the header declares it and the kernel reads it
    assert ctypes.sizeof(_lib.SlotElemStruct) == 8 and [f[0] for f in _lib.SlotElemStruct._fields_] == ["kind", "arg"]
    for name, val in (("ZERO", 0), ("TAG", 1), ("DIGEST", 2), ("CONST", 3)):
        assert re.search(r"#define LURK_SLOT_ELEM_%s %d\b" % (name, val), hdr) and getattr(SR, "SLOT_ELEM_" + name) == val
    # host-only calls on a null handle are refused, not crashed on; destroy(NULL) is a no-op
    assert lib.lurk_hip_store_info(None, None, None, None, None, None, None) != 0 and b"null store handle" in lib.lurk_hip_last_error()
    assert lib.lurk_hip_store_destroy(None) == 0


def test_create_fails_loudly_without_a_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from lurk_beta_amd import LurkHipError

    with pytest.raises(LurkHipError, match="no CPU fallback"):
        SR.DeviceStore(1)
    with pytest.raises(LurkHipError, match="no CPU fallback"):
        SR.DeviceStore(7)  # the device comes first, as for every compute entry point
