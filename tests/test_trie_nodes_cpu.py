"""CPU-only: the root-addressed trie calls (lurk_hip_trie_nodes_*) are declared in the header under the unchanged ABI revision, exported by
the library, bound with the header's arity, present in the generated Rust extern block and called with that arity by the Rust wrapper;
without a device every one of them returns the library's no-device error instead of crashing."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = {
    "lurk_hip_trie_nodes_create": ["ns", "field_id", "height", "reserve_nodes"],
    "lurk_hip_trie_nodes_destroy": ["ns"],
    "lurk_hip_trie_nodes_info": ["ns", "field_id", "height", "n_nodes", "slots", "device"],
    "lurk_hip_trie_nodes_register_dev": ["ns", "d_preimages", "count", "d_digests_out", "stream"],
    "lurk_hip_trie_nodes_add_trie": ["ns", "trie", "stream"],
    "lurk_hip_trie_nodes_get_dev": ["ns", "d_digests32", "m", "d_preimages", "d_found", "stream"],
    "lurk_hip_trie_nodes_prove_lookup_dev": ["ns", "d_roots32", "root_stride", "d_keys32", "m", "d_paths", "d_values32", "d_status", "n_missing", "stream"],
    "lurk_hip_trie_nodes_prove_insert_dev": ["ns", "d_roots32", "root_stride", "d_keys32", "d_new_values32", "m", "d_old_paths", "d_new_paths", "d_old_values32",
                                             "d_new_roots32", "d_status", "n_missing", "register_new", "stream"],
    "lurk_hip_trie_nodes_insert_chain_dev": ["ns", "root32_host", "d_keys32", "d_values32", "m", "d_old_paths", "d_new_paths", "d_old_values32", "d_roots32",
                                             "stream"],
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lurk_hip.h")).read(), flags=re.S)


def test_the_entry_points_are_declared_exported_and_bound_under_abi_4():
    from lurk_beta_amd import _lib

    raw = open(os.path.join(ROOT, "include", "lurk_hip.h")).read()
    assert re.search(r"^#define LURK_HIP_ABI_VERSION 4$", raw, flags=re.M)  # an addition
    hdr = _header()
    assert re.search(r"typedef\s+struct\s+lurk_hip_trie_nodes\s+lurk_hip_trie_nodes\s*;", hdr)
    assert sorted(set(re.findall(r"\b(lurk_hip_trie_nodes_[a-z0-9_]+)\s*\(", hdr))) == sorted(PARAMS)
    lib = _lib.load()
    assert lib.lurk_hip_abi_version() == 4
    for name, want in PARAMS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl, name
        params = [a.strip().split()[-1].lstrip("*") for a in decl.group(1).split(",")]
        assert params == want, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(want), name
        assert hasattr(lib, name), name
    # the new section follows the trie's
    assert hdr.index("lurk_hip_trie_verify_insert_dev") < hdr.index("lurk_hip_trie_nodes_create") < hdr.index("lurk_hip_trie_circuit_size")


def test_the_rust_crate_declares_and_calls_them_with_the_headers_arity():
    src = os.path.join(ROOT, "rust", "lurk-hip-sys", "src")
    ffi = open(os.path.join(src, "ffi.rs")).read()
    assert "pub struct lurk_hip_trie_nodes {" in ffi
    fns = dict(re.findall(r"pub fn (\w+)\((.*?)\)(?: -> [^;]+)?;", ffi[ffi.index('extern "C" {'):]))
    for name, want in PARAMS.items():
        assert name in fns, name
        assert [p.split(":")[0].strip() for p in fns[name].split(", ")] == want, name
    wrapper = open(os.path.join(src, "trie.rs")).read()
    assert "pub struct TrieNodes" in wrapper and "impl Drop for TrieNodes" in wrapper
    for name, want in PARAMS.items():
        calls = list(re.finditer(r"\b" + name + r"\s*\(", wrapper))
        assert calls, f"rust/lurk-hip-sys/src/trie.rs never calls {name}"
        for m in calls:
            i, depth, args, cur = m.end(), 1, 0, ""
            while depth and i < len(wrapper):
                ch = wrapper[i]
                depth += ch in "([{"
                depth -= ch in ")]}"
                if ch == "," and depth == 1:
                    args += bool(cur.strip())
                    cur = ""
                elif depth:
                    cur += ch
                i += 1
            args += bool(cur.strip())
            assert args == len(want), (name, args)


def test_the_mirror_imports_and_is_exported_without_a_gpu():
    import lurk_beta_amd
    from lurk_beta_amd.trie import DeviceTrieNodes

    assert lurk_beta_amd.DeviceTrieNodes is DeviceTrieNodes and "DeviceTrieNodes" in lurk_beta_amd.__all__
    for method in ("create", "register", "add_trie", "get", "prove_lookup", "prove_insert", "insert_chain", "close"):
        assert callable(getattr(DeviceTrieNodes, method)), method


def test_every_device_call_fails_loudly_without_a_device():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from lurk_beta_amd import _lib

    lib = _lib.load()
    h = ctypes.c_void_p()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fake = ctypes.c_void_p(ctypes.addressof(buf))  # never dereferenced: the device check comes first
    miss = ctypes.c_uint64()
    calls = {
        "lurk_hip_trie_nodes_create": (ctypes.byref(h), 2, 3, 0),
        "lurk_hip_trie_nodes_register_dev": (fake, p, 1, p, None),
        "lurk_hip_trie_nodes_add_trie": (fake, fake, None),
        "lurk_hip_trie_nodes_get_dev": (fake, p, 1, p, p, None),
        "lurk_hip_trie_nodes_prove_lookup_dev": (fake, p, 0, p, 1, p, p, p, ctypes.byref(miss), None),
        "lurk_hip_trie_nodes_prove_insert_dev": (fake, p, 0, p, p, 1, p, p, p, p, p, ctypes.byref(miss), 1, None),
        "lurk_hip_trie_nodes_insert_chain_dev": (fake, p, p, p, 1, p, p, p, p, None),
    }
    for name, args in calls.items():
        rc = getattr(lib, name)(*args)
        assert rc == 1, (name, rc)  # LURK_HIP_ERR_NO_DEVICE
        assert "no CPU fallback" in lib.lurk_hip_last_error().decode(), name
    assert not h.value
    # the two host-only calls: a null store is an argument error, destroying nothing is fine
    assert lib.lurk_hip_trie_nodes_info(None, None, None, None, None, None) == 2
    assert lib.lurk_hip_trie_nodes_destroy(None) == 0
