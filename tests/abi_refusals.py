"""The bad calls whose refusals are pinned to recorded answers (tests/golden/abi_refusals_*.json; checked by tests/test_abi_refusals.py).

A case is (entry point, arguments).  An argument is an int (passed as it is), None (NULL), or a word: "z<n>" = n zero bytes, "f<n>" = n bytes
of 0xff (a canonical scalar that is not reduced), "one32" = the scalar 1, "i" / "s" = an int / size_t the call may write (recorded with the
row), "h" = a handle slot the call may fill (released afterwards; only its NULL-ness is recorded), "T" = a fresh Keccak transcript.
Every case refuses its arguments before any buffer is read past the sizes given here and before any kernel is launched.

The answers are recorded from the build the behaviour is pinned to and never from the code under test:
    LURK_HIP_LIB=<that build's liblurk_hip.so> python -m tests.abi_refusals host|device"""
import ctypes
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z96 = "z96"

# host-only entry points: no device is needed
HOST_CASES = [
    ("lurk_hip_point_sum", [7, Z96, Z96, 1]),
    ("lurk_hip_point_sum", [4, Z96, Z96, 1]),
    ("lurk_hip_point_sum", [-1, Z96, Z96, 1]),
    ("lurk_hip_point_sum", [7, None, None, 1]),  # two bad arguments: the curve is named
    ("lurk_hip_point_sum", [0, None, Z96, 1]),
    ("lurk_hip_point_sum_gathered", [7, Z96, Z96, 0]),
    ("lurk_hip_point_mul", [7, Z96, Z96, "one32", 0]),
    ("lurk_hip_point_mul", [4, Z96, Z96, "one32", 1]),
    ("lurk_hip_point_mul", [2, Z96, None, "one32", 0]),
    ("lurk_hip_point_to_affine_canonical", [7, "z64", Z96]),
    ("lurk_hip_point_to_affine_canonical", [-1, "z64", Z96]),
    ("lurk_hip_point_to_affine_canonical", [3, None, Z96]),
    ("lurk_hip_shake256", [None, 4, "z32", 32]),
    ("lurk_hip_shake256", [b"abc", 3, None, 32]),
    ("lurk_hip_ck_params_get", [None]),
    ("lurk_hip_ck_params_set", ["z112"]),  # struct_size 0
    ("lurk_hip_ck_from_label_host", [7, b"ck", 2, 1, "z64"]),
    ("lurk_hip_ck_from_label_host", [2, b"ck", 2, 1, "z64"]),
    ("lurk_hip_ck_from_label_host", [3, b"ck", 2, 1, "z64"]),
    ("lurk_hip_ck_from_label_host", [0, None, 2, 1, "z64"]),
    ("lurk_hip_ck_from_label_host", [1, b"ck", 2, (1 << 16) + 1, "z64"]),
    ("lurk_hip_poseidon_constants", [3, 4, "i", "i", None, None]),
    ("lurk_hip_poseidon_constants", [7, 4, "i", "i", None, None]),
    ("lurk_hip_poseidon_constants", [-1, 4, "i", "i", None, None]),
    ("lurk_hip_poseidon_constants", [7, 5, "i", "i", None, None]),
    ("lurk_hip_poseidon_constants", [2, 5, "i", "i", None, None]),
    ("lurk_hip_slot_witness_size", [3, 4, "s"]),
    ("lurk_hip_slot_witness_size", [7, 4, "s"]),
    ("lurk_hip_slot_witness_size", [7, 0, "s"]),
    ("lurk_hip_slot_witness_size", [7, 5, "s"]),
    ("lurk_hip_slot_witness_size", [0, 4, None]),
    ("lurk_hip_poseidon_hash_host", [3, 4, "z128", 1, "z32"]),
    ("lurk_hip_poseidon_hash_host", [7, 4, "z128", 1, "z32"]),
    ("lurk_hip_poseidon_hash_host", [7, 5, None, 1, None]),
    ("lurk_hip_poseidon_hash_host", [1, 4, None, 1, "z32"]),
    ("lurk_hip_sumcheck_verify", [3, 2, 0, "z32", None, None, "z32", "i"]),
    ("lurk_hip_sumcheck_verify", [7, 2, 0, "z32", None, None, "z32", "i"]),
    ("lurk_hip_sumcheck_verify", [7, 4, 0, None, None, None, None, None]),
    ("lurk_hip_sumcheck_verify", [0, 4, 0, "z32", None, None, "z32", "i"]),
    ("lurk_hip_sumcheck_verify", [0, 2, 0, "f32", None, None, "z32", "i"]),  # a claim that is not reduced: rc 0, ok 0
    ("lurk_hip_sumcheck_verify", [1, 3, 0, "f32", None, None, "z32", "i"]),
    ("lurk_hip_sumcheck_verify", [2, 2, 1, "z32", "z96", "f32", "z32", "i"]),  # a challenge that is not reduced
    ("lurk_hip_sumcheck_verify", [2, 2, 1, "z32", "f96", "z32", "z32", "i"]),  # coefficients that are not reduced
    ("lurk_hip_hyperkzg_pairing_inputs", [7, 1, Z96, "z32", "z32", None, Z96, "z288", "one32", "z32", "z32", Z96, Z96, "i", "i"]),
    ("lurk_hip_hyperkzg_pairing_inputs", [0, 1, Z96, "z32", "z32", None, Z96, "z288", "one32", "z32", "z32", Z96, Z96, "i", "i"]),
    ("lurk_hip_hyperkzg_pairing_inputs", [3, 1, Z96, "z32", "z32", None, Z96, "z288", "one32", "z32", "z32", Z96, Z96, "i", "i"]),
    ("lurk_hip_hyperkzg_pairing_inputs", [2, 0, Z96, "z32", "z32", None, Z96, "z288", "one32", "z32", "z32", Z96, Z96, "i", "i"]),
    ("lurk_hip_hyperkzg_pairing_inputs", [2, 1, None, "z32", "z32", None, Z96, "z288", "one32", "z32", "z32", Z96, Z96, "i", "i"]),
    ("lurk_hip_hyperkzg_pairing_inputs", [2, 1, Z96, "z32", "z32", None, Z96, "z288", "f32", "z32", "z32", Z96, Z96, "i", "i"]),  # r not reduced
    ("lurk_hip_hyperkzg_pairing_inputs", [2, 1, Z96, "f32", "z32", None, Z96, "z288", "one32", "z32", "z32", Z96, Z96, "i", "i"]),  # x not reduced
    ("lurk_hip_hyperkzg_pairing_inputs", [2, 1, Z96, "z32", "z32", None, "f96", "z288", "one32", "z32", "z32", Z96, Z96, "i", "i"]),  # v not reduced
    ("lurk_hip_hyperkzg_pairing_inputs", [2, 1, Z96, "z32", "z32", None, Z96, "z288", "z32", "z32", "z32", Z96, Z96, "i", "i"]),  # r = 0
    ("lurk_hip_slot_constraints_size", [3, 4, "s", "s", "s", "s"]),
    ("lurk_hip_slot_constraints_size", [7, 4, "s", "s", "s", "s"]),
    ("lurk_hip_slot_constraints_size", [-1, 4, "s", "s", "s", "s"]),
    ("lurk_hip_slot_constraints_size", [7, 5, "s", "s", "s", "s"]),
    ("lurk_hip_slot_constraints_size", [0, 5, "s", "s", "s", "s"]),
    ("lurk_hip_slot_constraints_size", [7, 4, None, "s", "s", "s"]),
    ("lurk_hip_slot_constraints", [7, 4] + ["z8"] * 9),
    ("lurk_hip_slot_constraints", [3, 4] + ["z8"] * 9),
    ("lurk_hip_slot_constraints", [7, 4] + [None] * 9),
    ("lurk_hip_nova_ro_squeeze", [3, "z32", 1, 128, "z32"]),
    ("lurk_hip_nova_ro_squeeze", [7, "z32", 1, 128, "z32"]),
    ("lurk_hip_nova_ro_squeeze", [7, "z32", 1, 0, "z32"]),
    ("lurk_hip_nova_ro_squeeze", [0, "z32", 1, 251, "z32"]),
    ("lurk_hip_nova_ro_squeeze", [7, None, 1, 128, "z32"]),
    ("lurk_hip_nova_ro_pattern_tag", [1, 1, 0, None]),
    ("lurk_hip_ro_params_get", [None]),
    ("lurk_hip_ro_params_set", ["z96"]),  # struct_size 0
    ("lurk_hip_nifs_absorb_list", [7, "z32", Z96, Z96, "z32", None, Z96, None, 0, Z96, None, 0, "s"]),
    ("lurk_hip_nifs_absorb_list", [2, "z32", Z96, Z96, "z32", None, Z96, None, 0, Z96, None, 0, "s"]),
    ("lurk_hip_nifs_absorb_list", [3, "z32", Z96, Z96, "z32", None, Z96, None, 0, Z96, None, 0, "s"]),
    ("lurk_hip_nifs_absorb_list", [7, None, Z96, Z96, "z32", None, Z96, None, 0, Z96, None, 0, "s"]),
    ("lurk_hip_nifs_absorb_list", [0, "f32", Z96, Z96, "z32", None, Z96, None, 0, Z96, None, 0, "s"]),  # a digest that is not a canonical scalar
    ("lurk_hip_nifs_challenge", [7, "z32", Z96, Z96, "z32", None, Z96, None, 0, Z96, "z32"]),
    ("lurk_hip_nifs_challenge", [2, "z32", Z96, Z96, "z32", None, Z96, None, 0, Z96, "z32"]),
    ("lurk_hip_nifs_challenge", [1, "z32", Z96, Z96, "z32", None, Z96, None, 0, Z96, None]),
    ("lurk_hip_nifs_challenge", [1, "f32", Z96, Z96, "z32", None, Z96, None, 0, Z96, "z32"]),
    ("lurk_hip_keccak256", [None, 1, "z32"]),
    ("lurk_hip_keccak_transcript_new", [None, b"x", 1]),
    ("lurk_hip_keccak_transcript_absorb", [None, b"x", 1, b"y", 1]),
    ("lurk_hip_keccak_transcript_absorb_scalars", ["T", b"x", 1, None, 1]),
    ("lurk_hip_keccak_transcript_absorb_point", ["T", b"x", 1, 7, Z96]),
    ("lurk_hip_keccak_transcript_absorb_point", ["T", b"x", 1, 4, Z96]),
    ("lurk_hip_keccak_transcript_absorb_point", ["T", b"x", 1, 7, None]),
    ("lurk_hip_keccak_transcript_dom_sep", [None, b"x", 1]),
    ("lurk_hip_keccak_transcript_squeeze", ["T", b"x", 1, 3, "z32"]),
    ("lurk_hip_keccak_transcript_squeeze", ["T", b"x", 1, 7, "z32"]),
    ("lurk_hip_keccak_transcript_squeeze", ["T", b"x", 1, -1, "z32"]),
    ("lurk_hip_keccak_transcript_squeeze", ["T", b"x", 1, 7, None]),
]

# device entry points whose dispatch goes through with_field / with_curve: refused behind require_device(), before any launch
DEVICE_CASES = [
    ("lurk_hip_sumcheck_round_dev", [7, 2, None, 0, None, None, None]),
    ("lurk_hip_sumcheck_prove_dev", [3, 2, None, 0, None, None, None, None, None, None, None]),
    ("lurk_hip_sumcheck_prove_batch_dev", [7, 2, 1, None, 0, None, None, None, None, None, None, None, None]),
    ("lurk_hip_eq_evals_dev", [7, None, 0, None, None]),
    ("lurk_hip_eq_evals_dev", [3, None, 0, None, None]),
    ("lurk_hip_inner_product_dev", [7, None, None, 0, None, None]),
    ("lurk_hip_fold_halves_dev", [3, None, 0, None, None, None]),
    ("lurk_hip_ipa_round_scalars_dev", [7, None, 0, None, 0, None, None, None]),
    ("lurk_hip_ipa_coef_fold_dev", [7, None, 0, 0, None, None, None]),
    ("lurk_hip_ipa_s_vector_dev", [7, None, 0, None, None]),
    ("lurk_hip_ipa_s_vector_dev", [2, "f32", 1, "z8", None]),  # a challenge that is not reduced (refused on the host)
    ("lurk_hip_points_fold_halves_dev", [7, None, 0, None, None, None, None]),
    ("lurk_hip_points_fold_halves_dev", [2, None, 0, None, None, None, None]),
    ("lurk_hip_fold_vec_dev", [7, None, None, None, 0, None, None]),
    ("lurk_hip_fold_vecs_dev", [3, 0, None, None, None, None, None, None]),
    ("lurk_hip_fold_vec", [7, None, None, None, 0, None]),
    ("lurk_hip_r1cs_create", ["h", 7, 0, 0, 0] + [None] * 9),
    ("lurk_hip_r1cs_create", ["h", 3, 0, 0, 0] + [None] * 9),
    ("lurk_hip_poseidon_batch_dev", [7, 4, None, 0, None, None]),
    ("lurk_hip_poseidon_batch_dev", [3, 8, None, 0, None, None]),
    ("lurk_hip_poseidon_batch", [7, 4, None, 0, None]),
    ("lurk_hip_slot_witness_dev", [7, 4, None, 0, 0, None, None, 0, 0, None]),
    ("lurk_hip_slot_witness_dev", [7, 0, None, 0, 0, None, None, 0, 0, None]),
    ("lurk_hip_slot_witness", [3, 4, None, 0, 0, None]),
    ("lurk_hip_mle_fold_pairs_dev", [7, None, 0, None, None, None]),
    ("lurk_hip_poly_eval_dev", [3, None, 0, None, 0, None, None]),
    ("lurk_hip_poly_div_linear_dev", [7, None, 0, None, 0, None, None, None]),
    ("lurk_hip_synth_scalars_dev", [7, 0, 0, 0, 0, None, 0, None]),
    ("lurk_hip_synth_scalars_dev", [4, 0, 0, 0, 0, None, 0, None]),
    ("lurk_hip_synth_scalars_dev", [3, 0, 0, 0, 1, None, 0, None]),  # the fourth field is served here: the NULL buffer is what is refused
    ("lurk_hip_synth_bases_dev", [7, 0, 0, None, None]),
    ("lurk_hip_synth_bases_dev", [3, 0, 1, None, None]),
    ("lurk_hip_synth_kzg_bases_dev", [7, "z32", 0, 0, None, None]),
    ("lurk_hip_synth_kzg_bases_dev", [0, "z32", 0, 0, None, None]),
    ("lurk_hip_synth_kzg_bases_dev", [2, "f32", 0, 0, None, None]),  # tau not reduced
    ("lurk_hip_ntt_dev", [2, None, 0, 0, None]),
    ("lurk_hip_ntt_dev", [7, None, 0, 0, None]),
    ("lurk_hip_ntt", [2, None, 0, 0]),
    ("lurk_hip_msm_ctx_create", ["h", 7, None, 0, 0]),
    ("lurk_hip_msm_ctx_create", ["h", 4, None, 0, 0]),
    ("lurk_hip_msm_ctx_create_dev", ["h", 7, None, 0, 0, None]),
    ("lurk_hip_msm_ctx_create_dev", ["h", -1, None, 0, 0, None]),
    ("lurk_hip_msm_ctx_from_label", ["h", 7, b"ck", 2, 0, 0]),
    ("lurk_hip_msm_ctx_from_label", ["h", 2, b"ck", 2, 0, 0]),
    ("lurk_hip_msm_multi_create", ["h", 7, None, 0, None, 0, 0]),
    ("lurk_hip_ck_hash_to_curve_dev", [7, b"d", None, 0, None, None]),
    ("lurk_hip_ck_hash_to_curve_dev", [3, b"d", None, 0, None, None]),
    ("lurk_hip_ck_from_label_dev", [7, b"ck", 2, 0, None, None]),
    ("lurk_hip_ck_from_label_dev", [2, b"ck", 2, 0, None, None]),
    ("lurk_hip_fold_ctx_create", ["h", 7, None, None]),
]


def _jsonable(args):
    return [a.decode() if isinstance(a, bytes) else a for a in args]


def replay(lib, name, args):
    """Make one call; the row it answers with: {name, args, rc, message, outs}."""
    keep, outs, handles, transcripts, cargs = [], [], [], [], []
    argtypes = getattr(lib, name).argtypes
    for a, ty in zip(args, argtypes):
        if a is None or isinstance(a, int):
            cargs.append(a)
        elif isinstance(a, bytes):
            cargs.append(a if ty is ctypes.c_char_p else ctypes.cast(ctypes.c_char_p(a), ctypes.c_void_p))
            keep.append(a)
        elif a in ("i", "s", "h"):
            v = {"i": ctypes.c_int, "s": ctypes.c_size_t, "h": ctypes.c_void_p}[a](-1 if a == "i" else 0)
            (handles if a == "h" else outs).append(v)
            cargs.append(ctypes.byref(v) if not isinstance(ty, type) or ty is not ctypes.c_void_p else ctypes.cast(ctypes.pointer(v), ctypes.c_void_p))
        elif a == "T":
            t = ctypes.c_void_p()
            assert lib.lurk_hip_keccak_transcript_new(ctypes.byref(t), b"refusals", 8) == 0
            transcripts.append(t)
            cargs.append(t)
        else:
            n = 32 if a == "one32" else int(a[1:])
            buf = ctypes.create_string_buffer(b"\x01" + bytes(31) if a == "one32" else (b"\xff" if a[0] == "f" else b"\x00") * n, n)
            keep.append(buf)
            cargs.append(ctypes.cast(buf, ty) if ty is not ctypes.c_void_p else ctypes.cast(buf, ctypes.c_void_p))
    rc = getattr(lib, name)(*cargs)
    row = {"name": name, "args": _jsonable(args), "rc": rc, "message": lib.lurk_hip_last_error().decode(),
           "outs": [v.value for v in outs] + [h.value is not None for h in handles]}
    for t in transcripts:
        lib.lurk_hip_keccak_transcript_destroy(t)
    assert all(h.value is None for h in handles), f"{name} accepted {args}: this table holds refusals only"
    return row


def golden_path(which):
    return os.path.join(GOLDEN, f"abi_refusals_{which}.json")


def load_golden(which):
    with open(golden_path(which)) as f:
        return {(r["name"], json.dumps(r["args"])): r for r in json.load(f)}


if __name__ == "__main__":
    from lurk_beta_amd import _lib

    which = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else golden_path(which)
    rows = [replay(_lib.load(), name, args) for name, args in {"host": HOST_CASES, "device": DEVICE_CASES}[which]]
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows from {_lib.LIB_PATH} -> {out}")
