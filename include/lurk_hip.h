/*
 * lurk_hip.h - C ABI of liblurk_hip.so: the MI355X (gfx950) proving hot path for Lurk.
 *
 * This is the drop-in boundary.  lurk-beta has no backend plugin registry; the seam is one level
 * below its Rust generics, where arecibo calls the `pasta-msm` C symbols and where lurk-beta's
 * PoseidonCache calls neptune.  Every entry point below names the
 * reference interface it replaces.  Conventions kept from that seam:
 *   - plain pointers and sizes only; the caller owns every buffer, borrowed for the call;
 *   - field elements are 32 bytes, 4 x u64 little-endian limbs;
 *   - curve points use the pasta_curves `repr-c` layouts (/root/reference/Cargo.toml:42):
 *       affine  {x, y}      64 B, Montgomery form, identity = (0, 0)
 *       jacobian{x, y, z}   96 B, Montgomery form, identity has z = 0
 *   - scalars handed to the MSM are Montgomery form when is_mont != 0 (how pasta_curves stores
 *     them in memory), canonical integers otherwise;
 *   - Poseidon / NTT take and return canonical bytes (`PrimeField::to_repr()`,
 *     /root/reference/src/field.rs:72-75);
 *   - every function returns 0 on success, non-zero on failure; lurk_hip_last_error() then holds
 *     the message for the calling thread (pasta-msm returns {code, message}; the Rust side panics
 *     on non-zero).  There is NO CPU fallback: without a usable gfx950 device every compute entry
 *     point fails with LURK_HIP_ERR_NO_DEVICE.
 *   - entry points are thread-safe (arecibo commits from rayon worker threads).
 *   - *_dev variants take device pointers and a hipStream_t (as void*; NULL = default stream) and
 *     do not synchronise: inputs stay resident in HBM across calls.  Device buffers of field elements / points must be
 *     16-byte aligned (anything hipMalloc returns, at any multiple of 32 bytes); host buffers need no alignment.
 */
#ifndef LURK_HIP_H
#define LURK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* field ids (LurkField instances, /root/reference/src/field.rs:265-279) */
#define LURK_FIELD_PALLAS_FP 0 /* pasta_curves::Fp  = pallas::Base  = vesta::Scalar */
#define LURK_FIELD_PALLAS_FQ 1 /* pasta_curves::Fq  = pallas::Scalar = vesta::Base  */
#define LURK_FIELD_BN254_FR 2  /* halo2curves::bn256::Fr (the field of every KAT in the reference) */
#define LURK_FIELD_BN254_FQ 3  /* halo2curves::bn256::Fq = grumpkin::Fr: the BN254 base field.  Offered where a commitment needs it
                                * (the MSM contexts, the point helpers, lurk_hip_synth_scalars_dev) and as the field of a shape made by
                                * lurk_hip_r1cs_create_for_curve(LURK_CURVE_GRUMPKIN) - what a folding context on Grumpkin runs over;
                                * every other entry point that takes a field id as an argument refuses it */

/* curve ids (CurveCycleEquipped engines, /root/reference/src/proof/nova.rs:40-71) */
#define LURK_CURVE_PALLAS 0
#define LURK_CURVE_VESTA 1
/* the BN254 / Grumpkin cycle (lurk-beta's default: Bn256EngineKZG + GrumpkinEngine).  Both have a = 0: BN254 G1 is y^2 = x^3 + 3 over
 * Fq with scalars in Fr, Grumpkin is y^2 = x^3 - 17 over Fr with scalars in Fq.  Layouts as halo2curves `repr-c` has them, recalled
 * [MEM] and unpinned like the Pasta ones: affine {x, y} 64 B Montgomery with (0, 0) for the identity, Jacobian {x, y, z} 96 B.
 * Offered: every lurk_hip_msm_* / lurk_hip_msm_ctx_* / lurk_hip_msm_multi_* commitment path, the point helpers,
 * lurk_hip_synth_bases_dev (generators (1, 2) and (1, sqrt(-16))) and lurk_hip_fold_ctx_* on both curves with a caller-supplied
 * challenge (Grumpkin over a shape from lurk_hip_r1cs_create_for_curve: its scalar field is LURK_FIELD_BN254_FQ);
 * on BN254 G1 alone the HyperKZG opening argument (lurk_hip_hyperkzg_prove_dev, lurk_hip_hyperkzg_pairing_inputs) and the powers-of-tau
 * test key (lurk_hip_synth_kzg_bases_dev), which refuse Grumpkin and the Pasta curves by name, and the compressing SNARK whose opening
 * is that argument (lurk_hip_spartan_kzg_prove*_dev, lurk_hip_spartan_kzg_verify*_dev; the Pasta / IPA calls keep refusing BN254).
 * Refused by name (non-zero, the curve named in lurk_hip_last_error()): lurk_hip_msm_ctx_from_label and the other hash-to-curve calls,
 * lurk_hip_msm_ctx_fold_key_dev, the IPA / Spartan / verify calls, lurk_hip_fold_step, _set_pp_digest, _challenge and
 * lurk_hip_nifs_* (no Poseidon constants over either base field of this cycle yet). */
#define LURK_CURVE_BN254 2
#define LURK_CURVE_GRUMPKIN 3

#define LURK_HIP_OK 0
#define LURK_HIP_ERR_NO_DEVICE 1
#define LURK_HIP_ERR_INVALID_ARG 2
#define LURK_HIP_ERR_HIP 3
#define LURK_HIP_ERR_OOM 4

/* ---- runtime ---------------------------------------------------------------------------- */
int lurk_hip_device_count(void);
const char* lurk_hip_last_error(void);
const char* lurk_hip_version(void);
/* The ABI revision this header describes; lurk_hip_abi_version() is what the loaded library was built from (a binding compares the
 * two at start-up).  A revision that only adds entry points raises the number too: a binding built against revision n runs on any library
 * that reports >= n until a revision says otherwise.  4: the verifiers - lurk_hip_r1cs_sparse_mle_dev, lurk_hip_ipa_s_vector_dev,
 * lurk_hip_sumcheck_verify, lurk_hip_ipa_verify_dev, lurk_hip_spartan_verify_dev, lurk_hip_spartan_verify_batch_dev (additions only);
 * later additions under the same number (a binding probes for them by symbol): lurk_hip_r1cs_transpose_dev, lurk_hip_r1cs_read,
 * lurk_hip_grid_cus, the four lurk_hip_trie_circuit_* calls, the nine lurk_hip_trie_nodes_* calls, lurk_hip_r1cs_create_for_curve.
 * 3: lurk_hip_slot_constraints_size / lurk_hip_slot_constraints,
 * lurk_hip_frames_r1cs_create, lurk_hip_r1cs_is_sat_dev (additions only).  2 (round 6): lurk_hip_msm_ctx_info's *precomputed is a boolean (the key's form comes from lurk_hip_msm_ctx_form),
 * LURK_MSM_SLOTS is 6, LURK_MSM_SUBMIT_FOLLOW, the parameter blocks lurk_hip_ro_params / lurk_hip_ck_params, lurk_hip_scratch_trim.
 * 1: rounds 1-4 (*precomputed returned the form 0 / 1 / 2, four slots). */
#define LURK_HIP_ABI_VERSION 4
int lurk_hip_abi_version(void);
/* Prover scratch (the compressing SNARK's sum-check tables, eq tables, opening-argument halves) comes from one stack arena per
 * (device, stream) that grows by blocks of >= 256 MiB and is KEPT between proofs: about 2 GB per stream that has run a 2^20-row proof,
 * for the life of the process.  trim releases every arena no prover is using right now (nothing is live in it) back to the driver;
 * *released_bytes (may be NULL) = what went back.  The next proof on that stream re-allocates (a device-wide synchronisation the first
 * time a size is seen): call it when a process stops proving, not between proofs.
 * Threads: a prover call (lurk_hip_spartan_prove*_dev, lurk_hip_ipa_prove_dev, lurk_hip_sumcheck_prove*_dev) holds its stream's arena
 * for as long as the call runs - two calls on ONE stream from two threads run one after the other, calls on different streams run
 * side by side.  No entry point of the library takes the arenas of two streams at once, so the arenas cannot deadlock among
 * themselves; a caller that wraps prover calls in locks of its own must take them in one order. */
int lurk_hip_scratch_trim(size_t* released_bytes);
/* bind the calling thread to a device (one process per GPU; the multi-GPU layer calls this) */
int lurk_hip_set_device(int device);
/* The CU count the capped grids of the vector kernels (sum-check, inner-product argument, HyperKZG, Poseidon batches) are computed from:
 * the current device's, or LURK_GRID_CUS from the environment (a test switch, read once per process: a small value sends short inputs
 * through the second pass of every grid-stride loop; results do not depend on it).  Host-side: no device is touched (256 is reported
 * until a device call has read the device's count). */
int lurk_hip_grid_cus(int* out);
/* per-kernel timing with HIP events on the launch stream (bench.py's roofline leg) */
int lurk_hip_profile_enable(int on);
int lurk_hip_profile_reset(void);
/* total milliseconds and launch count recorded for kernels whose name starts with `prefix` */
int lurk_hip_profile_get(const char* prefix, double* total_ms, uint64_t* launches);

/* ---- Pedersen MSM ------------------------------------------------------------------------
 * Replaces pasta-msm's
 *   void mult_pippenger_pallas(pallas_point* out, const pallas_affine* points, size_t npoints,
 *                              const pallas_scalar* scalars, bool is_mont);        (and _vesta)
 * reached from arecibo CommitmentEngine::commit -> DlogGroup::vartime_multiscalar_mul, whose
 * lurk-beta callers are RecursiveSNARK::new / prove_step (/root/reference/src/proof/nova.rs:287-293,
 * /root/reference/src/proof/supernova.rs:231-244) and PublicParams::setup (nova.rs:205). */
int lurk_hip_msm_pallas(void* out_jacobian96, const void* bases_affine64, size_t npoints,
                        const void* scalars32, int is_mont);
int lurk_hip_msm_vesta(void* out_jacobian96, const void* bases_affine64, size_t npoints,
                       const void* scalars32, int is_mont);
int lurk_hip_msm_bn254(void* out_jacobian96, const void* bases_affine64, size_t npoints,
                       const void* scalars32, int is_mont);
int lurk_hip_msm_grumpkin(void* out_jacobian96, const void* bases_affine64, size_t npoints,
                          const void* scalars32, int is_mont);
/* The two symbols above under the names and the signature pasta-msm's src/lib.rs binds (pasta-msm 0.1.x, arecibo's
 * dependency; un-vendored: /root/reference/Cargo.toml:128 pulls it in through nova): a pasta-msm whose build script links
 * liblurk_hip.so instead of compiling its own C objects needs no source change.  They return nothing, as the originals; a
 * failure (no device, allocation) prints lurk_hip_last_error() and aborts the process. */
/* Opt-in key cache of the four one-shot symbols (default off; LURK_MSM_ONESHOT_KEY_CACHE=1 in the environment, read once when the library is loaded, turns it on for
 * callers that link mult_pippenger_* / cuda_pippenger_* without a source change and so cannot call this function):
 * arecibo commits under ONE immutable key at ONE address for a whole proof, yet the pasta-msm signature makes it hand the
 * bases over on every call (64 of the 96 bytes per point that cross PCIe).  With the cache on, the bases of the previous call
 * stay in HBM; a call with the same `points` pointer, npoints <= the cached length and bit-identical points at 4 096 sampled
 * positions reuses them (2^22: 14.0 ms -> 8.9 ms per call, of which 2.7 ms are the scalars' own upload).  A buffer rewritten in place at unsampled positions only would be missed:
 * do not enable it for callers that edit a key in place. */
int lurk_hip_msm_oneshot_key_cache(int enable);
#include <stdbool.h>
void mult_pippenger_pallas(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);
void mult_pippenger_vesta(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);
/* pasta-msm's GPU symbols (its `cuda` feature over sppark; what arecibo's GPU build binds instead of the two above, SURVEY.md
 * section 8b [MEM]): same arguments, sppark's RustError returned BY VALUE - code 0 and a NULL message on success; otherwise the
 * library's error code and a malloc'd message that the caller frees (sppark's Rust side does, in Drop).  No abort, no fallback. */
typedef struct lurk_hip_rust_error {
    int code;
    char* message;
} lurk_hip_rust_error;
lurk_hip_rust_error cuda_pippenger_pallas(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);
lurk_hip_rust_error cuda_pippenger_vesta(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);
/* grumpkin-msm's symbols (arecibo's MSM crate for the BN254 / Grumpkin cycle; names and signatures recalled [MEM], unpinned): the same
 * behaviour as the four pasta-msm names above - mult_pippenger_* return nothing and abort with the library's message on failure,
 * cuda_pippenger_* return the RustError by value. */
void mult_pippenger_bn254(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);
void mult_pippenger_grumpkin(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);
lurk_hip_rust_error cuda_pippenger_bn254(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);
lurk_hip_rust_error cuda_pippenger_grumpkin(void* out_jacobian96, const void* points_affine64, size_t npoints, const void* scalars32, bool is_mont);

/* Resident-bases context: the commitment key `ck` is constant for the whole proof
 * (/root/reference/src/proof/nova.rs:196-216), so it is uploaded once and kept in HBM.
 * Mirrors the msm-context API of the argumentcomputer pasta-msm fork (init(points) -> ctx,
 * with(ctx, scalars) -> point).  flags: bit0 = build the per-window precomputed table
 * (2^(c*k) * P_i for every window k; costs windows x 64 B x npoints of HBM; every window then shares
 * one bucket set, so the window grows to c = 20 bits from 2^19 points on: 13 n mixed additions instead of
 * 16 n); bits 8..15 = window-bit override for the table mode (16..20, 0 = automatic).
 * Footprint of bit0 for keys of <= 2^16 points with no window override: the SMALL form - every multiple m * 2^(c k) * P_i
 * resident, 256 KiB per point (2.6 GB at 10^4 points, 4.3 GB at 2^14, 5.6 GB at 2^16) plus <= 1 GiB of scratch while it is
 * built - so that a commitment is one launch (0.13 ms at 2^13 points instead of 0.35).  It is chosen only when it fits a quarter
 * of the device memory free at creation time; otherwise, and always with LURK_MSM_FLAG_WINDOW_BITS(16), the key takes the window
 * table (64 B x 16 per point).  lurk_hip_msm_ctx_form reports the form that was taken; a caller that needs the choice to be
 * the same on every run and device states it: LURK_MSM_FLAG_SMALL_FORM (the small form, or LURK_HIP_ERR_INVALID_ARG / _OOM) or
 * LURK_MSM_FLAG_NO_SMALL_FORM (the window table whatever is free). */
typedef struct lurk_hip_msm_ctx lurk_hip_msm_ctx;
#define LURK_MSM_FLAG_PRECOMPUTE 1
#define LURK_MSM_FLAG_WINDOW_BITS(c) (((c) & 0xff) << 8)
#define LURK_MSM_FLAG_SMALL_FORM (1 << 16)
#define LURK_MSM_FLAG_NO_SMALL_FORM (1 << 17)
/* lurk_hip_msm_multi_create only: cut the key over as many of the listed devices as leave every slice at least 2^20 points (the first k
 * of the list; LURK_MSM_MULTI_MIN_SLICE_LOG in the environment moves the threshold).  A slice pays a whole commitment's latency-bound
 * chain (~0.64 ms) around 0.83 ms of accumulation per 2^20 points: smaller slices cost more than they take off. */
#define LURK_MSM_FLAG_AUTO_SLICES (1 << 18)
int lurk_hip_msm_ctx_create(lurk_hip_msm_ctx** ctx, int curve, const void* bases_affine64,
                            size_t npoints, int flags);
/* same, bases already in device memory (borrowed for the lifetime of the ctx unless precomputed) */
int lurk_hip_msm_ctx_create_dev(lurk_hip_msm_ctx** ctx, int curve, const void* d_bases_affine64,
                                size_t npoints, int flags, void* stream);
/* commit to the first nscalars bases: out = sum_i scalars[i] * bases[i]  (nscalars <= npoints,
 * as CommitmentEngine::commit uses ck[..v.len()]) */
int lurk_hip_msm_ctx_run(lurk_hip_msm_ctx* ctx, void* out_jacobian96, const void* scalars32,
                         size_t nscalars, int is_mont);
/* device scalars in, 96-byte result written to *host* memory out_jacobian96 after the stream
 * has been synchronised by this call (the result is needed by the host-side transcript) */
int lurk_hip_msm_ctx_run_dev(lurk_hip_msm_ctx* ctx, void* out_jacobian96, const void* d_scalars32,
                             size_t nscalars, int is_mont, void* stream);
/* Asynchronous form: up to LURK_MSM_SLOTS commitments in flight per context, each with its own
 * workspace and stream - e.g. commit(W) and commit(T) of one folding step, or the commitments of
 * consecutive steps - so that the latency-bound tail of one overlaps the throughput-bound bucket
 * accumulation of the next.  submit enqueues (ordered after `stream`, the stream that produced the
 * scalars) and returns; wait blocks for that slot and writes the 96-byte result to host memory. */
#define LURK_MSM_SLOTS 6
int lurk_hip_msm_ctx_submit_dev(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars32,
                                size_t nscalars, int is_mont, void* stream);
/* The same with a scheduling class.  Commitments in flight share the integer VALU; a prover knows which one its next step
 * waits for.  FOREGROUND: the accumulation is the plain launch (three waves per SIMD, raised wave priority) - the commitment
 * the host is about to wait for (commit(T) of the open folding step).  BACKGROUND: the persistent one-wave-per-SIMD
 * accumulation at the lowest priority whatever the size - work staged ahead (commit(W2) of the next step), which fills the
 * issue slots the foreground commitment leaves during its sort and its bucket reduction.  DEFAULT = submit_dev (by size).
 * FOLLOW (round 6): work staged ahead that must only take what the open step's serial chain leaves - commit(W2 of the next
 * step).  Sort and plan run at once at the LOWEST wave priority; the accumulation (persistent, two waves per SIMD - LURK_MSM_FOLLOW_WGS -,
 * lowest priority) starts behind the ACCUMULATION of the latest FOREGROUND commitment in flight on this context and fills the window the
 * step leaves idle (commit(T)'s bucket reduction, the host's transcript, the folds, the next cross term); the tail (finalize, bucket
 * reduction) keeps the raised priority: the next step waits for this commitment too. */
#define LURK_MSM_SUBMIT_DEFAULT 0
#define LURK_MSM_SUBMIT_FOREGROUND 1
#define LURK_MSM_SUBMIT_BACKGROUND 2
#define LURK_MSM_SUBMIT_FOLLOW 3
int lurk_hip_msm_ctx_submit_dev_mode(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars32, size_t nscalars, int is_mont,
                                     void* stream, int mode);
int lurk_hip_msm_ctx_wait(lurk_hip_msm_ctx* ctx, int slot, void* out_jacobian96);
/* A PAIR of commitments with disjoint supports in one pass (the L and R of an inner-product-argument round under the resident key:
 * arecibo ipa_pc, /root/reference/src/proof/nova.rs:57-62): ONE scalar vector; the scalars whose index has bit `sel_bit` clear commit
 * to out_lo, the others to out_hi - two key spaces of one sort / accumulate / reduce instead of two commitments that each scan all
 * n scalars for half of them.  Window-table keys only (precompute flag, more than 2^16 points or a window-bit override). */
int lurk_hip_msm_ctx_submit_pair_dev(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars32, size_t nscalars, int is_mont, void* stream,
                                     int sel_bit);
int lurk_hip_msm_ctx_wait_pair(lurk_hip_msm_ctx* ctx, int slot, void* out_lo_jacobian96, void* out_hi_jacobian96);
/* A BATCH of short commitments under prefixes of the resident key in one pass (the folded polynomials of a HyperKZG opening:
 * hyperkzg.hip):
 *     out[k] = sum_{i < lens[k]} d_scalars32[offsets[k] + i] * bases[i],   k < count
 * - every vector commits to the FIRST lens[k] bases, as lurk_hip_msm_ctx_run does.  `offsets` and `lens` are HOST arrays, in elements of
 * 32 B; they are read during the call and not kept.  Vectors may overlap and come in any order; lens[k] == 0 gives the identity.
 * Window-table keys only, as for the pair (all four curves).  A batch takes one of the LURK_MSM_SLOTS slots and is ordered after
 * `stream`, like lurk_hip_msm_ctx_submit_dev; its workspaces are allocated on first use and grow on demand (an allocation failure
 * returns LURK_HIP_ERR_OOM and leaves the slot free).  wait_batch blocks and writes count x 96 B to host memory: for each vector the
 * normalised representative lurk_hip_msm_ctx_wait writes (Z = 1 in Montgomery form, or z = 0 for the identity), so a batch result is
 * byte for byte what lurk_hip_msm_ctx_run_dev gives for that vector.
 * Refused with LURK_HIP_ERR_INVALID_ARG before anything is allocated or launched, the message naming which: a NULL ctx, offsets, lens
 * or output; NULL scalars when some length is non-zero; count == 0 or above LURK_MSM_BATCH_MAX_VECTORS; a length above
 * LURK_MSM_BATCH_MAX_LEN or above the key's points; a total above LURK_MSM_BATCH_MAX_TOTAL; a key that is not in the window-table form;
 * a slot out of range or still pending; wait_batch on a slot that holds an ordinary or pair commitment, and lurk_hip_msm_ctx_wait /
 * _wait_pair on a slot that holds a batch (the pending commitment stays pending). */
#define LURK_MSM_BATCH_MAX_VECTORS 64
#define LURK_MSM_BATCH_MAX_LEN ((size_t)1 << 16)   /* scalars per vector */
#define LURK_MSM_BATCH_MAX_TOTAL ((size_t)1 << 20) /* scalars per batch  */
int lurk_hip_msm_ctx_submit_batch_dev(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars32, const size_t* offsets, const size_t* lens,
                                      size_t count, int is_mont, void* stream);
int lurk_hip_msm_ctx_wait_batch(lurk_hip_msm_ctx* ctx, int slot, void* out_jacobian96);
int lurk_hip_msm_ctx_destroy(lurk_hip_msm_ctx* ctx);
/* Points the context at other device-resident bases (borrowed, plain key) and keeps its workspaces: a key that changes every
 * round (the folded key of the inner-product argument) without re-allocation. */
int lurk_hip_msm_ctx_rebind_dev(lurk_hip_msm_ctx* ctx, const void* d_bases_affine64, size_t npoints);
/* Workspaces (sort buffers, task partials, buckets: ~1 GiB per slot at 2^22 points) are allocated on a slot's first use; a
 * prover that wants no allocation inside its first steps reserves them up front for the largest commitment it will make. */
int lurk_hip_msm_ctx_reserve(lurk_hip_msm_ctx* ctx, size_t nscalars, int slots);
/* *precomputed is a boolean (1 = the key holds precomputed multiples, in either table form).  The FORM of the resident key comes
 * from lurk_hip_msm_ctx_form: 0 = plain (64 B/point), 1 = window table (the only form that commits a pair in one pass:
 * lurk_hip_msm_ctx_submit_pair_dev), 2 = the small-commitment multiples table (keys of <= 2^16 points). */
#define LURK_MSM_FORM_PLAIN 0
#define LURK_MSM_FORM_TABLE 1
#define LURK_MSM_FORM_SMALL 2
int lurk_hip_msm_ctx_info(const lurk_hip_msm_ctx* ctx, int* curve, size_t* npoints, int* window_bits, int* precomputed);
int lurk_hip_msm_ctx_form(const lurk_hip_msm_ctx* ctx, int* form);
int lurk_hip_msm_ctx_device(const lurk_hip_msm_ctx* ctx, int* device); /* the device the key is resident on */
/* Commitment-key generation: arecibo's CommitmentEngine::setup(label, n) = DlogGroup::from_label as
 * PublicParams::setup reaches it (/root/reference/src/proof/nova.rs:196-216): SHAKE256(label) squeezed 32 bytes per point (host:
 * the XOF is sequential), point i = pasta_curves hash_to_curve("from_uniform_bytes") of its bytes - BLAKE2b-512 expand_message_xmd,
 * simplified SWU on the 3-isogenous curve, the degree-3 isogeny - one point per lane on the device, affine Montgomery out.
 * from_label_dev writes npoints x 64 B to device memory (synchronises `stream`); ctx_from_label builds the resident context in
 * place, no host copy of the key ever exists; hash_to_curve_dev is the per-point map on caller-supplied 32-byte strings. */
int lurk_hip_shake256(const void* in, size_t in_len, void* out, size_t out_len); /* host-only helper (the XOF above) */
/* Run-time parameters of the restatement above (round 6): arecibo's from_label and pasta_curves' hash_to_curve are un-vendored
 * (/root/reference/Cargo.toml:128,131) and /root/reference holds no key bytes, so what was recalled from memory is a FIELD, not a
 * literal: the XOF, the bytes squeezed per point, and the three parts of the hash_to_curve domain-separation tag
 * DST = domain_prefix "-" curve_name suite.  Process-wide, set(NULL) restores the defaults (in brackets); from_label_dev /
 * ctx_from_label / from_label_host read them per call.  hash_to_curve_dev takes its own domain prefix and uses the rest.
 * from_label_host is the same map on the host (no device; <= 2^16 points, ~0.3 ms each): the first points of a key for a LURKDUMP
 * probe record (`python -m lurk_beta_amd.dump probe FILE`) or a CPU test. */
#define LURK_CK_XOF_SHAKE256 0
#define LURK_CK_XOF_SHAKE128 1
typedef struct lurk_hip_ck_params {
    uint32_t struct_size;       /* sizeof(lurk_hip_ck_params): get() fills it, set() checks it */
    uint32_t xof;               /* LURK_CK_XOF_* over the label [SHAKE256] */
    uint32_t bytes_per_point;   /* XOF bytes handed to hash_to_curve per point, 1..64 [32] */
    uint32_t reserved;          /* 0 */
    char domain_prefix[32];     /* hash_to_curve's domain prefix, NUL-terminated ["from_uniform_bytes"] */
    char curve_name_pallas[16]; /* CURVE_ID of Pallas in the tag ["pallas"] */
    char curve_name_vesta[16];  /* ["vesta"] */
    char suite[32];             /* the tag's tail ["_XMD:BLAKE2b_SSWU_RO_"] */
} lurk_hip_ck_params;
int lurk_hip_ck_params_get(lurk_hip_ck_params* out);
int lurk_hip_ck_params_set(const lurk_hip_ck_params* params);
int lurk_hip_ck_from_label_host(int curve, const void* label, size_t label_len, size_t npoints, void* out_affine64);
int lurk_hip_ck_hash_to_curve_dev(int curve, const char* domain_prefix, const void* d_uniform32, size_t n, void* d_out_affine64,
                                  void* stream);
int lurk_hip_ck_from_label_dev(int curve, const void* label, size_t label_len, size_t npoints, void* d_out_affine64,
                               void* stream);
int lurk_hip_msm_ctx_from_label(lurk_hip_msm_ctx** ctx, int curve, const void* label, size_t label_len, size_t npoints,
                                int flags);
/* Key files.  The reference caches its public parameters - mostly the commitment key - on disk and
 * maps them back (/root/reference/src/public_parameters/mod.rs:33-56, disk_cache.rs:69-77).  save writes the resident key as it
 * sits in HBM (64-byte header + 64-byte affine Montgomery records; with_table != 0 also the per-window multiples of a
 * precomputed context); load maps the file and copies it straight into device memory.  load's flags: LURK_MSM_FLAG_PRECOMPUTE
 * takes the file's table when it has one and rebuilds it on the device otherwise (one inversion per point: faster than
 * reading 13 x the bytes from disk unless the file is hot in the page cache). */
int lurk_hip_msm_ctx_save(const lurk_hip_msm_ctx* ctx, const char* path, int with_table);
int lurk_hip_msm_ctx_load(lurk_hip_msm_ctx** ctx, const char* path, int flags);
/* the same for a caller that knows which curve its key is over: a file that records another curve is refused (both curves named in
 * lurk_hip_last_error()) before anything is uploaded */
int lurk_hip_msm_ctx_load_curve(lurk_hip_msm_ctx** ctx, int curve, const char* path, int flags);

/* One process, several GPUs.  arecibo's prover is a single process (/root/reference/src/proof/nova.rs:304-326: one
 * witness-producer thread, rayon inside), so the multi-GPU form of the commitment is a context that owns a list
 * of devices: the key is cut into len(devices) contiguous slices (the first npoints % n_dev slices hold one more
 * point), every slice stays resident on its device, and a commit runs the slices concurrently (one host thread
 * per device inside the library), brings the 96-byte partial commitments back and sums them on the host.  A
 * device id may appear more than once (two slices on one GPU).  flags as for lurk_hip_msm_ctx_create.
 * commit takes the whole scalar vector in host memory; commit_dev takes one device pointer per slice (slice i's
 * scalars resident on slice i's device; entries of slices beyond nscalars are ignored). */
typedef struct lurk_hip_msm_multi lurk_hip_msm_multi;
int lurk_hip_msm_multi_create(lurk_hip_msm_multi** ctx, int curve, const void* bases_affine64, size_t npoints,
                              const int* devices, int n_dev, int flags);
int lurk_hip_msm_multi_num_shards(const lurk_hip_msm_multi* ctx);
int lurk_hip_msm_multi_shard(const lurk_hip_msm_multi* ctx, int index, int* device, size_t* first, size_t* count);
int lurk_hip_msm_multi_commit(lurk_hip_msm_multi* ctx, void* out_jacobian96, const void* scalars32, size_t nscalars,
                              int is_mont);
int lurk_hip_msm_multi_commit_dev(lurk_hip_msm_multi* ctx, void* out_jacobian96, const void* const* d_scalars32,
                                  size_t n_slices, size_t nscalars, int is_mont); /* n_slices must equal num_shards */
/* Asynchronous form (as lurk_hip_msm_ctx_submit_dev_mode / _wait, LURK_MSM_SLOTS slots): the slices of a commitment are submitted
 * from the calling thread and run concurrently on their devices; after_streams (or NULL) holds, per slice, the stream ON THAT
 * SLICE'S DEVICE that produced its scalars (e.g. the stream a peer copy into the device was enqueued on).  wait sums the partial
 * commitments.  Two slots give commit(W) and commit(T) of a folding step in flight on every device at once. */
int lurk_hip_msm_multi_submit_dev(lurk_hip_msm_multi* ctx, int slot, const void* const* d_scalars32, void* const* after_streams,
                                  size_t n_slices, size_t nscalars, int is_mont, int mode);
int lurk_hip_msm_multi_wait(lurk_hip_msm_multi* ctx, int slot, void* out_jacobian96);
int lurk_hip_msm_multi_destroy(lurk_hip_msm_multi* ctx);

/* Group helpers used by the multi-GPU gather (sum of per-rank partial commitments) and by tests:
 * out = sum of `count` Jacobian points (host memory, 96 B each). */
int lurk_hip_point_sum(int curve, void* out_jacobian96, const void* points_jacobian96, size_t count);
/* One process per GPU (a Rust host under MPI / its own launcher instead of one process with a device list): every rank commits its
 * slice of the vector under its slice of the key (lurk_hip_msm_ctx_*), the ranks all-gather the 96-byte partial commitments with
 * whatever transport they have (RCCL ncclAllGather on bytes, MPI_Allgather, a socket) into `gathered` (world x 96 B, rank order), and
 * THIS is the only library call the exchange needs: out = the commitment of the whole vector.  Host memory, no device touched; the
 * identity partial of a rank with an empty slice is handled.  (lurk_beta_amd/distributed.py drives exactly this from Python for the
 * tests and bench.py --gpus N: test plumbing, not a second ABI.) */
int lurk_hip_point_sum_gathered(int curve, void* out_jacobian96, const void* gathered_jacobian96, size_t world);
/* out = [scalar] point on the host (the transcript-side folding of commitments: comm_W1 + r comm_W2, comm_E1 + r comm_T) */
int lurk_hip_point_mul(int curve, void* out_jacobian96, const void* point_jacobian96, const void* scalar32, int is_mont);
/* Jacobian (Montgomery) -> canonical affine bytes (x, y), 64 B; identity -> all zero */
int lurk_hip_point_to_affine_canonical(int curve, void* out_xy64, const void* point_jacobian96);

/* ---- Poseidon ----------------------------------------------------------------------------
 * Replaces neptune's Poseidon::new_with_preimage(preimage, constants).hash() as called by
 * PoseidonCache::hash3/hash4/hash6/hash8 (/root/reference/src/hash.rs:180-204); constants are
 * PoseidonConstants::new() (standard strength, Merkle-tree domain tag; hash.rs:59-84).
 * preimages: n x arity x 32 B canonical; digests: n x 32 B canonical.  arity in {3,4,6,8}
 * (anything else fails, as HashArity::from panics, hash.rs:19-29). */
int lurk_hip_poseidon_batch(int field_id, int arity, const void* preimages, size_t n, void* digests);
int lurk_hip_poseidon_batch_dev(int field_id, int arity, const void* d_preimages, size_t n,
                                void* d_digests, void* stream);
/* Dense arity-8 tree (the dense analogue of coprocessor::trie::Trie,
 * /root/reference/src/coprocessor/trie/mod.rs:434-481): node = hash8(children in index order).
 * n_leaves must be a power of 8, >= 8.  levels_or_null (if given) receives every internal level,
 * level 1 first, root last: (n_leaves/8 + n_leaves/64 + ... + 1) x 32 B. */
int lurk_hip_poseidon_tree8(int field_id, const void* leaves, size_t n_leaves, void* root32,
                            void* levels_or_null);
/* device form: d_levels must hold (n_leaves-1)/7 elements (all internal levels, root last) */
int lurk_hip_poseidon_tree8_dev(int field_id, const void* d_leaves, size_t n_leaves, void* d_levels,
                                void* stream);
/* the constants the library generated (canonical): rc has (rf+rp)*(arity+1) elements, mds
 * (arity+1)^2; pass NULL to query sizes only */
int lurk_hip_poseidon_constants(int field_id, int arity, int* rf, int* rp, void* rc, void* mds);
/* n hashes on the HOST (no device needed): the same digests as lurk_hip_poseidon_batch, for callers that hash one preimage at a
 * time, as PoseidonCache::hash{3,4,6,8} does on a cache miss (/root/reference/src/hash.rs:180-204) - a single hash costs a host
 * core ~20 us and a kernel launch + copies several times that; batches belong on the device.  The store hydration below uses it
 * for DAG levels too narrow to be worth a kernel's dependency chain. */
int lurk_hip_poseidon_hash_host(int field_id, int arity, const void* preimages, size_t n, void* digests);

/* ---- the sparse Poseidon trie, resident on the device --------------------------------------------------------------------
 * Replaces coprocessor::trie::Trie<F, 8, HEIGHT> (/root/reference/src/coprocessor/trie/mod.rs) for bulk work: building the trie of n
 * (key, value) pairs, prove_lookup (:718-743) and prove_insert / modify_value_at_path (:751-800) for batches of keys, and
 * LookupProof::verify (:349-362) / InsertProof::verify (:383-424) for batches of proofs.  Arity 8; height H = 1 .. 85 (85 is the
 * StandardTrie, :43); fields LURK_FIELD_PALLAS_FP, _PALLAS_FQ and _BN254_FR.  Elements are canonical 32 B.
 *   path       the low 3 H bits of the key's canonical value (its PATH VALUE) read as H 3-bit digits, top digit first (:589-608);
 *              path order = numeric order of path values; two keys with one path value occupy one leaf
 *   empty      the empty element is 0; empty_roots[0] = hash8([0; 8]), empty_roots[i] = hash8([empty_roots[i-1]; 8]) (:464-481)
 *   node       hash8(children): the digests of lurk_hip_poseidon_batch, bit for bit
 *   proof      H preimages of 8 elements, root level first, the last one holding the payloads: H * 256 B per proof.  An absent subtree
 *              contributes [empty root below; 8] ([0; 8] at the leaf level), as the reference's init_empty registers them, so a lookup
 *              proof exists for an absent key (value 0).
 * Only lurk_hip_trie_path_digits runs without a device. */
typedef struct lurk_hip_trie lurk_hip_trie;
/* host only: the n * H path digits of n keys (key-major).  Bits at and above the field's NUM_BITS are ignored (no reduced key has them). */
int lurk_hip_trie_path_digits(int field_id, int height, const void* keys32, size_t n, uint8_t* digits);
/* The trie that holds exactly these n pairs.  Keys must be reduced and strictly increasing in path order: one device pass checks it, and
 * a violation is refused with LURK_HIP_ERR_INVALID_ARG, the message naming the first offending index and whether that key is "not
 * reduced", "out of order" or has a "duplicate path"; a refused call leaves nothing allocated.  n = 0 gives the empty trie; a value of 0
 * is legal (the empty element: that leaf hashes as if absent).  The caller's buffers are copied; the call synchronises `stream`.
 * The handle keeps on the device: the keys and the values (n * 32 B each), the hash of every non-empty node at every level (H arrays of
 * n elements: H * n * 32 B), one byte per key and the H + 1 empty roots - 178 MB of node hashes at H = 85, n = 2^16 (182 MB in all).
 * Built in at most H + 2 launches: the check, one launch in which every key hashes the part of its path it does not share with another
 * key, and one launch per depth at which two keys still share a node (about log8(n) + 1 for random keys).  An allocation failure comes
 * back as LURK_HIP_ERR_OOM with everything freed.  A built trie is not modified afterwards: lurk_hip_trie_insert_chain_dev gives a NEW
 * handle for the trie after a sequence of updates. */
int lurk_hip_trie_build_dev(lurk_hip_trie** t, int field_id, int height, const void* d_keys32, const void* d_values32, size_t n, void* stream);
int lurk_hip_trie_root(const lurk_hip_trie* t, void* root32);
/* any output may be NULL */
int lurk_hip_trie_info(const lurk_hip_trie* t, int* field_id, int* height, size_t* n, int* device);
int lurk_hip_trie_destroy(lurk_hip_trie* t);
/* prove_lookup for m keys, present or absent, in any order: d_paths receives m * H * 8 elements, d_values32 the m values (0 = absent).
 * Only the low 3 H bits of a key are read.  Reads the handle only: calls on several streams may run side by side.  Does not synchronise. */
int lurk_hip_trie_prove_lookup_dev(const lurk_hip_trie* t, const void* d_keys32, size_t m, void* d_paths, void* d_values32, void* stream);
/* m independent prove_inserts, each against the trie as built (the handle is not modified): the old path and value as above, the new path
 * = modify_value_at_path (the entry replaced bottom-up, H hashes), and the root after that one insertion.  d_old_paths and d_new_paths
 * (m * H * 8 elements each) may not overlap.  Does not synchronise. */
int lurk_hip_trie_prove_insert_dev(const lurk_hip_trie* t, const void* d_keys32, const void* d_new_values32, size_t m, void* d_old_paths, void* d_new_paths,
                                   void* d_old_values32, void* d_new_roots32, void* stream);
/* A CHAIN of m dependent inserts, as a host that calls Trie::insert / Trie::prove_insert (:745-776) step after step produces them: T_0 = t,
 * update i = (key_i, value_i) is applied to T_i and leaves T_{i+1}.  Per update: the old path (prove_lookup of key_i in T_i, laid out as
 * above) and the old value (0 = absent), the new path (modify_value_at_path) and d_roots32[i] = the root of T_{i+1}.  Keys may repeat, be
 * present in t or not, and share any number of leading digits; two keys with one path value are one leaf; a value of 0 is legal (that
 * leaf then hashes as if absent); an update that changes nothing repeats the previous root.
 *   outputs    each of d_old_paths, d_new_paths, d_old_values32, d_roots32 and out_trie may be NULL when it is not wanted; all five NULL is
 *              refused.  d_old_paths and d_new_paths (m * H * 8 elements each) may not overlap.
 *   out_trie   when non-NULL receives a NEW handle that holds T_m: the pairs of t merged on the device with the last update of every path
 *              value (a value of 0 stays a pair), sorted by path value and built by lurk_hip_trie_build_dev, from which it cannot be told
 *              apart; its root is d_roots32[m - 1].  The caller destroys it.  t itself is read only: chains on several streams may share
 *              it.  With m = 0, out_trie holds a copy of t's pairs and nothing else is written.  Not written when the call fails.
 *   refusals   keys and values must be reduced: both are read back and checked on the host first, a violation is LURK_HIP_ERR_INVALID_ARG
 *              with the first offending index in the message, and nothing has been launched or allocated by then.  m <= 2^28.
 *   work       the m * H hashes of the sequential loop at a dependency depth of H: one hashing launch per depth, bottom-up, one update
 *              per lane.  What an update finds in a node is the node's preimage in T_0 with every child replaced by the new hash of the
 *              latest earlier update through that child; that update is found by binary search in the updates ordered by (prefix,
 *              sequence index), one stable sort (rocprim) and one 4-byte read-back per depth at which two different keys still share a
 *              node - about 2 log8(m) depths for random keys, H at the most.  The number of launches does not depend on m.
 *   scratch    freed before the call returns: 8 B per update and depth for the orders (680 B per update at H = 85), 80 B per update of
 *              work space and hashes, the sort's temporary storage, and - ONLY when d_old_paths is NULL - the m * H * 256 B of old paths,
 *              which the call then keeps to itself (the preimages of T_0 are written where the old paths go and patched in place; they
 *              are not recomputed per level).  An allocation failure is LURK_HIP_ERR_OOM with everything freed and no handle written.
 * The call synchronises `stream`. */
int lurk_hip_trie_insert_chain_dev(const lurk_hip_trie* t, const void* d_keys32, const void* d_values32, size_t m, void* d_old_paths, void* d_new_paths,
                                   void* d_old_values32, void* d_roots32, lurk_hip_trie** out_trie, void* stream);
/* LookupProof::verify per proof.  root_stride: 0 = d_roots32 is one root for every proof, 1 = one root per proof.  d_codes[i]: 0 =
 * accepted; k + 1 = the hash of preimage k is not the expected node (level 0 is checked against the root) or preimage k holds an element
 * that is not reduced; H + 1 = the selected leaf entry is not the value.  *n_failed (host) = the number of non-zero codes; the call
 * synchronises `stream`.  Keys and values that are not reduced are refused before anything is launched. */
int lurk_hip_trie_verify_lookup_dev(int field_id, int height, const void* d_roots32, size_t root_stride, const void* d_keys32, const void* d_values32,
                                    const void* d_paths, size_t m, uint32_t* d_codes, uint64_t* n_failed, void* stream);
/* InsertProof::verify per proof, in the reference's order, the first failing check giving the code: the old proof (1 .. H + 1 as above; an
 * absent old value is passed as 0), then at every level the two preimages equal or different in at most one position (0x100 + level + 1),
 * then the new proof (0x200 + 1 .. H + 1). */
int lurk_hip_trie_verify_insert_dev(int field_id, int height, const void* d_old_roots32, const void* d_new_roots32, size_t root_stride, const void* d_keys32,
                                    const void* d_old_values32, const void* d_new_values32, const void* d_old_paths, const void* d_new_paths, size_t m,
                                    uint32_t* d_codes, uint64_t* n_failed, void* stream);

/* ---- root-addressed tries: the trie's child map resident on the device ------------------------------------------------------
 * The reference's trie is addressed by its ROOT: every version of every trie lives in one child map, digest -> 8-element preimage
 * (InversePoseidonCache::a8, /root/reference/src/hash.rs:116-166, written by register_hash, src/coprocessor/trie/mod.rs:453-458), the
 * coprocessors rebuild a trie from a root (Trie::new_with_root, :566-576) and walk the map from it (prove_lookup_at_path, :725-743).
 * lurk_hip_trie_nodes is that map for one (field, height) in device memory: content-addressed and append-only (registering a digest
 * that is present is a no-op; nothing is ever removed, so a root stays valid), arity 8, height 1 .. 85, the three fields of the trie
 * calls, canonical 32-byte elements, paths laid out as the trie calls lay them out (m * H * 8 elements, root level first).
 *
 * The store is an open-addressing table with a power-of-two slot count: a 64-bit tag (0 = empty), the 32 B digest and the 256 B
 * preimage per slot, 296 B per slot, at most half the slots taken.  Before a batch would take more than half, the table is rebuilt at
 * the next sufficient power of two (one allocation, one re-insert launch, one free); an allocation that fails is LURK_HIP_ERR_OOM with
 * the store unchanged.  A trie of 2^16 keys at H = 85 has about 5.6 M nodes: 2^24 slots, 4.97 GB (against 178 MB for the handle, which
 * holds ONE version; every further version of that trie adds at most H nodes per update).  n_nodes is exact: the number of distinct
 * digests registered, whatever the batches held.  LURK_TRIE_NODES_TAG_BITS keeps fewer tag bits, for tests.
 *
 * Calls that register (create, register_dev, add_trie, prove_insert_dev with register_new, insert_chain_dev) synchronise `stream` - the
 * host learns n_nodes - and must not run while another call on the same store is in flight; get_dev, prove_lookup_dev and
 * prove_insert_dev without register_new only read, and may run side by side on several streams.  Every call requires the store's device
 * to be the calling thread's current one and refuses otherwise with nothing launched. */
typedef struct lurk_hip_trie_nodes lurk_hip_trie_nodes;
/* init_empty (:464-481): the H preimages of the empty chain are registered, n_nodes == height.  reserve_nodes: how many nodes the table
 * should hold before it first grows (0 = the minimum). */
int lurk_hip_trie_nodes_create(lurk_hip_trie_nodes** ns, int field_id, int height, size_t reserve_nodes);
int lurk_hip_trie_nodes_destroy(lurk_hip_trie_nodes* ns);
/* any output may be NULL; host only */
int lurk_hip_trie_nodes_info(const lurk_hip_trie_nodes* ns, int* field_id, int* height, size_t* n_nodes, size_t* slots, int* device);
/* register_hash for a batch: hash8 of `count` preimages (count * 8 elements; the batch hasher's permutation), every (digest, preimage)
 * inserted, the digests written to d_digests_out when it is non-NULL.  A preimage element that is not reduced refuses the call before
 * anything is hashed: "preimage element <i> is not reduced" (i counts elements, lowest first). */
int lurk_hip_trie_nodes_register_dev(lurk_hip_trie_nodes* ns, const void* d_preimages, size_t count, void* d_digests_out, void* stream);
/* Every node of a built handle (same field and height), with no hash computed: the digests are read from the handle's level arrays and
 * the preimages gathered from the level below.  At most n * H - sum(shared digits of neighbouring keys) nodes; n = 0 adds nothing. */
int lurk_hip_trie_nodes_add_trie(lurk_hip_trie_nodes* ns, const lurk_hip_trie* trie, void* stream);
/* InversePoseidonCache::get for m digests: d_preimages m * 8 elements, d_found[j] 1 or 0; a digest that is not in the store gives a
 * zero row.  Stream-ordered: does not synchronise. */
int lurk_hip_trie_nodes_get_dev(const lurk_hip_trie_nodes* ns, const void* d_digests32, size_t m, void* d_preimages, uint32_t* d_found, void* stream);
/* new_with_root + prove_lookup per query: query i walks from d_roots32[i * root_stride] (root_stride 0 = one root for every query, 1 =
 * one per query; roots of several versions may be mixed).  d_status[i]: 0 = found (d_paths and d_values32 as
 * lurk_hip_trie_prove_lookup_dev writes them); k + 1 = the node expected at level k is not in the store (Error::MissingPreimage, :738):
 * rows k .. H - 1 of that path and the value are then zero.  *n_missing (host, may be NULL) = the number of non-zero statuses; the walk is
 * stream-ordered and the call waits for it only when n_missing is non-NULL.  Keys and roots that are not reduced are refused by name before
 * anything is launched (that check copies them to the host and waits for `stream`). */
int lurk_hip_trie_nodes_prove_lookup_dev(const lurk_hip_trie_nodes* ns, const void* d_roots32, size_t root_stride, const void* d_keys32, size_t m, void* d_paths,
                                         void* d_values32, uint32_t* d_status, uint64_t* n_missing, void* stream);
/* m independent new_with_root + prove_insert (:751-800), query i at its own root: outputs as lurk_hip_trie_prove_insert_dev, d_status and
 * n_missing as above; a query with a non-zero status writes zero rows to d_new_paths and a zero new root, and registers nothing.
 * register_new != 0: the m * H new nodes are registered from the hashes just computed (nothing is hashed twice), every new root is
 * addressable when the call returns, and the call synchronises.  register_new == 0: the store is unchanged. */
int lurk_hip_trie_nodes_prove_insert_dev(lurk_hip_trie_nodes* ns, const void* d_roots32, size_t root_stride, const void* d_keys32, const void* d_new_values32,
                                         size_t m, void* d_old_paths, void* d_new_paths, void* d_old_values32, void* d_new_roots32, uint32_t* d_status,
                                         uint64_t* n_missing, int register_new, void* stream);
/* lurk_hip_trie_insert_chain_dev with T_0 named by a root (root32_host: 32 canonical bytes in HOST memory): update i is applied to T_i and
 * leaves T_{i + 1}; outputs as there, each may be NULL.  All m keys are walked in T_0 first; a miss refuses the whole call with
 * LURK_HIP_ERR_INVALID_ARG, "update <i>: missing preimage at level <k>" (lowest i), nothing hashed or registered (the old-path and
 * old-value buffers are then unspecified).  Otherwise every new node of every T_i is registered: all m roots d_roots32[i] are addressable,
 * the result is d_roots32[m - 1]. */
int lurk_hip_trie_nodes_insert_chain_dev(lurk_hip_trie_nodes* ns, const void* root32_host, const void* d_keys32, const void* d_values32, size_t m,
                                         void* d_old_paths, void* d_new_paths, void* d_old_values32, void* d_roots32, void* stream);

/* ---- store hydration -----------------------------------------------------------------------
 * Replaces the recursive, node-by-node hashing of StoreCore::hydrate_z_cache / hash_ptr
 * (/root/reference/src/lem/store_core.rs:256-269) with the StoreHasher preimage layouts
 * (/root/reference/src/lem/store.rs:29-78).  nodes: the DAG in topological order (children before parents); the digest of
 * every node is written to digests32 (n x 32 B canonical; an atom's digest is its value).  Every level is hashed on the
 * device - one preimage gather + one Poseidon batch per (level, arity) - and nothing crosses PCIe in between.
 * *levels (optional) receives the depth of the DAG.  Tags are the u16 tag values of /root/reference/src/tag.rs. */
#define LURK_NODE_ATOM 0    /* digest = values32[value]                                   (store_core.rs:204) */
#define LURK_NODE_TUPLE2 2  /* hash4(tag_a, h_a, tag_b, h_b)                              (store.rs:32-36) */
#define LURK_NODE_TUPLE3 3  /* hash6(...)                                                 (store.rs:37-49) */
#define LURK_NODE_TUPLE4 4  /* hash8(...)                                                 (store.rs:50-65) */
#define LURK_NODE_COMPACT 5 /* hash4(h_a, tag_b, h_b, h_c)                                (store.rs:75-77) */
#define LURK_NODE_COMM 6    /* hash3(values32[value] = secret, tag_a, h_a)                (store.rs:70-73) */
typedef struct {
    uint32_t kind;     /* LURK_NODE_* */
    uint32_t tag;      /* the tag a parent's preimage records for this node */
    uint32_t child[4]; /* indices of earlier nodes (tuple2: 2, tuple3: 3, tuple4: 4, compact: 3, comm: 1) */
    uint32_t value;    /* atom: index of its value; comm: index of the secret */
    uint32_t reserved;
} lurk_hip_store_node;
int lurk_hip_store_hydrate(int field_id, const lurk_hip_store_node* nodes, size_t n, const void* values32, size_t n_values,
                           void* digests32, size_t* levels);

/* ---- the store, resident on the device -----------------------------------------------------------------------------------
 * lurk_hip_store_hydrate is one shot: the whole DAG up, every node hashed, every digest down.  StoreCore is append-only and keeps its
 * digest memo (z_cache) for its whole life (/root/reference/src/lem/store_core.rs:199-248); hydrate_z_cache (:256-269) hashes what has
 * been interned since the last hydration, and Prover::prove hydrates before every proof (/root/reference/src/proof/mod.rs:180-198).
 * A lurk_hip_store is that memo in HBM; fields LURK_FIELD_PALLAS_FP, _PALLAS_FQ and _BN254_FR (another id: "unknown field id").
 *   node ids   assigned in append order, the first node ever appended is 0; a store holds fewer than 2^31 nodes
 *   device     per node id the canonical digest (32 B; an atom's digest is its value) and the tag (4 B): 36 B per node of capacity
 *   host       per node its level, its tag, and a copy of the digest of the nodes the host hashed or once fetched (below)
 *   threads    appends to one store are serialised by the library; the two _dev readers may run on any stream once an append has
 *              returned.  An append concurrent with readers of the same store is the caller's error (growth moves the arrays).
 * Nodes are not interned or deduplicated: the host's Store interns, and ids are the caller's.  Every call must be made with the store's
 * device current (lurk_hip_store_info's *device). */
typedef struct lurk_hip_store lurk_hip_store;
/* reserve_nodes: the initial capacity, 0 = the library's default (2^16).  Capacity grows geometrically on demand (at least doubling), the
 * resident arrays moved by ONE device-to-device copy; the digest array never crosses PCIe, at any growth. */
int lurk_hip_store_create(lurk_hip_store** s, int field_id, size_t reserve_nodes);
int lurk_hip_store_destroy(lurk_hip_store* s);
/* any output may be NULL.  *levels: the depth of the DAG held (an atom is level 0); *hashes_done: the Poseidon hashes performed since
 * creation, on the host and on the device - after any sequence of appends it equals the number of non-atom nodes, each hashed once. */
int lurk_hip_store_info(const lurk_hip_store* s, int* field_id, size_t* n_nodes, size_t* levels, size_t* hashes_done, size_t* capacity, int* device);
/* n_new further nodes, which receive the ids *first_id .. *first_id + n_new - 1 (first_id may be NULL).  The records are those of
 * lurk_hip_store_hydrate with
 *   child[k]   a GLOBAL node id, smaller than the id the node itself receives: from an earlier append or from earlier in this batch
 *              (any prefix of a topologically ordered DAG is a valid batch)
 *   value      (an atom's value, a commitment's secret) an index into THIS call's values32 (n_values x 32 B canonical, reduced); no
 *              value array stays resident
 * Only the new nodes are hashed, grouped by (level, arity) as the one-shot call groups them: a group of more than 6 nodes is one gather
 * of its preimages from the resident arrays and one batch of the Poseidon kernel, a narrower one goes to the library's host Poseidon.
 * Within the append, digests change sides as in the one-shot call (one copy when a group changes sides), so appending a whole DAG in
 * one call costs about what lurk_hip_store_hydrate costs.  Digests of children from EARLIER appends that a narrow group needs and the
 * host holds no copy of come down once per append (one indexed gather, one copy).  Host-hashed digests are in the device array before
 * the call returns.  new_digests32_or_null: NULL, or n_new x 32 B for the digests of the new nodes - with NULL no digest crosses PCIe but
 * those narrow groups need.  The call synchronises (the null stream).
 *   refusals   every argument is checked on the host before anything is allocated, launched or changed; a refused append leaves the
 *              store exactly as it was.  LURK_HIP_ERR_INVALID_ARG, the message opening with "record <i>: " for the first offending
 *              record i of this call: "unknown node kind"; "nodes must be in topological order (children first)" (a child id that is
 *              not smaller than the node's own, within or beyond the store); "atom value index out of range" / "commitment secret
 *              index out of range"; "value <v> is not reduced modulo the field order".  "too many nodes" at 2^31.
 *   growth     an allocation failure, of the grown arrays or of the call's scratch, is LURK_HIP_ERR_OOM with the store unchanged
 * n_new == 0 is legal and does nothing. */
int lurk_hip_store_append(lurk_hip_store* s, const lurk_hip_store_node* nodes, size_t n_new, const void* values32, size_t n_values, size_t* first_id,
                          void* new_digests32_or_null);
/* d_out32[j] = the digest of node d_ids[j] (device arrays, m < 2^31).  Stream-ordered, does not synchronise.  The ids are not read on the
 * host: an id >= n_nodes reads nothing and its row is ZERO. */
int lurk_hip_store_digests_dev(const lurk_hip_store* s, const uint32_t* d_ids, size_t m, void* d_out32, void* stream);
/* the same with host arrays; an id >= n_nodes is refused ("id <j> is out of range").  Synchronises. */
int lurk_hip_store_digests(const lurk_hip_store* s, const uint32_t* ids, size_t m, void* out32);
/* The preimages of a MultiFrame's hash slots straight from the resident digests: element j of d_out is the element d_elems[j]
 * describes, canonical or - as_mont - Montgomery (one product per element).  allocate_slot (/root/reference/src/lem/circuit.rs:249-315)
 * builds a slot's preimage from its SlotData, value by value (:265-292):
 *   Val::Pointer(ptr)    ->  TAG(id), DIGEST(id)      (store.hash_ptr(ptr): its tag, then its hash, :270-277)
 *   Val::Num(ptr_val)    ->  DIGEST(id)               (store.hash_ptr_val(ptr_val).0: id names the node of that value, :278-284)
 *   Val::Boolean(b)      ->  CONST(b)                 (ONE or ZERO, :285-291)
 *   an absent slot       ->  ZERO x arity             (the dummy preimage, :300-308)
 * With the descriptors of num_frames x count slots of one type in frame-major order, d_out (n_elems x 32 B) is what
 * lurk_hip_frames_witness_dev and lurk_hip_slot_witness_dev read as their d_preimages: n x arity x 32 B.  A TAG or DIGEST whose id is
 * >= n_nodes reads nothing and gives ZERO, and so does an unknown kind.  n_elems < 2^31.  Stream-ordered, does not synchronise. */
#define LURK_SLOT_ELEM_ZERO 0
#define LURK_SLOT_ELEM_TAG 1    /* arg = node id: that node's tag */
#define LURK_SLOT_ELEM_DIGEST 2 /* arg = node id: that node's digest */
#define LURK_SLOT_ELEM_CONST 3  /* arg itself: booleans, literal tags */
typedef struct {
    uint32_t kind; /* LURK_SLOT_ELEM_* */
    uint32_t arg;
} lurk_hip_slot_elem;
int lurk_hip_store_slot_preimages_dev(const lurk_hip_store* s, const lurk_hip_slot_elem* d_elems, size_t n_elems, int as_mont, void* d_out, void* stream);

/* ---- slot witnesses: the Poseidon / bit-decomposition part of the witness vector, produced on the device ------------
 * Replaces generate_slots_witnesses (/root/reference/src/lem/multiframe.rs:520-592), which runs allocate_slot
 * (/root/reference/src/lem/circuit.rs:242-315) on a WitnessCS per slot: neptune's circuit2::poseidon_hash_allocated for
 * the Hash4 / Hash6 / Hash8 / Commitment slots (circuit.rs:212-235) and bellpepper's to_bits_le_strict for the BitDecomp
 * slots (circuit.rs:236-238).  A slot's block in W is, in the circuit's allocation order,
 *     hash slots:  [preimage (arity) | l^2, l^4, l^5 + key for every S-box | digest]
 *     bit decomp:  [value | bits of the value from the top, with the AND chain closing every run of 1-bits of p - 1]
 * as 32-byte Montgomery values: about 85 % of the step circuit's W (7 808 of 9 119 aux per frame on BN254,
 * /root/reference/src/lem/eval.rs:1960-1966).  With these W is assembled in HBM - [globals | frame 0 | frame 1 | ...],
 * each frame = its slots' blocks back to back, then the rest of the frame's aux (multiframe.rs:699-702,
 * circuit.rs:1429-1433) - and handed to lurk_hip_msm_ctx_submit_dev / lurk_hip_r1cs_cross_term_dev without crossing PCIe.
 * slot_type: the arity for hash slots (LURK_SLOT_COMMITMENT = 3, HASH4 = 4, HASH6 = 6, HASH8 = 8) or LURK_SLOT_BIT_DECOMP. */
#define LURK_SLOT_BIT_DECOMP 1
#define LURK_SLOT_COMMITMENT 3
#define LURK_SLOT_HASH4 4
#define LURK_SLOT_HASH6 6
#define LURK_SLOT_HASH8 8
/* elements per slot block = compute_witness_size (multiframe.rs:503-516); host-only, needs no device */
int lurk_hip_slot_witness_size(int field_id, int slot_type, size_t* size);
/* n slots of one type: preimages n x (arity | 1) x 32 B (Montgomery if preimages_mont, else canonical); slot i's block is
 * written at element d_w[d_offsets[i]] (device array) or, with d_offsets == NULL, at d_w[first + i * stride] */
int lurk_hip_slot_witness_dev(int field_id, int slot_type, const void* d_preimages, size_t n, int preimages_mont, void* d_w,
                              const uint64_t* d_offsets, size_t first, size_t stride, void* stream);
/* host buffers in and out, blocks back to back (n x size x 32 B): small inputs and tests */
int lurk_hip_slot_witness(int field_id, int slot_type, const void* preimages, size_t n, int preimages_mont, void* w_out);
/* every slot block of a MultiFrame in one call: counts5 / d_preimages5 are indexed (hash4, hash6, hash8, commitment, bit_decomp)
 * - the order generate_slots_witnesses walks a frame's hints in (multiframe.rs:527-536) - with counts per frame and, per type,
 * num_frames * count preimages in frame-major order.  Frame f's slot blocks are written back to back from
 * d_w[first + f * frame_len].  The per-type launches run concurrently inside; ordered after and before `stream`. */
int lurk_hip_frames_witness_dev(int field_id, size_t num_frames, const size_t* counts5, const void* const* d_preimages5,
                                int preimages_mont, void* d_w, size_t first, size_t frame_len, void* stream);
/* places n_blocks packed blocks of block_len elements (host or device memory) at d_w[first + b * stride]: the globals and
 * the non-slot remainder of every frame, which the CPU synthesis still produces */
int lurk_hip_witness_blocks_dev(void* d_w, size_t first, size_t stride, const void* src, int src_on_host, size_t n_blocks,
                                size_t block_len, void* stream);

/* The constraint rows of one slot: what neptune's circuit2::poseidon_hash_allocated (three rows per S-box - l * l = l2, l2 * l2 = l4,
 * l4 * l = l5k - key, the S-box inputs being linear combinations carried through the linear layers - and the digest's ensure_allocated
 * row) and bellpepper's to_bits_le_strict (a boolean row per bit, the AND chains, the unpacking row) enforce on the block
 * lurk_hip_slot_witness* writes, as three CSR matrices {indptr (num_cons + 1), indices, data (32 B Montgomery)} like lurk_hip_r1cs_create
 * takes.  Local column k < size is element k of the slot's block, local column `size` (lurk_hip_slot_witness_size) is the constant
 * ONE.  Rows in the gadget's emission order, columns ascending within a row, no coefficient that reduces to zero; an empty linear
 * combination (the boolean rows' C) is an empty CSR row.  Host-only like lurk_hip_slot_witness_size; every output is required. */
int lurk_hip_slot_constraints_size(int field_id, int slot_type, size_t* num_cons, size_t* nnz_a, size_t* nnz_b, size_t* nnz_c);
int lurk_hip_slot_constraints(int field_id, int slot_type, uint64_t* a_indptr, uint64_t* a_indices, void* a_data, uint64_t* b_indptr,
                              uint64_t* b_indices, void* b_data, uint64_t* c_indptr, uint64_t* c_indices, void* c_data);
/* A resident shape (as lurk_hip_r1cs_create makes) of every slot row of a MultiFrame at the layout lurk_hip_frames_witness_dev writes:
 * rows frame-major, within a frame the slots in that call's order (hash4, hash6, hash8, commitment, bit_decomp; counts5 per frame), each
 * slot's rows relocated to its block (first + f * frame_len + the slot's offset); ONE maps to column num_vars - the u position of
 * z = [W | u | X], so constants relax with u as in Nova.  The caller's extra_cons further rows (the non-slot body of the circuit, which
 * CPU synthesis still produces; nine CSR pointers over the num_vars + 1 + num_io columns, all NULL when extra_cons == 0) are appended
 * unchanged after the slot rows.  The result is an ordinary lurk_hip_r1cs: multiply_vec, cross_term, cross_term_cached, is_sat,
 * lurk_hip_fold_ctx_create and lurk_hip_spartan_prove_dev take it as they take any shape; destroy it with lurk_hip_r1cs_destroy.
 * Refused before any allocation: a block that would reach past num_vars, a count that overflows, an unknown field.
 * The ORDER of the slot rows relative to the rest of lurk-beta's real circuit is unpinned: the reference holds no vector for it (as
 * for the aux order of the slot blocks).  The call is for checking a traced W, for benchmarking on the slot gadgets' real row mix and
 * for cross-checking a host's own shape; it does not replace the host's R1CSShape. */
typedef struct lurk_hip_r1cs lurk_hip_r1cs;
int lurk_hip_frames_r1cs_create(lurk_hip_r1cs** shape, int field_id, size_t num_frames, const size_t* counts5, size_t first,
                                size_t frame_len, size_t num_vars, size_t num_io, size_t extra_cons, const uint64_t* xa_indptr,
                                const uint64_t* xa_indices, const void* xa_data, const uint64_t* xb_indptr, const uint64_t* xb_indices,
                                const void* xb_data, const uint64_t* xc_indptr, const uint64_t* xc_indices, const void* xc_data);

/* ---- the trie coprocessor's step circuits: witness on the device, rows, resident shape --------------------------------------------
 * LookupCoprocessor and InsertCoprocessor are NIVC step circuits whose bodies are Trie::synthesize_lookup and Trie::synthesize_insert
 * (/root/reference/src/coprocessor/trie/mod.rs:652-714, 802-880).  These calls cover exactly those two functions, given allocated_root, key
 * (and value): the block of W they allocate and the rows they enforce.  The wrappers around them (synthesize_*_aux: the
 * allocated_root_value allocation, implies_equal under not_dummy, the AllocatedPtr tags, the globals) stay with the host, as the non-slot
 * body of a frame does, and arrive as extra_cons.  Arity 8, H = 1 .. 85, fields LURK_FIELD_PALLAS_FP, _PALLAS_FQ and _BN254_FR.
 * LOOKUP block, local columns in allocation order; B = lurk_hip_slot_witness_size(LURK_SLOT_BIT_DECOMP) (301 / 298 / 354 for field 0 / 1 /
 * 2), size = 1 + B + 403 H:
 *     0                      allocated_root
 *     1 .. B                 the bit-decomposition slot block of the key (synthesize_path, :611-629), as lurk_hip_slot_witness* writes it
 *     1 + B + 403 i + ...    level i = 0 .. H - 1, root level first: the hash8 slot block of path preimage i (396: [8 preimage | 387 S-box
 *                            aux | digest]), then the seven picks of select (/root/reference/src/circuit/gadgets/constraints.rs:334-391):
 *                            three rounds of 4, 2 and 1 picks, round r on the digit's bit 2 - r, pick (r, j) taking a = state[half + j],
 *                            b = state[j]; a pick's value is a copy of one of its inputs
 *   The digit of level i is key bits 3 (H - 1 - i) .. + 2; bits at and above the field's NUM_BITS are Boolean::Constant(false) (BN254 at
 *   H = 85 only: bit 254).  result_col (`found`) is the last pick of level H - 1.
 * LOOKUP rows, emission order, Rb + 396 H of them (Rb = the bit-decomposition slot's rows): that slot's rows; then per level the 388
 * hash8 slot rows, hashed * 1 = next (enforce_equal, constraints.rs:14-31; next = the root at level 0, else the previous level's last pick)
 * and seven pick rows (b - a) * cond = (b - c), B an empty row where cond is the constant false.
 * INSERT = the lookup block and rows (synthesize_insert_at_path runs the lookup first), then value_col - one element for the new value -
 * and, from the leaf level upward (synthesize_modify_value_at_path, :846-880), the hash8 slot block (396) and rows (388) of that level's new
 * preimage: size = size_lookup + 1 + 396 H, Rb + 784 H rows, result_col = the last digest (the new root).  As in the reference, no row
 * ties a new preimage's entries to the old preimage, to the value or to the digest below it: synthesize_modify_value_at_path allocates
 * them with those values and enforces nothing.
 * Rows follow the slot rows' contract: columns ascending within a row, no coefficient that reduces to zero, an empty linear combination
 * is an empty CSR row, local column `size` is the constant ONE.  The two inner gadgets are the slot gadgets' rows relocated. */
#define LURK_TRIE_CIRCUIT_LOOKUP 0
#define LURK_TRIE_CIRCUIT_INSERT 1
/* host only.  value_col: the new value's column (insert); not written, and may be NULL, for a lookup.  Every other output is required. */
int lurk_hip_trie_circuit_size(int field_id, int height, int op, size_t* size, size_t* num_cons, size_t* nnz_a, size_t* nnz_b, size_t* nnz_c,
                               size_t* result_col, size_t* value_col);
/* host only: the rows as three CSR matrices {indptr (num_cons + 1), indices, data (32 B Montgomery)}; every output is required */
int lurk_hip_trie_circuit_constraints(int field_id, int height, int op, uint64_t* a_indptr, uint64_t* a_indices, void* a_data, uint64_t* b_indptr,
                                      uint64_t* b_indices, void* b_data, uint64_t* c_indptr, uint64_t* c_indices, void* c_data);
/* A resident shape of n_blocks such circuits, block b's rows relocated to columns first + b * stride (rows block-major), ONE mapped to
 * column num_vars (the u position of z = [W | u | X]); the caller's extra_cons rows over the num_vars + 1 + num_io columns (nine CSR
 * pointers, all NULL when extra_cons == 0) are appended unchanged.  Refusals before any allocation and the result - an ordinary
 * lurk_hip_r1cs - as for lurk_hip_frames_r1cs_create. */
int lurk_hip_trie_circuit_r1cs_create(lurk_hip_r1cs** shape, int field_id, int height, int op, size_t n_blocks, size_t first, size_t stride,
                                      size_t num_vars, size_t num_io, size_t extra_cons, const uint64_t* xa_indptr, const uint64_t* xa_indices,
                                      const void* xa_data, const uint64_t* xb_indptr, const uint64_t* xb_indices, const void* xb_data,
                                      const uint64_t* xc_indptr, const uint64_t* xc_indices, const void* xc_data);
/* The blocks of m circuits, written as 32-byte Montgomery values: block i at d_w[d_offsets[i]] (device array) or, with d_offsets == NULL,
 * at d_w[first + i * stride].  Inputs are canonical 32 B on the device, as the trie calls leave them: lurk_hip_trie_prove_lookup_dev's
 * d_paths as d_old_paths; lurk_hip_trie_prove_insert_dev's and lurk_hip_trie_insert_chain_dev's d_old_paths / d_new_paths (m * H * 8
 * elements, root level first).  Block i's root is d_roots32[i * root_stride], root_stride 0 (one root for every block) or 1.  For a
 * CHAIN the root of block i is the root of T_i: the caller passes [root(T_0), then lurk_hip_trie_insert_chain_dev's d_roots32[0 .. m - 2]]
 * with root_stride 1.  For a lookup d_new_values32 and d_new_paths must be NULL.
 * The call does not judge the proof: it writes what synthesis would allocate from these inputs, and a wrong proof gives a W the rows do
 * not accept.  Inputs are not checked to be reduced.  Work: m H hash8 traces (2 m H for an insert), each reading its preimage from the
 * path buffer, in two launches whatever m and H.  Refused before any launch: an unknown field, op or height, a NULL buffer with m > 0,
 * m > 2^28, a stride shorter than a block.  Does not synchronise. */
int lurk_hip_trie_circuit_witness_dev(int field_id, int height, int op, const void* d_roots32, size_t root_stride, const void* d_keys32,
                                      const void* d_new_values32, const void* d_old_paths, const void* d_new_paths, size_t m, void* d_w,
                                      const uint64_t* d_offsets, size_t first, size_t stride, void* stream);

/* ---- NTT ---------------------------------------------------------------------------------
 * No reference counterpart: radix-2 NTT over a Pasta field, natural order in
 * and out, omega = 5^((p-1)/2^32)^(2^(32-log_n)); inverse includes the 1/n scaling.  log_n <= 28; field_id 0 or 1.
 * Input: n canonical field elements (< p, 4 x u64 little-endian each); other values give unspecified results.  Output: n
 * canonical field elements.  A refused call (log_n, field, null buffer) returns an error before any launch or copy. */
int lurk_hip_ntt(int field_id, void* inout, unsigned log_n, int inverse);
int lurk_hip_ntt_dev(int field_id, void* d_inout, unsigned log_n, int inverse, void* stream);

/* ---- relaxed-R1CS folding -----------------------------------------------
 * The arithmetic arecibo's NIFS::prove runs on the CPU between the two commitments of a folding step
 * (caller: RecursiveSNARK::prove_step, /root/reference/src/proof/nova.rs:291-293; arecibo is the
 * un-vendored `nova` dependency, /root/reference/Cargo.toml:128): with these the witness vectors
 * stay in HBM from commit(W) through commit(T) to the next step.
 * Shape = the three CSR matrices as arecibo's SparseMatrix {data, indices, indptr} holds them:
 * indptr (num_cons + 1) x usize, indices nnz x usize (column into z = [W | u | X], i.e.
 * num_vars + 1 + num_io columns), data nnz x 32 B Montgomery.  Copied to the device at creation
 * (coefficients de-duplicated into a dictionary); the host arrays are only borrowed for the call. */
int lurk_hip_r1cs_create(lurk_hip_r1cs** shape, int field_id, size_t num_cons, size_t num_vars,
                         size_t num_io, const uint64_t* a_indptr, const uint64_t* a_indices,
                         const void* a_data, const uint64_t* b_indptr, const uint64_t* b_indices,
                         const void* b_data, const uint64_t* c_indptr, const uint64_t* c_indices,
                         const void* c_data);
/* The same shape over the SCALAR field of `curve` (Pallas: LURK_FIELD_PALLAS_FQ, Vesta: LURK_FIELD_PALLAS_FP, BN254:
 * LURK_FIELD_BN254_FR, Grumpkin: LURK_FIELD_BN254_FQ): validation, dictionary and long-row list are lurk_hip_r1cs_create's.  The one
 * way to a shape over the BN254 base field - lurk_hip_r1cs_create keeps refusing field id 3 - for the circuit a folding context on
 * Grumpkin folds (the default cycle's secondary half).  lurk_hip_r1cs_dims reports the field id.  A shape over LURK_FIELD_BN254_FQ is
 * served by lurk_hip_r1cs_multiply_vec(_dev), lurk_hip_r1cs_cross_term(_dev), lurk_hip_r1cs_cross_term_cached_dev,
 * lurk_hip_r1cs_is_sat_dev, lurk_hip_r1cs_read, _info, _dims, _device, _destroy and lurk_hip_fold_ctx_create(_multi); everything else
 * that takes a shape (lurk_hip_r1cs_transpose_dev, lurk_hip_r1cs_sparse_mle_dev, the compressing provers and verifiers) refuses it with
 * nothing launched.  An unknown curve id is refused by name. */
int lurk_hip_r1cs_create_for_curve(lurk_hip_r1cs** shape, int curve, size_t num_cons, size_t num_vars,
                                   size_t num_io, const uint64_t* a_indptr, const uint64_t* a_indices,
                                   const void* a_data, const uint64_t* b_indptr, const uint64_t* b_indices,
                                   const void* b_data, const uint64_t* c_indptr, const uint64_t* c_indices,
                                   const void* c_data);
int lurk_hip_r1cs_destroy(lurk_hip_r1cs* shape);
int lurk_hip_r1cs_dims(const lurk_hip_r1cs* shape, int* field_id, size_t* num_cons, size_t* num_vars, size_t* num_io);
int lurk_hip_r1cs_info(const lurk_hip_r1cs* shape, size_t* nnz_a, size_t* nnz_b, size_t* nnz_c,
                       size_t* distinct_coefficients);
int lurk_hip_r1cs_device(const lurk_hip_r1cs* shape, int* device); /* the device the shape is resident on */
/* The transpose of a resident shape, made on the device it is resident on: what lurk_hip_spartan_prove_dev / _prove_batch_dev and
 * lurk_hip_spartan_kzg_prove_dev / _prove_batch_dev take as shape_t (rows_t = 2 * num_vars), without a host CSR - so a shape the
 * library built itself (lurk_hip_frames_r1cs_create) can be compressed.  With ncols = num_vars + 1 + num_io of the source, *out is an
 * ordinary lurk_hip_r1cs over the same field with num_cons' = rows_t (0 means ncols), num_vars' = num_cons - 1, num_io' = 0 - its z
 * has exactly num_cons entries - and, for each of A, B, C, M'[j][i] = M[i][j]: row j lists its entries by ascending i, entries of
 * equal (i, j) in their input order, rows j >= ncols are empty.  Read back (lurk_hip_r1cs_read) it is bit for bit what a stable sort of
 * the host CSR by column followed by lurk_hip_r1cs_create gives, on every run: nothing depends on the order in which atomics land.
 * The coefficient dictionary is the source's (one device-to-device copy), so lurk_hip_r1cs_info reports the source's nnz per matrix
 * and distinct_coefficients; the rows the wave-per-row kernels take (more than 32 entries in A, B or C) are found again.  multiply_vec,
 * is_sat, sparse_mle, the provers and lurk_hip_r1cs_destroy take the result as any shape.
 * The work is ordered after `stream`, which the call synchronises ONCE, at its end (the host keeps the number of long rows): the
 * result is complete when the call returns.  The source is only read: calls on one source from several threads are independent.
 * Temporary memory comes from the stream's scratch arena (lurk_hip_scratch_trim releases it): 16 B per non-zero of the largest of the
 * three matrices - twice that matrix's resident entry array - plus the sort's own storage (histograms and look-back state, a few per
 * cent of the entry array) and 8 B per 256 rows of the result.
 * Refused with LURK_HIP_ERR_INVALID_ARG before anything is allocated or launched, *out = NULL: a NULL shape or out, num_cons = 0,
 * rows_t non-zero and below ncols, rows_t >= 2^32, a source that is not resident on the calling thread's current device, a source over
 * LURK_FIELD_BN254_FQ (nothing downstream of a transpose is offered over that field).  An
 * allocation that fails returns LURK_HIP_ERR_OOM and leaves nothing behind. */
int lurk_hip_r1cs_transpose_dev(const lurk_hip_r1cs* shape, size_t rows_t, lurk_hip_r1cs** out, void* stream);
/* Matrix `which` (0 = A, 1 = B, 2 = C) of a resident shape as the CSR lurk_hip_r1cs_create takes: indptr num_cons + 1 entries, indices
 * and data32_mont nnz entries (sizes from lurk_hip_r1cs_dims / lurk_hip_r1cs_info), data 32 B Montgomery.  data32_mont may be NULL to
 * read the structure only; indices and data32_mont may both be NULL when nnz = 0.  A host call: it synchronises the device.  The shape
 * must be resident on the calling thread's current device; an unknown `which` is refused by name.  For cross-checking a host's own
 * shape against one the library built (lurk_hip_frames_r1cs_create) or transposed. */
int lurk_hip_r1cs_read(const lurk_hip_r1cs* shape, int which, uint64_t* indptr, uint64_t* indices, void* data32_mont);
/* R1CSShape::multiply_vec: (A z, B z, C z); d_z has num_vars + 1 + num_io elements, outputs num_cons */
int lurk_hip_r1cs_multiply_vec_dev(const lurk_hip_r1cs* shape, const void* d_z, void* d_az, void* d_bz,
                                   void* d_cz, void* stream);
/* R1CSShape::commit_T's vector: T = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - u2 CZ1 (u_i = z_i[num_vars]) */
int lurk_hip_r1cs_cross_term_dev(lurk_hip_r1cs* shape, const void* d_z1, const void* d_z2, void* d_t,
                                 void* stream);
/* The same vector with the running instance's products CACHED (round 6): A z1, B z1, C z1 fold linearly with the running pair
 * (A (z1 + r z2) = A z1 + r A z2), so a prover that keeps them resident gathers from z2 alone - half the gather chains of the call
 * above.  u1_32_mont: the running u (32 bytes, HOST memory: the caller folds scalars itself, u <- u + r u2).  Outputs T and (A z2,
 * B z2, C z2).  The fold of the cache rides in the call: given the PREVIOUS step's products d_*z2_prev and its challenge r_prev32_mont
 * (host; all four NULL = nothing to fold in), every cached row becomes row + r_prev * previous row - stored back in place - before it
 * is used, so that nothing stands between a step's transcript and the next cross term (two buffers: the previous products are read
 * while the new ones are written).  A folding context does all of this itself (lurk_hip_fold_step_*; LURK_FOLD_CACHED_PRODUCTS=0
 * keeps it on the call above). */
int lurk_hip_r1cs_cross_term_cached_dev(lurk_hip_r1cs* shape, const void* d_z2, void* d_az1, void* d_bz1, void* d_cz1, const void* u1_32_mont,
                                        const void* d_az2_prev, const void* d_bz2_prev, const void* d_cz2_prev, const void* r_prev32_mont, void* d_t,
                                        void* d_az2, void* d_bz2, void* d_cz2, void* stream);
/* R1CSShape::is_sat / is_sat_relaxed on the device: A z o B z == u * C z + E row by row, u = z[num_vars]; d_e == NULL means E = 0 (plain
 * is_sat when u = 1).  n_unsat: rows that fail; first_unsat: the lowest failing row index (num_cons when none).  Host outputs; the call
 * synchronises `stream`.  The three inner products of a row are formed and compared canonically in one pass - nothing is written per
 * row, so a host no longer pulls 3 x num_cons x 32 B of lurk_hip_r1cs_multiply_vec_dev's output back to check an instance.  Rows are
 * classed by length once per shape, on the first call (one lane per short row, a sub-wave group per mid-length row, 16 lanes per long
 * row); checks of ONE shape run one after the other.  The shape must be resident on the calling thread's current device (d_z and d_e
 * are that device's pointers): otherwise the call is refused with nothing launched. */
int lurk_hip_r1cs_is_sat_dev(const lurk_hip_r1cs* shape, const void* d_z, const void* d_e, uint64_t* n_unsat, uint64_t* first_unsat,
                             void* stream);
/* RelaxedR1CSWitness::fold: out = a + r b over n elements (W1 + r W2, E1 + r T); r: 32 B Montgomery, host */
int lurk_hip_fold_vec_dev(int field_id, const void* d_a, const void* d_b, const void* r32_mont, size_t n,
                          void* d_out, void* stream);
/* count (<= 8) such folds under one r in ONE launch: d_a / d_b / d_out / n are host arrays of count device pointers / lengths
 * (out_k may be a_k: the fold is elementwise) - the step's finish(r) folds [W | u | X], E and the three cached products this way. */
int lurk_hip_fold_vecs_dev(int field_id, int count, const void* const* d_a, const void* const* d_b, const size_t* n, void* const* d_out,
                           const void* r32_mont, void* stream);
/* host-pointer forms of the three calls above (copy in, run, copy out): small inputs and tests */
int lurk_hip_r1cs_multiply_vec(const lurk_hip_r1cs* shape, const void* z, void* az, void* bz, void* cz);
int lurk_hip_r1cs_cross_term(lurk_hip_r1cs* shape, const void* z1, const void* z2, void* t);
int lurk_hip_fold_vec(int field_id, const void* a, const void* b, const void* r32_mont, size_t n, void* out);
/* A linear combination of up to 128 vectors of DIFFERENT lengths, each read as if zero-padded to n_out, in ONE launch:
 *     d_out[j] = sum_k c_k (j < lens[k] ? d_vecs[k][j] : 0),   j < n_out
 * - the joint polynomial W + gamma E (or sum_k gamma^k P_k over a batch) that the BN254 compressing provers open, without the padded
 * copies: every input is read once, the output written once, nothing is cleared first.  d_vecs / lens: host arrays of `count` device
 * pointers / element counts (the shape of lurk_hip_sumcheck_prove_dev's d_polys); coeffs: count x 32 B Montgomery, host.  Refused:
 * count = 0, a NULL vector with a non-zero length (a zero-length vector may be NULL), lens[k] > n_out, d_out overlapping an input.
 * The call synchronises the stream once (its table of pointers is staged from the caller's memory). */
int lurk_hip_fold_padded_dev(int field_id, int count, const void* const* d_vecs, const size_t* lens, const void* coeffs32_mont, size_t n_out,
                             void* d_out, void* stream);

/* ---- one folding step on one curve of the cycle ----------------------------------------------
 * What RecursiveSNARK::prove_step (/root/reference/src/proof/nova.rs:282-295, SuperNova /root/reference/src/proof/
 * supernova.rs:231-244) runs per curve through arecibo's NIFS::prove, with the running pair (z1 = [W1 | u1 | X1], E1)
 * resident in HBM from step to step.  A prover holds one context per curve: Pallas (primary, the Lurk step circuit) and
 * Vesta (secondary), or on lurk-beta's default cycle BN254 (primary) and Grumpkin (secondary, over a shape from
 * lurk_hip_r1cs_create_for_curve).  On the BN254 cycle the caller derives r itself: lurk_hip_fold_step, _set_pp_digest and
 * _challenge refuse both curves by name and leave an open step usable.  shape and key are borrowed (same curve / scalar field, created on the same device) and must outlive
 * the context; the context uses the key's async slots (W2: 0 and 2 alternately, T: 1, late ranges: 3).  The challenge r is a
 * Poseidon sponge over the OTHER field of the cycle absorbing the two commitments `begin` returns, hence two halves (a caller
 * with its own transcript uses them; lurk_hip_fold_step below runs begin, the library's own transcript and finish in one call):
 *   begin:  comm_W2 = commit(W2); T = cross term of (z1, [W2 | 1 | X2]); comm_T = commit(T)   - commitments in flight
 *   finish: W <- W1 + r W2, u <- u1 + r, X <- X1 + r X2, E <- E1 + r T                         - stream-ordered, no sync
 * The public IO X2 of a Lurk step is Store::to_scalar_vector's [tag, hash] x 3 (/root/reference/src/lem/store.rs:883-895,
 * Z1) in Montgomery form.  A new context holds the default (all-zero) relaxed pair, as RecursiveSNARK::new starts from. */
typedef struct lurk_hip_fold_ctx lurk_hip_fold_ctx;
int lurk_hip_fold_ctx_create(lurk_hip_fold_ctx** ctx, int curve, lurk_hip_r1cs* shape, lurk_hip_msm_ctx* key);
/* The same context over a key cut across several devices (lurk_hip_msm_multi_create; the north star's "witness-commitment batches
 * shard across the GPUs of one node"): the cross term and the folds run on the shape's device, each commitment pushes slice i of
 * its vector peer-to-peer into device i, the slices commit concurrently and the 96-byte partials are summed on the host.  begin /
 * finish / lurk_hip_fold_step as above; staging ahead (prefetch) is not offered with a multi-device key. */
int lurk_hip_fold_ctx_create_multi(lurk_hip_fold_ctx** ctx, int curve, lurk_hip_r1cs* shape, lurk_hip_msm_multi* key);
int lurk_hip_fold_ctx_destroy(lurk_hip_fold_ctx* ctx);
/* running pair <- host values (Montgomery): z1 (num_vars + 1 + num_io elements), E1 (num_cons elements) */
int lurk_hip_fold_ctx_set_running(lurk_hip_fold_ctx* ctx, const void* z1, const void* e1);
/* w2: num_vars x 32 B Montgomery, host memory or (w2_on_device) device memory produced on w2_stream (NULL = default
 * stream); x2_mont: num_io x 32 B, host */
int lurk_hip_fold_step_begin(lurk_hip_fold_ctx* ctx, const void* w2, int w2_on_device, void* w2_stream, const void* x2_mont,
                             void* comm_w2_jacobian96, void* comm_t_jacobian96);
/* Staging ahead (MI355X-side pipelining of nova.rs:282-326, where the witness of step i+1 is synthesized by a producer thread
 * while step i folds): the commitment to W2 needs no running instance, so it can run under the previous step's commit(T).
 *   prefetch(range)  stages positions [offset, offset + count) of the NEXT fresh witness (the rest zero for now) and starts
 *                    its commitment; at most two instances may be staged;
 *   begin_prefetched consumes the oldest staged instance: `patches` are the ranges known only now (the augmented circuit's
 *                    own variables around the step circuit's: they depend on the previous step's fold), host memory,
 *                    Montgomery; commit is linear, so comm_W2 = commit(staged ranges) + commit(late ranges).
 * The context uses the key's four async slots (lurk_hip_msm_ctx_reserve(key, n, 4)): W2 commitments alternate between slots 0
 * and 2, T uses slot 1, the late ranges slot 3 - or, up to 2^16 late positions, a small-commitment key of their own: the key's points
 * at those positions, built at the first begin that brings late ranges and kept while their layout stays the same (one launch per
 * step instead of a pass over a num_vars-long vector; LURK_FOLD_LATE_KEY=0 in the environment keeps slot 3).
 * lurk_hip_fold_step_begin is prefetch(whole W2) + begin_prefetched(no patches). */
typedef struct lurk_hip_w2_patch {
    size_t offset, count;   /* positions [offset, offset + count) of W2 */
    const void* values;     /* count x 32 bytes, host memory */
} lurk_hip_w2_patch;
int lurk_hip_fold_step_prefetch(lurk_hip_fold_ctx* ctx, const void* w2_range, size_t offset, size_t count, int on_device, void* stream);
/* Staging ahead ACROSS DEVICES: helper_key is the same commitment key resident on another device (an ordinary lurk_hip_msm_ctx over
 * the same bases, created under lurk_hip_set_device(other)).  Instances staged with lurk_hip_fold_step_prefetch then have their
 * commitment computed on the helpers in turn - the staged ranges are pushed peer-to-peer - while the context's own device folds the
 * open step; late ranges and T stay on the context's device.  Folding steps are sequential, so this (the reference's witness producer
 * thread, /root/reference/src/proof/nova.rs:306-317, spread over GPUs) is how IVC itself gains from several devices.  Add helpers
 * before the first step; they are borrowed for the context's lifetime and use their slots 0 and 2. */
int lurk_hip_fold_ctx_add_helper(lurk_hip_fold_ctx* ctx, lurk_hip_msm_ctx* helper_key);
int lurk_hip_fold_step_begin_prefetched(lurk_hip_fold_ctx* ctx, const lurk_hip_w2_patch* patches, size_t n_patches, const void* x2_mont,
                                        void* comm_w2_jac96, void* comm_t_jac96);
int lurk_hip_fold_step_finish(lurk_hip_fold_ctx* ctx, const void* r32_mont);
/* The challenge of the OPEN step from the library's transcript, for callers of the begin / finish halves who do not bring their own:
 * set the digest of the public parameters once; every begin then absorbs pp_digest and the running instance U1 - and runs the
 * permutation that completes - while the device is still working on the step, absorbs U2 when comm_W2 has arrived, and
 * lurk_hip_fold_step_challenge finishes behind comm_T with ONE permutation: r = RO(pp_digest, U1, U2, comm_T), the value
 * lurk_hip_nifs_challenge gives (and lurk_hip_fold_step uses the same staging).  r comes back in Montgomery form, ready for finish. */
int lurk_hip_fold_ctx_set_pp_digest(lurk_hip_fold_ctx* ctx, const void* pp_digest32);
int lurk_hip_fold_step_challenge(lurk_hip_fold_ctx* ctx, void* r32_mont);
/* A hook into the open step, for the caller's own device work that should run BESIDE the step - the slot traces of the next witness
 * (lurk_hip_slot_witness_dev), what the reference's witness-producer thread does while prove_step folds
 * (/root/reference/src/proof/nova.rs:304-326).  begin / begin_prefetched / lurk_hip_fold_step call hook(user) ONCE per step, on the
 * calling thread, after the step's device work (cross term, both commitments) has been enqueued and before they block on the
 * commitments.  Work enqueued from the hook queues behind the step's opening kernels and fills what the commitments leave (their
 * sorts and bucket reductions); enqueued before begin it would run first and hold the cross term back, enqueued after begin has
 * returned it runs alone: 3.50-3.59 ms per step at rc = 100 against 4.22 and 3.85 (profiles/r04_step_witness_placement.txt).
 * Of this context's own functions the hook may call lurk_hip_fold_step_prefetch only (the next instance is then staged AND its
 * commitment started in the background class, beside the open step's commit(T)); a non-zero return fails the begin (the step is rolled
 * back).  NULL removes it. */
typedef int (*lurk_hip_fold_submit_hook_fn)(void* user);
int lurk_hip_fold_ctx_set_submit_hook(lurk_hip_fold_ctx* ctx, lurk_hip_fold_submit_hook_fn hook, void* user);
/* the running pair where it lives (valid until the next finish) and the stream its updates are ordered on */
int lurk_hip_fold_ctx_running_dev(lurk_hip_fold_ctx* ctx, void** d_z, void** d_e, void** stream);
/* copies of the running pair for the host (either may be NULL); synchronises the context's stream */
int lurk_hip_fold_ctx_read(lurk_hip_fold_ctx* ctx, void* z_host, void* e_host);
/* The running INSTANCE U = (comm_W, comm_E, u, X) lives in the context beside the running witness: finish(r) folds it on the host
 * as RelaxedR1CSInstance::fold does (comm_W1 + r comm_W2, comm_E1 + r comm_T, u1 + r, X1 + r X2) while the device folds the
 * vectors.  set_instance installs the two commitments of a running pair given with set_running (u and X are taken from its z1);
 * instance reads the four parts back (96-byte Jacobians, Montgomery scalars; any pointer may be NULL). */
int lurk_hip_fold_ctx_set_instance(lurk_hip_fold_ctx* ctx, const void* comm_w_jacobian96, const void* comm_e_jacobian96);
int lurk_hip_fold_ctx_instance(lurk_hip_fold_ctx* ctx, void* comm_w_jacobian96, void* comm_e_jacobian96, void* u32_mont, void* x_mont);
/* NIFS::prove whole (/root/reference/src/proof/nova.rs:291-293 -> arecibo nifs.rs): begin, the challenge
 * r = RO(pp_digest, U1, U2, comm_T) derived in the library (lurk_hip_nifs_challenge below), finish(r).  pp_digest32: the
 * public parameters' digest, a canonical scalar (32 B).  Outputs (any may be NULL): the step's two commitments and r (Montgomery). */
int lurk_hip_fold_step(lurk_hip_fold_ctx* ctx, const void* w2, int w2_on_device, void* w2_stream, const void* x2_mont,
                       const void* pp_digest32, void* comm_w2_jacobian96, void* comm_t_jacobian96, void* r32_mont);

/* ---- the transcript: Nova's random oracle (host code, no device needed; restated [MEM], parity unpinned) ------------------
 * arecibo PoseidonRO over neptune's sponge API (simplex, arity 24, standard strength):
 *   nova_ro_squeeze     absorbs n canonical elements of `field_id` (32 B each), squeezes one element and returns the integer of
 *                       its low num_bits bits (32 B little-endian) - PoseidonRO::{absorb, squeeze};
 *   nova_ro_pattern_tag neptune IOPattern([Absorb(a), Squeeze(s)]).value(domain_separator): the sponge's capacity element (16 B);
 *   nifs_challenge      the absorb list of NIFS::prove on `curve`: pp_digest, U1 = (comm_W1, comm_E1, u1, X1 as 4 x 64-bit limbs
 *                       each), U2 = (comm_W2, X2), comm_T - commitments as (x, y, is_infinity), scalars through scalar_as_base -
 *                       then r = squeeze(NUM_CHALLENGE_BITS = 128) in Montgomery form of the curve's scalar field. */
/* Run-time parameters of the restatement above (round 6).  arecibo and neptune are un-vendored dependencies of the reference
 * (/root/reference/Cargo.toml:127-128) and /root/reference holds no transcript value, so every constant of the sponge and of the
 * absorb list that was recalled from memory is a FIELD here instead of a compiled-in literal: the first Rust-side run that gets
 * another r than arecibo's NIFS::prove (caller: /root/reference/src/proof/nova.rs:282-295) can move one field at a time - or hand a
 * LURKDUMP probe record (lurk_beta_amd/dump.py, rust/lurk-hip-sys/src/dump.rs) to `python -m lurk_beta_amd.dump probe FILE`, which
 * searches them - with no rebuild.  Process-wide; set(NULL) restores the defaults (the values of rounds 1-5, in brackets); a folding
 * context reads them when a step's transcript begins.  nova_ro_squeeze / nova_ro_pattern_tag use arity, domain_separator (squeeze
 * only), absorb_tag_bit, pattern_absorbs and squeeze_element; nifs_challenge and the folding contexts use all of them. */
#define LURK_RO_ITEM_PP_DIGEST 0
#define LURK_RO_ITEM_U1 1
#define LURK_RO_ITEM_U2 2
#define LURK_RO_ITEM_COMM_T 3
#define LURK_RO_PART_COMM_W 0
#define LURK_RO_PART_COMM_E 1
#define LURK_RO_PART_U 2
#define LURK_RO_PART_X 3
typedef struct lurk_hip_ro_params {
    uint32_t struct_size;        /* sizeof(lurk_hip_ro_params): get() fills it, set() checks it */
    uint32_t arity;              /* rate of the sponge = neptune arity, width arity + 1 [24] */
    uint32_t domain_separator;   /* IOPattern::value(domain_separator) [0] */
    uint32_t absorb_tag_bit;     /* SpongeOp::Absorb(n).value() = n + 2^absorb_tag_bit [31] */
    uint32_t num_challenge_bits; /* NUM_CHALLENGE_BITS: low bits of the squeezed element kept as r [128] */
    uint32_t item_order[4];      /* NIFS::prove absorbs LURK_RO_ITEM_* in this order [pp_digest, U1, U2, comm_T] */
    uint32_t relaxed_order[4];   /* RelaxedR1CSInstance::absorb_in_ro: LURK_RO_PART_* in this order [comm_W, comm_E, u, X] */
    uint32_t fresh_order[2];     /* R1CSInstance::absorb_in_ro: 0 = comm_W, 1 = X [comm_W, X] */
    uint32_t point_elements;     /* a commitment is (x, y, is_infinity) = 3 elements, or (x, y) = 2 [3] */
    uint32_t relaxed_x_limbs;    /* every X_i of a relaxed instance as this many limbs (BN_N_LIMBS); 0 = one element through scalar_as_base [4] */
    uint32_t fresh_x_limbs;      /* the same for a fresh instance [0] */
    uint32_t limb_bits;          /* BN_LIMB_WIDTH [64] */
    uint32_t pattern_absorbs;    /* 0 = the IO pattern declares the number of elements really absorbed; else this constant (NUM_FE_FOR_RO) [0] */
    uint32_t squeeze_element;    /* which rate element squeeze reads [0] */
} lurk_hip_ro_params;
int lurk_hip_ro_params_get(lurk_hip_ro_params* out);
int lurk_hip_ro_params_set(const lurk_hip_ro_params* params);
/* Diagnostic twin of nifs_challenge: the elements it absorbs, in order, canonical 32-byte integers of the RO's field (the other
 * field of the cycle) - what a probe record's `absorbed` list is compared with, element by element.  *count = the number of
 * elements; out_elems32 (cap elements) may be NULL to ask for the count only. */
int lurk_hip_nifs_absorb_list(int curve, const void* pp_digest32, const void* comm_w1_jacobian96, const void* comm_e1_jacobian96,
                              const void* u1_mont, const void* x1_mont, const void* comm_w2_jacobian96, const void* x2_mont, size_t num_io,
                              const void* comm_t_jacobian96, void* out_elems32, size_t cap, size_t* count);
int lurk_hip_nova_ro_squeeze(int field_id, const void* elems32, size_t n, unsigned num_bits, void* out32);
int lurk_hip_nova_ro_pattern_tag(uint32_t absorbs, uint32_t squeezes, uint32_t domain_separator, void* out16);
int lurk_hip_nifs_challenge(int curve, const void* pp_digest32, const void* comm_w1_jacobian96, const void* comm_e1_jacobian96,
                            const void* u1_mont, const void* x1_mont, const void* comm_w2_jacobian96, const void* x2_mont, size_t num_io,
                            const void* comm_t_jacobian96, void* r32_mont);

/* ---- arecibo's Keccak256Transcript (host code; no device needed) --------------------------------------------------------------
 * The transcript RelaxedR1CSSNARK / BatchedRelaxedR1CSSNARK run behind CompressedSNARK::prove (/root/reference/src/proof/nova.rs:92,
 * 341-356; supernova.rs:110, 293-302): persona tag "NoTR", domain-separator tag "NoDS", a 64-byte state, a u16 round counter and a
 * running Keccak-256 hasher; a challenge is Scalar::from_uniform of 64 squeezed bytes.  Restated from arecibo's published source
 * and UNPINNED (arecibo is an un-vendored dependency, /root/reference/Cargo.toml:128); Keccak-256 itself is pinned by known answers.
 * absorb_scalars takes canonical little-endian 32-byte elements and absorbs their to_transcript_bytes (the repr reversed);
 * absorb_point takes a 96-byte Jacobian and absorbs x || y || [finite] of its affine form. */
typedef struct lurk_hip_keccak_transcript lurk_hip_keccak_transcript;
int lurk_hip_keccak256(const void* in, size_t len, void* out32);
int lurk_hip_keccak_transcript_new(lurk_hip_keccak_transcript** t, const void* label, size_t label_len);
int lurk_hip_keccak_transcript_destroy(lurk_hip_keccak_transcript* t);
int lurk_hip_keccak_transcript_absorb(lurk_hip_keccak_transcript* t, const void* label, size_t label_len, const void* bytes, size_t len);
int lurk_hip_keccak_transcript_absorb_scalars(lurk_hip_keccak_transcript* t, const void* label, size_t label_len,
                                              const void* scalars32_canonical, size_t n);
int lurk_hip_keccak_transcript_absorb_point(lurk_hip_keccak_transcript* t, const void* label, size_t label_len, int curve,
                                            const void* point_jacobian96);
int lurk_hip_keccak_transcript_dom_sep(lurk_hip_keccak_transcript* t, const void* bytes, size_t len);
int lurk_hip_keccak_transcript_squeeze(lurk_hip_keccak_transcript* t, const void* label, size_t label_len, int field_id,
                                       void* out32_canonical);
/* Ready-made `challenge` arguments for the round loops below (lurk_hip_sumcheck_prove_dev / _prove_batch_dev, lurk_hip_ipa_prove_dev)
 * over a Keccak transcript, so that a proof's rounds run without leaving the library: pass the function as `challenge` and a
 * lurk_hip_keccak_round_binding as `user`.  Sum-check: the round polynomial's n_scalars coefficients are absorbed under absorb_label,
 * the challenge is squeezed under squeeze_label.  Inner-product argument: L under absorb_label, R under absorb_label2 (points of
 * `curve`), then the squeeze.  Every challenge is also appended to challenges_out (32 canonical bytes each; NULL = not kept), n_rounds
 * counts the calls. */
typedef struct lurk_hip_keccak_round_binding {
    lurk_hip_keccak_transcript* transcript;
    int field_id, n_scalars, curve;
    const void* absorb_label;
    size_t absorb_label_len;
    const void* absorb_label2;
    size_t absorb_label2_len;
    const void* squeeze_label;
    size_t squeeze_label_len;
    void* challenges_out;
    size_t challenges_cap, n_rounds; /* capacity of challenges_out in challenges; calls so far */
} lurk_hip_keccak_round_binding;
int lurk_hip_keccak_sumcheck_challenge(void* binding, int round, const void* coefficients32_canonical, void* out_r32_canonical);
int lurk_hip_keccak_ipa_challenge(void* binding, int round, const void* l_jacobian96, const void* r_jacobian96, void* out_r32_canonical);

/* ---- sum-check rounds (the data-parallel half of CompressedSNARK::prove) -----------------------
 * CompressedSNARK::prove (/root/reference/src/proof/nova.rs:341-356, supernova.rs:293-302) -> arecibo RelaxedR1CSSNARK::prove ->
 * SumcheckProof::prove_cubic_with_additive_term (outer: eq(tau) (Az Bz - (u Cz + E))) and prove_quad (inner: poly_ABC z).
 * The tables (Montgomery, len = 2^k elements each, device memory) stay in HBM, the transcript stays on the host.  One call is
 * one round: if bind_r32_mont != NULL every table's top variable is first bound to it in place (P[i] += r (P[len/2 + i] - P[i]),
 * the table is len / 2 long afterwards); then, if evals_out != NULL, the evaluations of the next round polynomial over the
 * current tables are summed and written to HOST memory (the call synchronises the stream for them):
 *   degree 3: d_polys = {A, B, C, D}, evals_out = [e(0), e(2), e(3)] of sum_i A (B C - D)     (3 x 32 B)
 *   degree 2: d_polys = {A, B},       evals_out = [e(0), e(2)]       of sum_i A B             (2 x 32 B)
 * A prover calls it with (NULL, evals) for the first round, (r_j, evals) in between and (r_last, NULL) at the end, after which
 * P[0] of every table is its evaluation at the challenge point.  (A whole sum-check is cheaper through lurk_hip_sumcheck_prove_dev /
 * _prove_batch_dev below: they keep the rounds' scratch - workgroup partial sums, ticket counter, the pinned words the totals land in -
 * for the whole proof, this entry point sets it up per call.) */
int lurk_hip_sumcheck_round_dev(int field_id, int degree, void* const* d_polys, size_t len, const void* bind_r32_mont,
                                void* evals_out, void* stream);
/* EqPolynomial::evals: d_out[b] = prod_j (b_j ? r_j : 1 - r_j), r_0 <-> the most significant bit of b; r: ell x 32 B Montgomery, host */
/* A whole sum-check (SumcheckProof::prove_quad / prove_cubic_with_additive_term of arecibo's Spartan, behind
 * /root/reference/src/proof/nova.rs:341-356) with the tables resident: log2(len) rounds of lurk_hip_sumcheck_round_dev, the round
 * polynomial interpolated on the host, the transcript behind a callback: `challenge` receives the round and the polynomial's
 * degree + 1 canonical coefficients (low to high) and writes r as a canonical 32-byte value (return 0; anything else aborts the call).
 * The tables are consumed: their contents are UNSPECIFIED after the call (the first rounds bind them in place; once they are down to
 * 2^LURK_SUMCHECK_HOST_TAIL_LOG elements the remaining rounds run on a host copy, so d_polys[k][0] is NOT the final evaluation) -
 * out_finals is the only place the final evaluations are returned.  Outputs, all canonical: the round polynomials (rounds x (degree + 1) x 32 bytes), the
 * tables' final evaluations (2 or 4 x 32 bytes) and the final claim. */
typedef int (*lurk_hip_sumcheck_challenge_fn)(void* user, int round, const void* coefficients32_canonical, void* out_r32_canonical);
int lurk_hip_sumcheck_prove_dev(int field_id, int degree, void* const* d_polys, size_t len, const void* claim32_canonical,
                                lurk_hip_sumcheck_challenge_fn challenge, void* user, void* out_polys, void* out_finals,
                                void* out_claim32, void* stream);
/* Batched form: sum_i coeff_i * sum_x comb(tables of instance i) with ONE challenge per round shared by all instances - the
 * evaluation-claim batching of arecibo's RelaxedR1CSSNARK and the outer / inner sum-checks of its BatchedRelaxedR1CSSNARK (SuperNova's
 * compressor, /root/reference/src/proof/supernova.rs:110, 293-302).  d_polys: n_instances x (4 or 2) device tables, instance-major, all
 * of length len (shorter instances zero-padded by the caller); coeffs32_canonical: n_instances batching coefficients; claim: the
 * COMBINED claim sum_i coeff_i claim_i.  out_finals: n_instances x (4 or 2) x 32 B, the tables' final evaluations, instance-major. */
int lurk_hip_sumcheck_prove_batch_dev(int field_id, int degree, size_t n_instances, void* const* d_polys, size_t len,
                                      const void* coeffs32_canonical, const void* claim32_canonical,
                                      lurk_hip_sumcheck_challenge_fn challenge, void* user, void* out_polys, void* out_finals,
                                      void* out_claim32, void* stream);
int lurk_hip_eq_evals_dev(int field_id, const void* r32_mont, int ell, void* d_out, void* stream);

/* ---- inner-product argument rounds (the opening half of CompressedSNARK::prove) ------------------
 * EE1 / EE2 = ipa_pc::EvaluationEngine on the Pasta cycle (/root/reference/src/proof/nova.rs:57-62).  Per round of the published
 * argument, with the vectors a, b and the (folded) key resident in HBM: the two cross inner products, the two commitments
 * L, R (lurk_hip_msm_ctx_create_dev / run_dev over the halves of the device key), then with the transcript's challenge r the
 * folds a' = r a_L + r^-1 a_R, b' = r^-1 b_L + r b_R (fold_halves, in place: the vector is len / 2 long afterwards) and
 * ck' = [r^-1] ck_L + [r] ck_R (points_fold_halves: len / 2 affine points out; may not alias the input). */
int lurk_hip_inner_product_dev(int field_id, const void* d_a, const void* d_b, size_t n, void* out32_mont, void* stream);
int lurk_hip_fold_halves_dev(int field_id, void* d_v, size_t len, const void* s_lo32_mont, const void* s_hi32_mont, void* stream);
int lurk_hip_points_fold_halves_dev(int curve, const void* d_points_affine64, size_t len, const void* s_lo32_mont,
                                    const void* s_hi32_mont, void* d_out_affine64, void* stream);

/* The same rounds WITHOUT folding the key (the form lurk_beta_amd/ipa.py uses when the prover's resident table key is at hand):
 * the folded key of round k is a fixed linear image of the original one, ck_k[p] = sum_{i = p mod m} coef_k[i] ck[i] (m = the
 * current length, coef_k[i] = the product of the fold weights position i met so far), so L and R are ordinary commitments under
 * the ORIGINAL key of the two length-n vectors round_scalars writes (n/2 non-zeros each):
 *   out_l[i] = a[(i mod m) - m/2] coef[i] if (i mod m) >= m/2 else 0;  out_r[i] = a[(i mod m) + m/2] coef[i] if (i mod m) < m/2 else 0
 * and after the challenge coef_fold multiplies coef[i] by s_lo / s_hi according to the half (i mod m) lies in (coef starts as
 * all ones; after the last round it is the verifier's s vector: the final key element is commit(ck, coef)).  Two table-mode
 * MSMs per round replace m/2 full-size double scalar multiplications whose 255-step ladder is latency-bound for every m. */
/* (d_out_r == NULL: ONE merged vector in d_out_l - L's and R's supports are disjoint - for lurk_hip_msm_ctx_submit_pair_dev with
 *  sel_bit = log2(m / 2): out_hi = L, out_lo = R) */
int lurk_hip_ipa_round_scalars_dev(int field_id, const void* d_a, size_t m, const void* d_coef, size_t n, void* d_out_l,
                                   void* d_out_r, void* stream);
int lurk_hip_ipa_coef_fold_dev(int field_id, void* d_coef, size_t n, size_t m, const void* s_lo32_mont, const void* s_hi32_mont,
                               void* stream);
/* The whole inner-product argument under a resident key (arecibo ipa_pc::InnerProductArgument::prove, the opening of CompressedSNARK on
 * the Pasta cycle: /root/reference/src/proof/nova.rs:57-62, 341-356): log2(n) rounds of { composed scalars, commitment of L and R under
 * the ORIGINAL key, cross inner products, challenge, folds } with the vectors resident; the transcript is the caller's: `challenge`
 * receives the round number and L, R (96-byte Jacobians) and writes r as a canonical 32-byte value below the group order (return 0;
 * anything else aborts the call).  d_a, d_b: n Montgomery scalars on the device, consumed (folded in place); ck_c: the extra base,
 * already scaled by the transcript's first challenge.  Outputs: L and R per round (log2(n) x 96 bytes each), a_hat canonical, and the
 * folded key element as an affine Montgomery point ((0, 0) = identity).  n: a power of two, at most the key's points. */
/* The key folded by the weights of k rounds at once: d_out[p] = sum_{b < n_weights} weights[b] * key[b m + p], m = n / n_weights affine
 * Montgomery points on the device ((0, 0) = identity) - what k rounds of ck' = [r^-1] ck_L + [r] ck_R leave, the weights being the
 * products of the rounds' fold weights by block (arecibo ipa_pc.rs; /root/reference/src/proof/nova.rs:57-62).  The key must be in the
 * window-table form; weights: host memory, Montgomery, n_weights a power of two <= 2^12; n a multiple of it, at most the key's points.
 * lurk_hip_ipa_prove_dev does this by itself after its fourth round under a key of >= 2^18 points and continues under the folded key
 * (LURK_IPA_FOLD_MIN_LOG in the environment moves the threshold, 0 = never): 2^20 elements in 21 ms instead of 39. */
int lurk_hip_msm_ctx_fold_key_dev(lurk_hip_msm_ctx* key, size_t n, const void* weights32_mont, size_t n_weights, void* d_out_affine64,
                                  void* stream);
typedef int (*lurk_hip_ipa_challenge_fn)(void* user, int round, const void* l_jacobian96, const void* r_jacobian96, void* out_r32_canonical);
int lurk_hip_ipa_prove_dev(lurk_hip_msm_ctx* key, void* d_a32, void* d_b32, size_t n, const void* ck_c_jacobian96,
                           lurk_hip_ipa_challenge_fn challenge, void* user, void* out_l_jacobian96, void* out_r_jacobian96,
                           void* out_a_hat32, void* out_ck_hat_affine64, void* stream);

/* ---- HyperKZG: the opening argument of the BN254 cycle (EE1 of Bn256EngineKZG, /root/reference/src/proof/nova.rs:65-71) ---------------
 * The three polynomial primitives the argument is made of, over field ids 0, 1 and 2 (vectors of 32-byte Montgomery elements in device
 * memory; scalars Montgomery in HOST memory):
 *   mle_fold_pairs   d_out[j] = d_in[2j] + x (d_in[2j+1] - d_in[2j]) for j < ceil(len / 2): the LOWEST variable of a multilinear
 *                    polynomial's evaluation table is bound (lurk_hip_fold_halves_dev pairs i with len/2 + i: the highest).  An element
 *                    past the end reads as zero; d_out may not overlap d_in (refused).  len >= 1.  No synchronisation.
 *   poly_eval        out[k] = sum_j d_coeffs[j] points[k]^j for k < n_points <= 4, one pass over the coefficients (low to high); len = 0
 *                    gives zeros.  out32_mont: host memory; the call synchronises the stream for it.
 *   poly_div_linear  for every root u_k (n_roots <= 3, repeats allowed): d_quotients[k] (len - 1 coefficients on the device, may not
 *                    overlap d_coeffs) and remainders[k] (host) with  coeffs(X) = quotient_k(X) (X - u_k) + remainder_k,  one read of
 *                    the coefficients for all roots.  d_quotients: a host array of n_roots device pointers (ignored when len == 1).
 *                    len >= 1; the call synchronises the stream for the remainders. */
int lurk_hip_mle_fold_pairs_dev(int field_id, const void* d_in, size_t len, const void* x32_mont, void* d_out, void* stream);
int lurk_hip_poly_eval_dev(int field_id, const void* d_coeffs, size_t len, const void* points32_mont, int n_points, void* out32_mont, void* stream);
int lurk_hip_poly_div_linear_dev(int field_id, const void* d_coeffs, size_t len, const void* roots32_mont, int n_roots, void* const* d_quotients,
                                 void* remainders32_mont, void* stream);
/* The opening argument itself: this repository's own statement of the published HyperKZG scheme, recalled [MEM], NOT byte-compatible
 * with arecibo (tests/hyperkzg_ref.py restates it in Python integers).  key: a resident BN254 G1 key ck[0 .. N) - with a KZG SRS
 * ck[i] = [tau^i]G, so G = ck[0]; any other curve is refused by name.  d_poly: n = 2^ell Montgomery Fr values on the device (ell >= 1,
 * n <= N; not modified), the evaluations P_0 of a multilinear polynomial; x: ell Montgomery scalars on the host, x_0 <-> the most
 * significant index bit (the convention of lurk_hip_eq_evals_dev).
 *   P_{i+1}[j] = P_i[2j] + x_{ell-1-i} (P_i[2j+1] - P_i[2j]), i = 0 .. ell-2;  com_i = commit(P_i) under ck[0 .. len P_i), i = 1 .. ell-1;
 *   y = the same fold of P_{ell-1} with x_0;  r = challenge(0, com_1 .. com_{ell-1}), r = 0 is refused;  u = (r, -r, r^2);
 *   v[t][i] = P_i(u_t);  q = challenge(1, v);  B = sum_i q^i P_i (each P_i zero-padded to n);  h_t = (B - B(u_t)) / (X - u_t);
 *   W_t = commit(h_t).
 * The transcript is the caller's: `challenge` receives the stage, the stage's data (stage 0: count = ell - 1 Jacobians of 96 bytes;
 * stage 1: count = 3 ell canonical scalars, t-major) and writes the challenge as a canonical 32-byte value below the group order
 * (return 0; anything else aborts the call and leaves the key usable).  The verifier's third challenge d = challenge(2, W_0 .. W_2) is
 * not needed by the prover and is not asked for.  Outputs (host): out_com (ell - 1) x 96 B Jacobians (may be NULL when ell = 1), out_v
 * 3 ell x 32 B canonical (t-major), out_w 3 x 96 B, out_y 32 B canonical.  The call uses all LURK_MSM_SLOTS async slots of the key
 * (com_{i+1} accumulates while fold i + 1 runs; the three W_t are in flight together) and about 5 n x 32 B of the stream's scratch arena. */
typedef int (*lurk_hip_hyperkzg_challenge_fn)(void* user, int stage, const void* data, size_t count, void* out32_canonical);
int lurk_hip_hyperkzg_prove_dev(lurk_hip_msm_ctx* key, const void* d_poly32_mont, size_t n, const void* x32_mont,
                                lurk_hip_hyperkzg_challenge_fn challenge, void* user, void* out_com_jacobian96, void* out_v32, void* out_w_jacobian96,
                                void* out_y32, void* stream);
/* The verifier UP TO THE PAIRING (host code, no device needed; BN254 G1 only, any other curve is refused by name).  c = commit(P_0);
 * x (ell), y, v (3 ell, t-major), r, q, d: canonical scalars - r, q, d as the caller's transcript gives them, d = challenge(2, W);
 * com (ell - 1), w (3): 96-byte Jacobians.  Scalar checks, with Y_i = v[2][i] and Y_ell = y, for i = 0 .. ell-1:
 *     2 r Y_{i+1} = r (1 - x_{ell-1-i}) (v[0][i] + v[1][i]) + x_{ell-1-i} (v[0][i] - v[1][i])
 * then Bcom = sum_i q^i com_i (com_0 = c), b_t = sum_i q^i v[t][i], G = (1, 2) (= ck[0] of a powers-of-tau key) and
 *     L = sum_t d^t (Bcom - [b_t] G + [u_t] W_t),   R = sum_t d^t W_t.
 * The proof is valid iff e(L, H) = e(R, [tau] H): that pairing is the caller's (halo2curves, on the Rust side).  As with the verifiers
 * below the call succeeds whatever its answer: *accepted = 1 (accepted SO FAR: L and R are the pairing's inputs) or 0 with
 * *failed_check (may be NULL) = LURK_HYPERKZG_MALFORMED (a scalar not below the group order, r = 0, a point neither the identity nor
 * on the curve) or LURK_HYPERKZG_FOLD (one of the scalar checks); L and R are then the identity. */
#define LURK_HYPERKZG_ACCEPTED 0
#define LURK_HYPERKZG_MALFORMED 1
#define LURK_HYPERKZG_FOLD 2
int lurk_hip_hyperkzg_pairing_inputs(int curve, int ell, const void* c_jacobian96, const void* x32_canonical, const void* y32_canonical,
                                     const void* com_jacobian96, const void* v32_canonical, const void* w_jacobian96, const void* r32_canonical,
                                     const void* q32_canonical, const void* d32_canonical, void* out_l_jacobian96, void* out_r_jacobian96,
                                     int* accepted, int* failed_check);

/* ---- the BN254 pairing check: what lets the KZG verifiers DECIDE ------------------------------------------------------------------------
 * Host code, no device needed, and no kernel: one check is a 65-step Miller loop and one final exponentiation over twelve-limb towers,
 * a few milliseconds on one core, once per proof (lurk_beta_amd/csrc/bn254_pairing.hpp: the optimal ate pairing over the tower
 * Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - (9 + u)), Fq12 = Fq6[w]/(w^2 - v); tests/bn254_pairing_ref.py decides the same products by
 * another construction).  Only the DECISION crosses the ABI, never a GT element.
 *   G2 point: the sextic twist y^2 = x^3 + 3/(9 + u) over Fq2, affine, 128 bytes {x.c0, x.c1, y.c0, y.c1}, each 4 x u64 little-endian
 *   Montgomery (R = 2^256); all-zero is the identity.  This is halo2curves' G2Affine as recalled [MEM], unpinned like the G1 layouts.
 *   G1 point: the 96-byte Jacobian of every other entry point.
 * g2_mul: out = [k] P, P = the generator H of the order-r subgroup when g2_affine128 is NULL (so g2_mul(out, NULL, tau) is the verifier
 * key [tau]H of a trapdoor setup); k a canonical scalar.  Refused: a scalar not below r, a point off the twist (a point on the twist
 * outside the subgroup is multiplied as it is).
 * pairing_check: *product_is_one = (prod_{i < n} e(P_i, Q_i) == 1), one Miller accumulator for the n pairs and one final
 * exponentiation.  A pair with an identity on either side contributes 1; n = 0 gives 1.  Refused with LURK_HIP_ERR_INVALID_ARG, the
 * message naming the index and which: a G1 point neither the identity nor on the curve; a G2 point off the twist; a G2 point on the
 * twist but outside the order-r subgroup (the twist's cofactor is 2p - r: the curve equation alone does not put a point in G2; the test
 * is one 254-bit multiple per point, 1.4 ms). */
int lurk_hip_bn254_g2_mul(void* out_g2_affine128, const void* g2_affine128, const void* k32_canonical);
int lurk_hip_bn254_pairing_check(size_t n, const void* g1_jacobian96, const void* g2_affine128, int* product_is_one);
/* The HyperKZG verifier that decides: lurk_hip_hyperkzg_pairing_inputs (same arguments, same checks, same codes) and then
 * e(L, H) e(-R, tau_H) == 1 against the verifier key tau_H = [tau]H.  *accepted = 1: the proof is VALID.  *failed_check (may be NULL):
 * every failure the call above reports keeps its code; LURK_HYPERKZG_PAIRING when only the pairing equation fails; a tau_H that is off
 * the twist, outside the order-r subgroup or the identity gives LURK_HYPERKZG_MALFORMED whatever the proof.  tau_H is tested for
 * subgroup membership at every call (1.4 ms of the ~5 ms the pairing adds to a verification: DESIGN.md section 3.7.2); nothing is cached. */
#define LURK_HYPERKZG_PAIRING 3 /* lurk_hip_hyperkzg_verify only: e(L, H) e(-R, [tau]H) != 1 after every other check passed */
int lurk_hip_hyperkzg_verify(int curve, int ell, const void* c_jacobian96, const void* x32_canonical, const void* y32_canonical,
                             const void* com_jacobian96, const void* v32_canonical, const void* w_jacobian96, const void* r32_canonical,
                             const void* q32_canonical, const void* d32_canonical, const void* tau_h_g2_affine128, int* accepted,
                             int* failed_check);
/* Is a resident key a powers-of-tau key for THIS verifier key?  key: a resident BN254 G1 key of N points in any form (plain, window
 * table, small); Grumpkin and Pasta keys are refused by name.  *consistent = 1 iff ck[0] == (1, 2) - the G the verifiers assume - and
 * e(R, H) == e(L, tau_H) for
 *     rho_i = uniform(stream = seed, i), the scalars lurk_hip_synth_scalars_dev(LURK_FIELD_BN254_FR, seed, dist 0, ...) writes,
 *     L = sum_{i < N-1} rho_i ck[i],   R = sum_{i < N-1} rho_i ck[i+1]:
 * two commitments of ONE device buffer (0, rho_0 .. rho_{N-2}, 0) from its elements 1 and 0 through the key's ordinary commitment path -
 * no copy of the key, no kernel of its own.  N = 1 checks ck[0] only.  A key with any ck[j+1] != [tau] ck[j] passes with probability
 * 1/r over UNIFORM weights: the seed must be chosen AFTER the key exists (a key made knowing the seed can be made to pass), and
 * SplitMix64 is not a cryptographic generator - a caller that needs more than a file-integrity check draws its own weights.  A tau_H
 * that is off the twist, outside the subgroup or the identity is refused (LURK_HIP_ERR_INVALID_ARG, the message naming which).  The call
 * uses slots 0 and 1 of the key (they must be free), (N + 1) x 32 B of the stream's scratch arena, synchronises `stream`, and leaves the
 * key usable whatever happens. */
int lurk_hip_kzg_key_check_dev(lurk_hip_msm_ctx* key, const void* tau_h_g2_affine128, uint64_t seed, int* consistent, void* stream);

/* The single-instance compressing prover as ONE call (what CompressedSNARK::prove runs per curve: /root/reference/src/proof/nova.rs:341-356
 * -> arecibo RelaxedR1CSSNARK::prove): outer cubic sum-check, inner quadratic sum-check over the transposed shape, the two evaluation claims
 * batched to one point, one inner-product argument under the resident key - a sequence of the entry points above with the vectors resident
 * and the Keccak transcript inside.  The protocol is this repository's own (oracle/spartan_ref.py, oracle/spartan_fast.py: the oracle's
 * prover gives the same proof element for element, its verifier and lurk_hip_spartan_verify_dev below accept it), not arecibo's byte for byte.
 *   shape: num_cons x (num_vars + 1 + num_io) columns of z = [W | u | X]; shape_t: its transpose over 2 num_vars rows and num_cons columns
 *   (created with num_vars' = num_cons - 1, num_io' = 0); num_cons, num_vars: powers of two.  key: >= max(num_cons, num_vars) points, the
 *   key that committed W and E; ck_c: the inner-product base (a 96-byte Jacobian).  x, u: canonical; d_w (num_vars), d_e (num_cons):
 *   Montgomery, device memory, not modified.  label: the transcript's label.  Outputs (host memory, caller-sized, canonical):
 *   polys_outer log2(num_cons) x 4 x 32 B, claims_outer 3 x 32 (Az, Bz, Cz), eval_e 32, polys_inner (log2(num_vars) + 1) x 3 x 32,
 *   eval_w 32, polys_batch log2(N) x 3 x 32 (N = max(num_cons, num_vars)), evals_batch 2 x 32, ipa_l / ipa_r log2(N) x 96 (Jacobians),
 *   ipa_a 32. */
typedef struct lurk_hip_spartan_proof {
    void* polys_outer;
    void* claims_outer;
    void* eval_e;
    void* polys_inner;
    void* eval_w;
    void* polys_batch;
    void* evals_batch;
    void* ipa_l;
    void* ipa_r;
    void* ipa_a;
} lurk_hip_spartan_proof;
int lurk_hip_spartan_prove_dev(const lurk_hip_r1cs* shape, const lurk_hip_r1cs* shape_t, size_t num_cons, size_t num_vars, size_t num_io,
                               lurk_hip_msm_ctx* key, const void* ck_c_jacobian96, const void* x32_canonical, const void* u32_canonical,
                               const void* d_w32_mont, const void* d_e32_mont, const void* comm_w_jacobian96, const void* comm_e_jacobian96,
                               const void* label, size_t label_len, lurk_hip_spartan_proof* out, void* stream);

/* The BATCHED compressing prover as one call: n relaxed instances of different shapes and sizes under one key, one proof - the structure
 * of arecibo's spartan::batched::BatchedRelaxedR1CSSNARK, SuperNova's compressor (/root/reference/src/proof/supernova.rs:110, 293-302): one
 * outer and one inner sum-check shared through powers of a challenge, all 2 n evaluation claims batched to one point, one opening.  The
 * protocol is the repository's own (oracle/spartan_fast.py: prove_batched / verify_batched), as for the single-instance call.  Per
 * instance the arguments of lurk_hip_spartan_prove_dev.  With ell_x = log2(max num_cons), ell_y = log2(max num_vars) + 1,
 * N = max(num_cons, num_vars) over the instances, the outputs (host, canonical) are: polys_outer ell_x x 4 x 32 B, claims_outer
 * n x 3 x 32, evals_e n x 32, polys_inner ell_y x 3 x 32, evals_w n x 32, polys_batch log2(N) x 3 x 32, evals_batch 2 n x 32 (W_i, E_i
 * per instance), ipa_l / ipa_r log2(N) x 96 (Jacobians), ipa_a 32. */
typedef struct lurk_hip_spartan_instance {
    const lurk_hip_r1cs* shape;
    const lurk_hip_r1cs* shape_t;
    size_t num_cons, num_vars, num_io;
    const void* x32_canonical;
    const void* u32_canonical;
    const void* d_w32_mont;
    const void* d_e32_mont;
    const void* comm_w_jacobian96;
    const void* comm_e_jacobian96;
} lurk_hip_spartan_instance;
typedef struct lurk_hip_spartan_batch_proof {
    void* polys_outer;
    void* claims_outer;
    void* evals_e;
    void* polys_inner;
    void* evals_w;
    void* polys_batch;
    void* evals_batch;
    void* ipa_l;
    void* ipa_r;
    void* ipa_a;
} lurk_hip_spartan_batch_proof;
int lurk_hip_spartan_prove_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, lurk_hip_msm_ctx* key,
                                     const void* ck_c_jacobian96, const void* label, size_t label_len, lurk_hip_spartan_batch_proof* out,
                                     void* stream);

/* ---- the verifiers (the other half of the CompressedSNARK trait: /root/reference/src/proof/nova.rs:358-373, supernova.rs:304-316) ------
 * A verification is a SUCCESSFUL call whatever its answer: the return value says whether the call worked (bad arguments, no device,
 * out of memory -> non-zero with lurk_hip_last_error), *accepted = 1 / 0 is the answer and *failed_check (may be NULL) names the first
 * check that failed.  Malformed input is rejected before any arithmetic: a scalar of the proof or the statement that is not below the
 * field order, a point of the proof or a commitment that is neither the identity nor on the curve (or whose coordinates are not
 * reduced), an opening challenge that is zero. */
#define LURK_VERIFY_ACCEPTED 0
#define LURK_VERIFY_MALFORMED 1 /* input rejected before any arithmetic */
#define LURK_VERIFY_OUTER 2     /* outer sum-check: a round, or its final claim against claims_outer / eval_e */
#define LURK_VERIFY_INNER 3     /* inner sum-check: a round, or its final claim against the matrices at (r_x, r_y) and eval_w */
#define LURK_VERIFY_BATCH 4     /* the sum-check that batches the evaluation claims to one point */
#define LURK_VERIFY_OPENING 5   /* the inner-product argument's final point equation; the _kzg_ verifiers: HyperKZG's scalar checks */
#define LURK_VERIFY_PAIRING (6) /* the _kzg_verify_pairing verifiers only: e(L, H) e(-R, [tau]H) != 1 after every other check passed */
/* Building block: the sparse multilinear evaluation of a resident shape, M~ = sum_i eq_x[i] sum_{k in row i} val[k] eq_y[col[k]] for
 * M = A, B, C in ONE launch over the shape's non-empty rows (SparsePolynomial::evaluate of arecibo's Spartan verifier).  d_eq_x (n_x
 * elements), d_eq_y (n_y): Montgomery, device memory - whole eq tables or their leading parts (the batched verifier passes truncated
 * tables); n_x >= the shape's rows and n_y > its largest column, otherwise the call is refused.  out: three Montgomery elements
 * (A~, B~, C~) in HOST memory; the call synchronises the stream for them. */
int lurk_hip_r1cs_sparse_mle_dev(const lurk_hip_r1cs* shape, const void* d_eq_x, size_t n_x, const void* d_eq_y, size_t n_y,
                                 void* out_abc96_mont, void* stream);
/* Building block: the s vector of the inner-product argument's verifier, d_out[i] = prod_j (bit_{ell-1-j}(i) ? r_j : r_j^-1), 2^ell
 * Montgomery elements on the device (challenge 0 decides the highest index bit) - what ell rounds of lurk_hip_ipa_coef_fold_dev leave,
 * in one launch: one batched inversion on the host, two tables of 2^(ell/2) products, one product per element.  challenges: ell
 * canonical values of `field_id` in host memory, each non-zero and below the field order (refused otherwise); 0 <= ell <= 30. */
int lurk_hip_ipa_s_vector_dev(int field_id, const void* challenges32_canonical, int ell, void* d_out32_mont, void* stream);
/* SumcheckProof::verify (host only, no device needed): `rounds` round polynomials of degree + 1 canonical coefficients each (low to
 * high, as lurk_hip_sumcheck_prove_dev writes them), the challenge of every round (the caller replays its transcript).  Per round
 * p(0) + p(1) must equal the running claim, which becomes p(r).  *ok = 1 and the final claim in out_final32_canonical, or *ok = 0 (a
 * round failed, or a value was not reduced).  degree: 2 or 3. */
int lurk_hip_sumcheck_verify(int field_id, int degree, size_t rounds, const void* claim32_canonical, const void* polys,
                             const void* challenges32_canonical, void* out_final32_canonical, int* ok);
/* InnerProductArgument::verify under a resident key: with r_j = challenge(j, L_j, R_j) (the caller's transcript, as in
 * lurk_hip_ipa_prove_dev), s the vector above and b_hat = <s, b>, accepts iff
 *     P + sum_j (r_j^2 L_j + r_j^-2 R_j) == [a_hat] <s, key> + [a_hat b_hat] ck_c
 * P: the commitment to a plus [<a, b>] ck_c; ck_c: the extra base as the prover was given it (already scaled).  b: d_b32_mont (n
 * Montgomery scalars on the device, not modified) or, when that is NULL, eq(eq_point) for log2(n) canonical values on the host - b_hat
 * then has the closed form prod_j (r_j^-1 (1 - z_j) + r_j z_j) and no vector is read.  l, r: log2(n) x 96-byte Jacobians; a_hat
 * canonical.  n: a power of two, at most the key's points (a call error otherwise, not a rejection).  Device work: the s vector and ONE
 * commitment under the key; the 2 log2(n) + 2 scalar multiples of the equation run on the host. */
int lurk_hip_ipa_verify_dev(lurk_hip_msm_ctx* key, size_t n, const void* p_jacobian96, const void* ck_c_jacobian96, const void* d_b32_mont,
                            const void* eq_point32_canonical, const void* l_jacobian96, const void* r_jacobian96, const void* a_hat32,
                            lurk_hip_ipa_challenge_fn challenge, void* user, int* accepted, int* failed_check, void* stream);
/* CompressedSNARK::verify for one curve: the verifier of lurk_hip_spartan_prove_dev's proof (oracle/spartan_fast.py: verify, check for
 * check, over the same transcript).  The statement is (shape, X, u, comm_W, comm_E) under (key, ck_c, label); `proof` holds the prover's
 * outputs in the prover's layout (read only).  Device work: two eq tables, one sparse evaluation of the shape, the s vector, one
 * commitment under the key; everything else is a few hundred field operations and 2 log2(N) + 5 scalar multiples on the host.  Scratch
 * comes from the stream's arena; verifications on different streams are independent. */
int lurk_hip_spartan_verify_dev(const lurk_hip_r1cs* shape, size_t num_cons, size_t num_vars, size_t num_io, lurk_hip_msm_ctx* key,
                                const void* ck_c_jacobian96, const void* x32_canonical, const void* u32_canonical,
                                const void* comm_w_jacobian96, const void* comm_e_jacobian96, const void* label, size_t label_len,
                                const lurk_hip_spartan_proof* proof, int* accepted, int* failed_check, void* stream);
/* The verifier of lurk_hip_spartan_prove_batch_dev's proof (oracle/spartan_fast.py: verify_batched).  Of an instance it reads shape,
 * num_cons, num_vars, num_io, x, u and the two commitments; shape_t, d_w32_mont and d_e32_mont are ignored (a verifier has no witness
 * and needs no transpose). */
int lurk_hip_spartan_verify_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, lurk_hip_msm_ctx* key,
                                      const void* ck_c_jacobian96, const void* label, size_t label_len,
                                      const lurk_hip_spartan_batch_proof* proof, int* accepted, int* failed_check, void* stream);

/* ---- the compressing SNARK on BN254 G1: the same sum-checks, opened by HyperKZG -----------------------------------------------------
 * lurk-beta's default cycle is BN254 / Grumpkin, whose CompressedSNARK puts a HyperKZG evaluation engine under the Spartan sum-checks
 * (/root/reference/src/proof/nova.rs:65-71).  The protocol is lurk_hip_spartan_prove_dev's (or _prove_batch_dev's) step for step up to and
 * including the squeeze of gamma - same prologue, labels, absorb order, sum-checks, zero padding to N = max(num_cons, num_vars) - over
 * LURK_FIELD_BN254_FR; tests/spartan_kzg_ref.py restates it in Python integers.  From there nothing of the inner-product argument is
 * squeezed.  joint = sum_k gamma^k pad_N(P_k) over P = (W, E) (batched: W_0, E_0, W_1, ...; lurk_hip_fold_padded_dev), the claim is
 * y = sum_k gamma^k evals_batch[k] at x = r_z (x_0 <-> the most significant index bit on both sides: r_z passes through unchanged),
 * and lurk_hip_hyperkzg_prove_dev opens joint at x with its challenges bound to the same transcript:
 *     stage 0: com_1 .. com_{ell-1} absorbed as points under "kzg_com", r squeezed under "kzg_r"  (r = 0 fails the call)
 *     stage 1: the 3 ell values v (t-major) absorbed under "kzg_v", q squeezed under "kzg_q"
 *     stage 2 (verifier only): W_0, W_1, W_2 absorbed under "kzg_W", d squeezed under "kzg_d"
 * The prover compares the y of the opening with the claim: a mismatch is an internal error.  N >= 2; N = 1 cannot occur (num_cons and
 * num_vars are at least 2) and is refused by name.
 *   key: a resident BN254 G1 key - the powers-of-tau key that committed W and E - with at least N points; any other curve is refused by
 *   name.  The shapes must be over LURK_FIELD_BN254_FR.  There is no inner-product base.  Every other argument as for the Pasta calls.
 *   Outputs: the seven sum-check fields as lurk_hip_spartan_proof / _batch_proof; kzg_com (log2 N - 1) x 96 B Jacobians (may be NULL
 *   when N = 2), kzg_v 3 log2 N x 32 B canonical (t-major), kzg_w 3 x 96 B Jacobians. */
typedef struct lurk_hip_spartan_kzg_proof {
    void* polys_outer;
    void* claims_outer;
    void* eval_e;
    void* polys_inner;
    void* eval_w;
    void* polys_batch;
    void* evals_batch;
    void* kzg_com;
    void* kzg_v;
    void* kzg_w;
} lurk_hip_spartan_kzg_proof;
typedef struct lurk_hip_spartan_kzg_batch_proof {
    void* polys_outer;
    void* claims_outer;
    void* evals_e;
    void* polys_inner;
    void* evals_w;
    void* polys_batch;
    void* evals_batch;
    void* kzg_com;
    void* kzg_v;
    void* kzg_w;
} lurk_hip_spartan_kzg_batch_proof;
int lurk_hip_spartan_kzg_prove_dev(const lurk_hip_r1cs* shape, const lurk_hip_r1cs* shape_t, size_t num_cons, size_t num_vars, size_t num_io,
                                   lurk_hip_msm_ctx* key, const void* x32_canonical, const void* u32_canonical, const void* d_w32_mont,
                                   const void* d_e32_mont, const void* comm_w_jacobian96, const void* comm_e_jacobian96, const void* label,
                                   size_t label_len, lurk_hip_spartan_kzg_proof* out, void* stream);
int lurk_hip_spartan_kzg_prove_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, lurk_hip_msm_ctx* key, const void* label,
                                         size_t label_len, lurk_hip_spartan_kzg_batch_proof* out, void* stream);
/* The verifiers UP TO THE PAIRING, as lurk_hip_hyperkzg_pairing_inputs: the transcript replayed, the checks of lurk_hip_spartan_verify_dev /
 * _verify_batch_dev through the batch sum-check, then on the host C = comm_W + gamma comm_E (batched: sum_k gamma^k comm_k), y, HyperKZG's
 * scalar checks and the pairing's two G1 inputs L and R (96-byte Jacobians): the proof is valid iff *accepted and e(L, H) = e(R, [tau] H),
 * the caller's pairing.  *accepted = 1: accepted SO FAR.  *failed_check (may be NULL): LURK_VERIFY_OUTER / INNER / BATCH as above,
 * LURK_VERIFY_OPENING for HyperKZG's scalar checks, LURK_VERIFY_MALFORMED before any arithmetic for a scalar not below the group order or
 * a point off the curve, and for r = 0; L and R are then the identity.  No key: HyperKZG's verifier needs only G = (1, 2).  Device work
 * (on the shape's device): two eq tables and one sparse evaluation per shape.  The shapes must be over LURK_FIELD_BN254_FR. */
int lurk_hip_spartan_kzg_verify_dev(const lurk_hip_r1cs* shape, size_t num_cons, size_t num_vars, size_t num_io, const void* x32_canonical,
                                    const void* u32_canonical, const void* comm_w_jacobian96, const void* comm_e_jacobian96, const void* label,
                                    size_t label_len, const lurk_hip_spartan_kzg_proof* proof, void* out_l_jacobian96, void* out_r_jacobian96,
                                    int* accepted, int* failed_check, void* stream);
int lurk_hip_spartan_kzg_verify_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, const void* label, size_t label_len,
                                          const lurk_hip_spartan_kzg_batch_proof* proof, void* out_l_jacobian96, void* out_r_jacobian96,
                                          int* accepted, int* failed_check, void* stream);
/* The same two verifiers DECIDING: the calls above unchanged, then e(L, H) e(-R, tau_H) == 1 on the host (lurk_hip_bn254_pairing_check's
 * arithmetic) against the verifier key tau_H = [tau]H, a 128-byte G2 point, in place of the two outputs.  *accepted = 1: the proof is
 * VALID.  Every failure the calls above report keeps its code; LURK_VERIFY_PAIRING when only the pairing equation fails; a tau_H off
 * the twist, outside the order-r subgroup or the identity gives LURK_VERIFY_MALFORMED whatever the proof. */
int lurk_hip_spartan_kzg_verify_pairing_dev(const lurk_hip_r1cs* shape, size_t num_cons, size_t num_vars, size_t num_io, const void* x32_canonical,
                                            const void* u32_canonical, const void* comm_w_jacobian96, const void* comm_e_jacobian96,
                                            const void* label, size_t label_len, const lurk_hip_spartan_kzg_proof* proof,
                                            const void* tau_h_g2_affine128, int* accepted, int* failed_check, void* stream);
int lurk_hip_spartan_kzg_verify_pairing_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, const void* label,
                                                  size_t label_len, const lurk_hip_spartan_kzg_batch_proof* proof,
                                                  const void* tau_h_g2_affine128, int* accepted, int* failed_check, void* stream);

/* ---- synthetic inputs (bench / tests) -------------------------------------
 * SplitMix64 counter mode, seed 0x4C55524B.  dist 0 = uniform, 1 = witness-like. */
int lurk_hip_synth_scalars_dev(int field_id, uint64_t stream_id, int dist, size_t first, size_t n,
                               void* d_out32, int out_mont, void* stream);
/* bases P_i = [k_i]G, k_i = uniform(stream 0, first+i) (0 -> 1); affine Montgomery, 64 B each */
int lurk_hip_synth_bases_dev(int curve, size_t first, size_t n, void* d_out_affine64, void* stream);
/* A powers-of-tau key for tests and benchmarks of the HyperKZG argument: d_out[i] = [tau^(first + i)] G on BN254 G1 (G = (1, 2)),
 * affine Montgomery, from the same fixed-base tables.  tau: a canonical Fr value in host memory.  INSECURE BY CONSTRUCTION: whoever
 * knows tau (the caller does) can open any commitment to anything - a trapdoor setup that makes a proof checkable without a pairing
 * (L == [tau] R in G1), never a key to prove under.  Other curves are refused by name. */
int lurk_hip_synth_kzg_bases_dev(int curve, const void* tau32_canonical, size_t first, size_t n, void* d_out_affine64, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LURK_HIP_H */
