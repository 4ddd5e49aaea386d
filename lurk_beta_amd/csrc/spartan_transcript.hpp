// spartan_transcript.hpp - what the compressing provers (spartan.hip) and their verifiers (verify.hip) must agree on to the byte: the
// transcript's labels, its prologue (the statement as it is absorbed before the first challenge) and the small helpers both sides
// replay it with.  One place, so that prover and verifier cannot drift.
#pragma once
#include <memory>
#include <vector>

#include "common.hpp"
#include "dispatch.hpp"

namespace lurk {

// the labels of the protocol (oracle/spartan_ref.py, oracle/spartan_fast.py)
namespace splabel {
constexpr const char* N = "n";
constexpr const char* COMM_W = "comm_W";
constexpr const char* COMM_E = "comm_E";
constexpr const char* UX = "uX";
constexpr const char* TAU = "t";
constexpr const char* RHO_OUTER = "rho_outer";
constexpr const char* POLY = "p";
constexpr const char* CHALLENGE = "c";
constexpr const char* CLAIMS_OUTER = "claims_outer";
constexpr const char* R = "r";
constexpr const char* RHO_INNER = "rho_inner";
constexpr const char* EVAL_W = "eval_W";
constexpr const char* EVALS_W = "evals_W";
constexpr const char* RHO = "rho";
constexpr const char* EVALS_BATCH = "evals_batch";
constexpr const char* GAMMA = "gamma";
constexpr const char* IPA_R0 = "ipa_r0";
constexpr const char* IPA_L = "L";
constexpr const char* IPA_R = "R";
constexpr const char* IPA_CHALLENGE = "r";
// the HyperKZG opening of the BN254 provers (tests/spartan_kzg_ref.py)
constexpr const char* KZG_COM = "kzg_com";
constexpr const char* KZG_R = "kzg_r";
constexpr const char* KZG_V = "kzg_v";
constexpr const char* KZG_Q = "kzg_q";
constexpr const char* KZG_W = "kzg_W";
constexpr const char* KZG_D = "kzg_d";
}  // namespace splabel

using SpScratch = ArenaBuf;  // scratch vectors come off the stream's arena (common.hpp): a push, not a hipMallocAsync

struct SpTranscript {
    lurk_hip_keccak_transcript* t = nullptr;
    ~SpTranscript() {
        if (t) (void)lurk_hip_keccak_transcript_destroy(t);
    }
};

template <class F>
static Fe<F> sp_squeeze(lurk_hip_keccak_transcript* t, const char* label, int field_id) {
    uint64_t r[4];
    nested_ok(lurk_hip_keccak_transcript_squeeze(t, label, strlen(label), field_id, r));
    return fe_read_canonical<F>(r);
}
template <class F>
static void sp_absorb(lurk_hip_keccak_transcript* t, const char* label, const std::vector<Fe<F>>& mont_vals) {
    std::vector<uint64_t> can(4 * mont_vals.size());
    for (size_t i = 0; i < mont_vals.size(); i++) fe_write_canonical<F>(can.data() + 4 * i, mont_vals[i]);
    nested_ok(lurk_hip_keccak_transcript_absorb_scalars(t, label, strlen(label), can.data(), mont_vals.size()));
}
// eq(point) as 2^|point| Montgomery elements on the device
template <class F>
static void sp_eq(int field_id, const std::vector<Fe<F>>& point, void* d_out, hipStream_t s) {
    // (the point is copied out of pageable memory before the call returns; every caller's vector outlives the proof anyway)
    nested_ok(lurk_hip_eq_evals_dev(field_id, point.empty() ? nullptr : (const void*)point.data(), (int)point.size(), d_out, (void*)s));
}
// the multilinear extension of a device table at `point` (Montgomery): <table, eq(point)>
template <class F>
static Fe<F> sp_mle(int field_id, const void* d_table, const std::vector<Fe<F>>& point, hipStream_t s) {
    SpScratch eq(((size_t)32) << point.size(), s);
    sp_eq<F>(field_id, point, eq.p, s);
    Fe<F> out;
    nested_ok(lurk_hip_inner_product_dev(field_id, d_table, eq.p, (size_t)1 << point.size(), out.l, (void*)s));
    return out;
}
static int sp_log2(size_t n) {
    int k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

// the challenge of a stage of the HyperKZG opening over the transcript: stage 0 absorbs `count` 96-byte Jacobians of BN254 G1 (com_1 ..
// com_{ell-1}), stage 1 `count` canonical scalars (v, t-major), stage 2 (the verifier's) the three W_t; prover and verifier both come here
template <class F>
static Fe<F> sp_kzg_stage(lurk_hip_keccak_transcript* t, int stage, const void* data, size_t count) {
    const char* absorb = stage == 0 ? splabel::KZG_COM : stage == 1 ? splabel::KZG_V : splabel::KZG_W;
    const char* squeeze = stage == 0 ? splabel::KZG_R : stage == 1 ? splabel::KZG_Q : splabel::KZG_D;
    if (stage == 1) {
        nested_ok(lurk_hip_keccak_transcript_absorb_scalars(t, absorb, strlen(absorb), data, count));
    } else {
        for (size_t i = 0; i < count; i++)
            nested_ok(lurk_hip_keccak_transcript_absorb_point(t, absorb, strlen(absorb), LURK_CURVE_BN254, (const char*)data + 96 * i));
    }
    return sp_squeeze<F>(t, squeeze, F::ID);
}

// ---- the prologues: everything absorbed before the first challenge ---------------------------------------------------------------
// single instance: comm_W, comm_E, (u, X); ux = [u | X] in Montgomery form
template <class F>
static void sp_prologue(SpTranscript& tr, int curve, const void* label, size_t label_len, const void* comm_w_jac96, const void* comm_e_jac96,
                        const void* u_canonical, const void* x_canonical, size_t nio, std::vector<Fe<F>>& ux) {
    nested_ok(lurk_hip_keccak_transcript_new(&tr.t, label, label_len));
    nested_ok(lurk_hip_keccak_transcript_absorb_point(tr.t, splabel::COMM_W, strlen(splabel::COMM_W), curve, comm_w_jac96));
    nested_ok(lurk_hip_keccak_transcript_absorb_point(tr.t, splabel::COMM_E, strlen(splabel::COMM_E), curve, comm_e_jac96));
    ux.resize(1 + nio);
    ux[0] = fe_read_canonical<F>(u_canonical);
    for (size_t i = 0; i < nio; i++) ux[1 + i] = fe_read_canonical<F>((const char*)x_canonical + 32 * i);
    sp_absorb<F>(tr.t, splabel::UX, ux);
}
// batched: the number of instances, then every instance's comm_W, comm_E, (u, X)
template <class F>
static void sp_prologue_batch(SpTranscript& tr, int curve, const void* label, size_t label_len, const lurk_hip_spartan_instance* inst, size_t n,
                              std::vector<std::vector<Fe<F>>>& ux) {
    nested_ok(lurk_hip_keccak_transcript_new(&tr.t, label, label_len));
    {
        Fe<F> nn = fe_from_u64<F>((uint64_t)n);
        sp_absorb<F>(tr.t, splabel::N, {nn});
    }
    ux.resize(n);
    for (size_t i = 0; i < n; i++) {
        nested_ok(lurk_hip_keccak_transcript_absorb_point(tr.t, splabel::COMM_W, strlen(splabel::COMM_W), curve, inst[i].comm_w_jacobian96));
        nested_ok(lurk_hip_keccak_transcript_absorb_point(tr.t, splabel::COMM_E, strlen(splabel::COMM_E), curve, inst[i].comm_e_jacobian96));
        ux[i].resize(1 + inst[i].num_io);
        ux[i][0] = fe_read_canonical<F>(inst[i].u32_canonical);
        for (size_t k = 0; k < inst[i].num_io; k++) ux[i][1 + k] = fe_read_canonical<F>((const char*)inst[i].x32_canonical + 32 * k);
        sp_absorb<F>(tr.t, splabel::UX, ux[i]);
    }
}
// the round binding of a sum-check (n_scalars coefficients under POLY, the challenge under CHALLENGE) or of the opening argument
// (L, R, the challenge); `keep` receives the challenges
static lurk_hip_keccak_round_binding sp_round_binding(lurk_hip_keccak_transcript* t, int field_id, int curve, std::vector<uint64_t>& keep, int rounds,
                                                      const char* absorb, const char* absorb2, const char* squeeze, int n_scalars) {
    keep.assign((size_t)4 * (rounds > 0 ? rounds : 1), 0);
    lurk_hip_keccak_round_binding b;
    memset(&b, 0, sizeof(b));
    b.transcript = t;
    b.field_id = field_id;
    b.curve = curve;
    b.n_scalars = n_scalars;
    b.absorb_label = absorb;
    b.absorb_label_len = strlen(absorb);
    b.absorb_label2 = absorb2;
    b.absorb_label2_len = absorb2 ? strlen(absorb2) : 0;
    b.squeeze_label = squeeze;
    b.squeeze_label_len = strlen(squeeze);
    b.challenges_out = keep.data();
    b.challenges_cap = (size_t)(rounds > 0 ? rounds : 1);
    return b;
}

}  // namespace lurk
