// bn254_pairing.hip - the C ABI over bn254_pairing.hpp: G2 multiples (a verifier key [tau]H), the pairing-product check, the three KZG
// verifiers that DECIDE (the up-to-the-pairing code of hyperkzg.hip / verify.hip unchanged, then e(L, H) e(-R, [tau]H) == 1), and the
// check of a resident powers-of-tau key against a verifier key.  The pairing is host code and has no kernel; the key check's device work
// is two commitments through the existing paths.
//
// Reference: lurk-beta's compressing proof on its default cycle opens with HyperKZG (src/proof/nova.rs:65-71 of the reference), whose
// verifier ends in this pairing check (arecibo's hyperkzg, un-vendored; the protocol here is the repository's own: hyperkzg.hip).
#include <string>
#include <vector>

#include "common.hpp"
#include "dispatch.hpp"
#include "bn254_pairing.hpp"

namespace lurk {

using bn254::G1;
using bn254::G2;

// why a 128-byte G2 point cannot serve, or nullptr; identity_ok: whether the all-zero point may
static const char* g2_fault(const void* p128, G2& out, bool need_subgroup, bool identity_ok) {
    if (!bn254::g2_read(p128, out)) return "off the twist (a coordinate is not reduced modulo the field order)";
    if (out.inf) return identity_ok ? nullptr : "the identity";
    if (!bn254::g2_on_twist(out)) return "off the twist";
    if (need_subgroup && !bn254::g2_in_subgroup(out)) return "on the twist but outside the order-r subgroup";
    return nullptr;
}
// a verifier key [tau]H: in G2 and not the identity
static bool vk_ok(const void* tau_h128, G2& out) { return g2_fault(tau_h128, out, true, false) == nullptr; }

// e(L, H) e(-R, tau_H) == 1 for the two 96-byte Jacobians an up-to-the-pairing verifier accepted (well-formed by then)
static bool kzg_pairing_holds(const void* l96, const void* r96, const G2& tau_h) {
    G1 ps[2];
    LURK_REQUIRE(bn254::g1_from_jacobian(l96, ps[0]) && bn254::g1_from_jacobian(r96, ps[1]), "the pairing's G1 inputs are not on the curve");
    ps[1] = bn254::g1_neg(ps[1]);
    const G2 qs[2] = {bn254::g2_generator(), tau_h};
    return bn254::pairing_product_is_one(2, ps, qs);
}

static void refuse_other_curves(int curve, const char* entry) {
    if (curve == LURK_CURVE_BN254) return;
    if (curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN)
        throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string(entry) + " is offered on BN254 G1 only, not on " + curve_name(curve)};
    throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "unknown curve id"};
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_bn254_g2_mul(void* out_g2_affine128, const void* g2_affine128, const void* k32_canonical) {
    return host_guarded([&] {
        LURK_REQUIRE(out_g2_affine128 && k32_canonical, "null argument");
        const Fe<Bn254Fr> k = fe_from_mont<Bn254Fr>(fe_read_canonical<Bn254Fr>(k32_canonical, "the scalar"));
        G2 p = bn254::g2_generator();
        if (g2_affine128) {
            const char* why = g2_fault(g2_affine128, p, false, true);
            if (why) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string("lurk_hip_bn254_g2_mul: the point is ") + why};
        }
        bn254::g2_write(out_g2_affine128, bn254::g2_mul(p, k.l));
    });
}

int lurk_hip_bn254_pairing_check(size_t n, const void* g1_jacobian96, const void* g2_affine128, int* product_is_one) {
    return host_guarded([&] {
        LURK_REQUIRE(product_is_one && (n == 0 || (g1_jacobian96 && g2_affine128)), "null argument");
        LURK_REQUIRE(n <= ((size_t)1 << 20), "too many pairs");
        *product_is_one = 0;
        std::vector<G1> ps(n);
        std::vector<G2> qs(n);
        for (size_t i = 0; i < n; i++) {
            if (!bn254::g1_from_jacobian((const char*)g1_jacobian96 + 96 * i, ps[i]))
                throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "lurk_hip_bn254_pairing_check: G1 point " + std::to_string(i) + " is neither the identity nor on the curve"};
            const char* why = g2_fault((const char*)g2_affine128 + 128 * i, qs[i], true, true);
            if (why) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "lurk_hip_bn254_pairing_check: G2 point " + std::to_string(i) + " is " + why};
        }
        *product_is_one = bn254::pairing_product_is_one(n, ps.data(), qs.data()) ? 1 : 0;
    });
}

int lurk_hip_hyperkzg_verify(int curve, int ell, const void* c_jacobian96, const void* x32_canonical, const void* y32_canonical, const void* com_jacobian96,
                             const void* v32_canonical, const void* w_jacobian96, const void* r32_canonical, const void* q32_canonical, const void* d32_canonical,
                             const void* tau_h_g2_affine128, int* accepted, int* failed_check) {
    return host_guarded([&] {
        refuse_other_curves(curve, "lurk_hip_hyperkzg_verify");
        LURK_REQUIRE(tau_h_g2_affine128 && accepted, "null argument");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_HYPERKZG_MALFORMED;
        uint64_t l[12], r[12];
        int ok = 0, failed = 0;
        nested_ok(lurk_hip_hyperkzg_pairing_inputs(curve, ell, c_jacobian96, x32_canonical, y32_canonical, com_jacobian96, v32_canonical, w_jacobian96, r32_canonical,
                                                   q32_canonical, d32_canonical, l, r, &ok, &failed));
        G2 tau_h;
        if (!vk_ok(tau_h_g2_affine128, tau_h)) return;  // malformed input, whatever the proof says
        if (ok) {
            ok = kzg_pairing_holds(l, r, tau_h) ? 1 : 0;
            failed = ok ? LURK_HYPERKZG_ACCEPTED : LURK_HYPERKZG_PAIRING;
        }
        *accepted = ok;
        if (failed_check) *failed_check = failed;
    });
}

int lurk_hip_spartan_kzg_verify_pairing_dev(const lurk_hip_r1cs* shape, size_t num_cons, size_t num_vars, size_t num_io, const void* x32_canonical,
                                            const void* u32_canonical, const void* comm_w_jacobian96, const void* comm_e_jacobian96, const void* label,
                                            size_t label_len, const lurk_hip_spartan_kzg_proof* proof, const void* tau_h_g2_affine128, int* accepted,
                                            int* failed_check, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(tau_h_g2_affine128 && accepted, "null argument");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_VERIFY_MALFORMED;
        uint64_t l[12], r[12];
        int ok = 0, failed = 0;
        nested_ok(lurk_hip_spartan_kzg_verify_dev(shape, num_cons, num_vars, num_io, x32_canonical, u32_canonical, comm_w_jacobian96, comm_e_jacobian96, label, label_len,
                                                  proof, l, r, &ok, &failed, stream));
        G2 tau_h;
        if (!vk_ok(tau_h_g2_affine128, tau_h)) return;
        if (ok) {
            ok = kzg_pairing_holds(l, r, tau_h) ? 1 : 0;
            failed = ok ? LURK_VERIFY_ACCEPTED : LURK_VERIFY_PAIRING;
        }
        *accepted = ok;
        if (failed_check) *failed_check = failed;
    });
}

int lurk_hip_spartan_kzg_verify_pairing_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, const void* label, size_t label_len,
                                                  const lurk_hip_spartan_kzg_batch_proof* proof, const void* tau_h_g2_affine128, int* accepted, int* failed_check,
                                                  void* stream) {
    return guarded([&] {
        LURK_REQUIRE(tau_h_g2_affine128 && accepted, "null argument");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_VERIFY_MALFORMED;
        uint64_t l[12], r[12];
        int ok = 0, failed = 0;
        nested_ok(lurk_hip_spartan_kzg_verify_batch_dev(instances, n_instances, label, label_len, proof, l, r, &ok, &failed, stream));
        G2 tau_h;
        if (!vk_ok(tau_h_g2_affine128, tau_h)) return;
        if (ok) {
            ok = kzg_pairing_holds(l, r, tau_h) ? 1 : 0;
            failed = ok ? LURK_VERIFY_ACCEPTED : LURK_VERIFY_PAIRING;
        }
        *accepted = ok;
        if (failed_check) *failed_check = failed;
    });
}

int lurk_hip_kzg_key_check_dev(lurk_hip_msm_ctx* key, const void* tau_h_g2_affine128, uint64_t seed, int* consistent, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(key && tau_h_g2_affine128 && consistent, "null argument");
        *consistent = 0;
        int curve = 0, bits = 0, device = 0;
        size_t points = 0;
        nested_ok(lurk_hip_msm_ctx_info(key, &curve, &points, &bits, nullptr));
        nested_ok(lurk_hip_msm_ctx_device(key, &device));
        if (curve != LURK_CURVE_BN254)
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string("lurk_hip_kzg_key_check_dev needs a key on BN254 G1: this key is on ") + curve_name(curve)};
        LURK_REQUIRE(points >= 1, "the key has no points");
        G2 tau_h;
        const char* why = g2_fault(tau_h_g2_affine128, tau_h, true, false);
        if (why) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string("lurk_hip_kzg_key_check_dev: the verifier key is ") + why};
        DeviceGuard dg(device);
        hipStream_t s = (hipStream_t)stream;
        // ck[0] == (1, 2): the first record of the resident table is the first point in every form of the key
        Fe<Bn254Fq> first[2];
        LURK_HIP_CHECK(hipMemcpyAsync((void*)first, msm_ctx_table_view(key).table, 64, hipMemcpyDeviceToHost, s));
        LURK_HIP_CHECK(hipStreamSynchronize(s));
        const bool g_ok = fe_eq<Bn254Fq>(first[0], fe_one<Bn254Fq>()) && fe_eq<Bn254Fq>(first[1], fe_from_u64<Bn254Fq>(2));
        if (!g_ok || points == 1) {
            *consistent = g_ok ? 1 : 0;
            return;
        }
        // one buffer (0, rho_0 .. rho_{N-2}, 0): L commits it from element 1 (rho_i against ck[i]), R from element 0 (rho_i against ck[i+1])
        stream_pool_retain();
        ArenaBuf buf((points + 1) * 32, s);
        char* d = (char*)buf.p;
        LURK_HIP_CHECK(hipMemsetAsync(d, 0, 32, s));
        LURK_HIP_CHECK(hipMemsetAsync(d + points * 32, 0, 32, s));
        nested_ok(lurk_hip_synth_scalars_dev(LURK_FIELD_BN254_FR, seed, 0, 0, points - 1, d + 32, 1, stream));
        struct Drain {  // whatever fails, a slot that was submitted is waited for: the key stays usable
            lurk_hip_msm_ctx* key;
            bool pending[2];
            ~Drain() {
                uint64_t sink[12];
                for (int k = 0; k < 2; k++)
                    if (pending[k]) (void)lurk_hip_msm_ctx_wait(key, k, sink);
            }
        } drain{key, {false, false}};
        uint64_t l[12], r[12];
        nested_ok(lurk_hip_msm_ctx_submit_dev(key, 0, d + 32, points - 1, 1, stream));
        drain.pending[0] = true;
        nested_ok(lurk_hip_msm_ctx_submit_dev(key, 1, d, points, 1, stream));
        drain.pending[1] = true;
        drain.pending[0] = false;
        nested_ok(lurk_hip_msm_ctx_wait(key, 0, l));
        drain.pending[1] = false;
        nested_ok(lurk_hip_msm_ctx_wait(key, 1, r));
        LURK_HIP_CHECK(hipStreamSynchronize(s));  // (the scratch buffer goes back to the arena behind the commitments that read it)
        *consistent = kzg_pairing_holds(r, l, tau_h) ? 1 : 0;  // e(R, H) == e(L, tau_H)
    });
}
}
