// spartan.hip - the single-instance compressing prover as host code of the library.
//
// What CompressedSNARK::prove runs on the primary curve (/root/reference/src/proof/nova.rs:341-356 -> arecibo RelaxedR1CSSNARK::prove):
// outer cubic sum-check of eq(tau) (Az Bz - (u Cz + E)), inner quadratic sum-check of (A + r B + r^2 C)(r_x, .) z, the two evaluation
// claims (W at r_y[1..], E at r_x) batched to one point by a third sum-check, one inner-product argument under the resident key.
// The PROTOCOL (labels, order of what is absorbed, zero padding of the two polynomials to a common length) is this repository's own,
// restated in oracle/spartan_ref.py / oracle/spartan_fast.py, whose prover this one equals element for element and whose verifier
// accepts its proofs; the transcript construction is arecibo's Keccak256Transcript (transcript.hip).  Parity unpinned upstream.
//
// Everything here is a sequence of the library's own entry points - multiply_vec on the shape and on its transpose, eq_evals, fold_vec,
// inner products, the sum-check and inner-product round loops with the Keccak round bindings - with the vectors resident and the
// field arithmetic of the claims on the host: lurk_beta_amd/spartan.py: SpartanProver.prove did the same from Python (0.4 ms of
// interpreter between the sum-checks, 0.8 ms between proofs).
#include <algorithm>

#include "spartan_transcript.hpp"

namespace lurk {

// ---- the opening step: what the provers run after the squeeze of gamma -----------------------------------------------------------------
// Both provers end with `count` polynomials of different lengths (raw / raw_len; `padded`: the same zero-padded to N), the powers of
// gamma, their evaluations at r_z; the opening proves  (sum_k gamma^k pad_N(P_k))(r_z) = sum_k gamma^k evals[k].
template <class F>
struct SpOpenArgs {
    SpTranscript& tr;
    int curve, field_id;
    size_t N;
    size_t count;
    const void* const* raw;
    const size_t* raw_len;
    const void* const* padded;
    const Fe<F>& gamma;
    const std::vector<Fe<F>>& evals;
    const std::vector<Fe<F>>& r_z;
    hipStream_t s;
};

// the inner-product argument under the resident key (the Pasta provers): joint from the padded copies by count - 1 fold_vec passes
template <class F>
struct IpaOpening {
    lurk_hip_msm_ctx* key;
    const void* ck_c_jac96;
    void *ipa_l, *ipa_r, *ipa_a;
    void operator()(const SpOpenArgs<F>& a) const {
        void* vs = (void*)a.s;
        const int ell = sp_log2(a.N);
        SpScratch joint(a.N * 32, a.s), eq_rz(a.N * 32, a.s);
        {
            Fe<F> g = a.gamma;
            for (size_t k = 1; k < a.count; k++) {  // joint = P_0 + gamma P_1, then joint += gamma^k P_k (element-wise: in place)
                nested_ok(lurk_hip_fold_vec_dev(a.field_id, k == 1 ? a.padded[0] : joint.p, a.padded[k], g.l, a.N, joint.p, vs));
                g = fe_mul<F>(g, a.gamma);
            }
        }
        const Fe<F> r0 = sp_squeeze<F>(a.tr.t, splabel::IPA_R0, a.field_id);
        uint64_t ck_c_scaled[12], ck_hat[8];
        nested_ok(lurk_hip_point_mul(a.curve, ck_c_scaled, ck_c_jac96, r0.l, 1));
        sp_eq<F>(a.field_id, a.r_z, eq_rz.p, a.s);
        std::vector<uint64_t> keep;
        lurk_hip_keccak_round_binding b = sp_round_binding(a.tr.t, a.field_id, a.curve, keep, ell, splabel::IPA_L, splabel::IPA_R, splabel::IPA_CHALLENGE, 0);
        nested_ok(lurk_hip_ipa_prove_dev(key, joint.p, eq_rz.p, a.N, ck_c_scaled, lurk_hip_keccak_ipa_challenge, &b, ipa_l, ipa_r, ipa_a, ck_hat, vs));
    }
};

// HyperKZG under a resident BN254 G1 key: joint straight from the unpadded vectors in one pass (fold_padded_kernel), the opening's two
// prover challenges over the same transcript (spartan_transcript.hpp: sp_kzg_stage)
static int sp_kzg_challenge(void* user, int stage, const void* data, size_t count, void* out32_canonical) {
    return host_guarded([&] {
        LURK_REQUIRE(stage == 0 || stage == 1, "unknown stage");
        const Fe<Bn254Fr> c = sp_kzg_stage<Bn254Fr>(((SpTranscript*)user)->t, stage, data, count);
        fe_write_canonical<Bn254Fr>(out32_canonical, c);
    });
}
template <class F>
struct KzgOpening {
    lurk_hip_msm_ctx* key;
    void *kzg_com, *kzg_v, *kzg_w;
    void operator()(const SpOpenArgs<F>& a) const {
        LURK_REQUIRE(a.N >= 2, "the HyperKZG opening needs N = max(num_cons, num_vars) >= 2: N = 1 has no variable to fold");
        SpScratch joint(a.N * 32, a.s);
        std::vector<Fe<F>> pw(a.count);
        Fe<F> g = fe_one<F>(), claim = fe_zero<F>();
        for (size_t k = 0; k < a.count; k++) {
            pw[k] = g;
            claim = fe_add<F>(claim, fe_mul<F>(g, a.evals[k]));
            g = fe_mul<F>(g, a.gamma);
        }
        nested_ok(lurk_hip_fold_padded_dev(a.field_id, (int)a.count, a.raw, a.raw_len, pw.data(), a.N, joint.p, (void*)a.s));
        uint64_t y[4], want[4];
        nested_ok(lurk_hip_hyperkzg_prove_dev(key, joint.p, a.N, a.r_z.data(), sp_kzg_challenge, &a.tr, kzg_com, kzg_v, kzg_w, y, (void*)a.s));
        fe_write_canonical<F>(want, claim);
        if (memcmp(y, want, 32) != 0)
            throw HipFailure{LURK_HIP_ERR_HIP, "spartan_kzg: the opening's value differs from the batched evaluation claim (point order or padding)"};
    }
};

template <class F, class Proof, class Opening>
static void spartan_prove(int curve, int field_id, const lurk_hip_r1cs* shape, const lurk_hip_r1cs* shape_t, size_t nc, size_t nv, size_t nio,
                          const void* x_canonical, const void* u_canonical, const void* d_w,
                          const void* d_e, const void* comm_w_jac96, const void* comm_e_jac96, const void* label, size_t label_len,
                          Proof* out, const Opening& open, hipStream_t s) {
    const int ell_x = sp_log2(nc), ell_y = sp_log2(nv) + 1;
    const size_t N = nc > nv ? nc : nv;
    const int ell = sp_log2(N);
    void* vs = (void*)s;
    stream_pool_retain();
    SpTranscript tr;
    std::vector<Fe<F>> ux;
    sp_prologue<F>(tr, curve, label, label_len, comm_w_jac96, comm_e_jac96, u_canonical, x_canonical, nio, ux);
    // z = [W | u | X | 0 ...] of length 2 num_vars
    SpScratch z(2 * nv * 32, s), az(nc * 32, s), bz(nc * 32, s), cz(nc * 32, s);
    LURK_HIP_CHECK(hipMemsetAsync(z.p, 0, 2 * nv * 32, s));
    LURK_HIP_CHECK(hipMemcpyAsync(z.p, d_w, nv * 32, hipMemcpyDeviceToDevice, s));
    LURK_HIP_CHECK(hipMemcpyAsync((char*)z.p + nv * 32, ux.data(), (1 + nio) * 32, hipMemcpyHostToDevice, s));
    nested_ok(lurk_hip_r1cs_multiply_vec_dev(shape, z.p, az.p, bz.p, cz.p, vs));
    std::vector<Fe<F>> tau(ell_x);
    for (int j = 0; j < ell_x; j++) tau[j] = sp_squeeze<F>(tr.t, splabel::TAU, field_id);
    SpScratch d_tau(nc * 32, s), ucze(nc * 32, s);
    sp_eq<F>(field_id, tau, d_tau.p, s);
    nested_ok(lurk_hip_fold_vec_dev(field_id, d_e, cz.p, ux[0].l, nc, ucze.p, vs));  // E + u Cz
    // ---- outer sum-check: eq(tau) (Az Bz - (u Cz + E)), claim 0; Az and Bz are consumed, Cz and E are needed afterwards
    const uint64_t zero32[4] = {0, 0, 0, 0};
    std::vector<Fe<F>> r_x, r_y, r_z;
    auto challenges = [&](const std::vector<uint64_t>& buf, int rounds, std::vector<Fe<F>>& into) {
        into.resize(rounds);
        for (int j = 0; j < rounds; j++) into[j] = fe_read_canonical<F>(buf.data() + 4 * j);
    };
    auto binding = [&](std::vector<uint64_t>& keep, int rounds, const char* absorb, const char* absorb2, const char* squeeze) {
        return sp_round_binding(tr.t, field_id, curve, keep, rounds, absorb, absorb2, squeeze, 0);
    };
    uint64_t finals4[16], claim_out[4];
    {
        void* tabs[4] = {d_tau.p, az.p, bz.p, ucze.p};  // (consumed: nothing reads Az, Bz or the other two afterwards)
        std::vector<uint64_t> keep;
        lurk_hip_keccak_round_binding b = binding(keep, ell_x, splabel::POLY, nullptr, splabel::CHALLENGE);
        b.n_scalars = 4;
        nested_ok(lurk_hip_sumcheck_prove_dev(field_id, 3, tabs, nc, zero32, lurk_hip_keccak_sumcheck_challenge, &b, out->polys_outer, finals4, claim_out, vs));
        challenges(keep, ell_x, r_x);
    }
    const Fe<F> claim_az = fe_read_canonical<F>(finals4 + 4), claim_bz = fe_read_canonical<F>(finals4 + 8);
    const Fe<F> claim_cz = sp_mle<F>(field_id, cz.p, r_x, s), eval_e = sp_mle<F>(field_id, d_e, r_x, s);
    fe_write_canonical<F>((char*)out->claims_outer, claim_az);
    fe_write_canonical<F>((char*)out->claims_outer + 32, claim_bz);
    fe_write_canonical<F>((char*)out->claims_outer + 64, claim_cz);
    fe_write_canonical<F>(out->eval_e, eval_e);
    sp_absorb<F>(tr.t, splabel::CLAIMS_OUTER, {claim_az, claim_bz, claim_cz, eval_e});
    const Fe<F> r = sp_squeeze<F>(tr.t, splabel::R, field_id), r2 = fe_mul<F>(r, r);
    const Fe<F> claim_inner = fe_add<F>(fe_add<F>(claim_az, fe_mul<F>(r, claim_bz)), fe_mul<F>(r2, claim_cz));
    // ---- inner sum-check: (A + r B + r^2 C)(r_x, .) z over the 2 num_vars columns: the transposed shape applied to eq(r_x)
    SpScratch abc(2 * nv * 32, s);
    {
        SpScratch eq_rx(nc * 32, s), ea(2 * nv * 32, s), eb(2 * nv * 32, s), ec(2 * nv * 32, s), ab(2 * nv * 32, s);
        sp_eq<F>(field_id, r_x, eq_rx.p, s);
        nested_ok(lurk_hip_r1cs_multiply_vec_dev(shape_t, eq_rx.p, ea.p, eb.p, ec.p, vs));
        nested_ok(lurk_hip_fold_vec_dev(field_id, ea.p, eb.p, r.l, 2 * nv, ab.p, vs));
        nested_ok(lurk_hip_fold_vec_dev(field_id, ab.p, ec.p, r2.l, 2 * nv, abc.p, vs));  // (the block's scratch is released in stream order)
    }
    {
        void* tabs[2] = {abc.p, z.p};  // (z is consumed: W itself is read below, not z)
        uint64_t claim_can[4];
        fe_write_canonical<F>(claim_can, claim_inner);
        std::vector<uint64_t> keep;
        lurk_hip_keccak_round_binding b = binding(keep, ell_y, splabel::POLY, nullptr, splabel::CHALLENGE);
        b.n_scalars = 3;
        uint64_t fin2[8];
        nested_ok(lurk_hip_sumcheck_prove_dev(field_id, 2, tabs, 2 * nv, claim_can, lurk_hip_keccak_sumcheck_challenge, &b, out->polys_inner, fin2, claim_out, vs));
        challenges(keep, ell_y, r_y);
    }
    const std::vector<Fe<F>> r_y_tail(r_y.begin() + 1, r_y.end());
    const Fe<F> eval_w = sp_mle<F>(field_id, d_w, r_y_tail, s);
    fe_write_canonical<F>(out->eval_w, eval_w);
    sp_absorb<F>(tr.t, splabel::EVAL_W, {eval_w});
    // ---- the two evaluation claims -> one point: W and E zero-padded to N, their points padded with leading zeros
    SpScratch p1(N * 32, s), p2(N * 32, s);
    LURK_HIP_CHECK(hipMemsetAsync(p1.p, 0, N * 32, s));
    LURK_HIP_CHECK(hipMemsetAsync(p2.p, 0, N * 32, s));
    LURK_HIP_CHECK(hipMemcpyAsync(p1.p, d_w, nv * 32, hipMemcpyDeviceToDevice, s));
    LURK_HIP_CHECK(hipMemcpyAsync(p2.p, d_e, nc * 32, hipMemcpyDeviceToDevice, s));
    std::vector<Fe<F>> x1((size_t)ell - (ell_y - 1), fe_zero<F>()), x2((size_t)ell - ell_x, fe_zero<F>());
    x1.insert(x1.end(), r_y_tail.begin(), r_y_tail.end());
    x2.insert(x2.end(), r_x.begin(), r_x.end());
    const Fe<F> rho = sp_squeeze<F>(tr.t, splabel::RHO, field_id);
    uint64_t fin_batch[16];
    {
        SpScratch e1(N * 32, s), e2(N * 32, s), q1(N * 32, s), q2(N * 32, s);
        sp_eq<F>(field_id, x1, e1.p, s);
        sp_eq<F>(field_id, x2, e2.p, s);
        LURK_HIP_CHECK(hipMemcpyAsync(q1.p, p1.p, N * 32, hipMemcpyDeviceToDevice, s));
        LURK_HIP_CHECK(hipMemcpyAsync(q2.p, p2.p, N * 32, hipMemcpyDeviceToDevice, s));
        void* tabs[4] = {e1.p, q1.p, e2.p, q2.p};
        uint64_t coeffs[8], claim_can[4];
        const Fe<F> one = fe_one<F>();
        fe_write_canonical<F>(coeffs, one);
        fe_write_canonical<F>(coeffs + 4, rho);
        fe_write_canonical<F>(claim_can, fe_add<F>(eval_w, fe_mul<F>(rho, eval_e)));
        std::vector<uint64_t> keep;
        lurk_hip_keccak_round_binding b = binding(keep, ell, splabel::POLY, nullptr, splabel::CHALLENGE);
        b.n_scalars = 3;
        nested_ok(lurk_hip_sumcheck_prove_batch_dev(field_id, 2, 2, tabs, N, coeffs, claim_can, lurk_hip_keccak_sumcheck_challenge, &b, out->polys_batch, fin_batch,
                                                    claim_out, vs));
        challenges(keep, ell, r_z);
    }
    const Fe<F> ev1 = fe_read_canonical<F>(fin_batch + 4), ev2 = fe_read_canonical<F>(fin_batch + 12);  // (A_i(r), B_i(r)) per instance: the B's
    fe_write_canonical<F>((char*)out->evals_batch, ev1);
    fe_write_canonical<F>((char*)out->evals_batch + 32, ev2);
    sp_absorb<F>(tr.t, splabel::EVALS_BATCH, {ev1, ev2});
    const Fe<F> gamma = sp_squeeze<F>(tr.t, splabel::GAMMA, field_id);
    {
        const void* raw[2] = {d_w, d_e};
        const size_t raw_len[2] = {nv, nc};
        const void* padded[2] = {p1.p, p2.p};
        const std::vector<Fe<F>> evals = {ev1, ev2};
        open(SpOpenArgs<F>{tr, curve, field_id, N, 2, raw, raw_len, padded, gamma, evals, r_z, s});
    }
    LURK_HIP_CHECK(hipStreamSynchronize(s));
}

// ---- the batched prover: several relaxed instances of different shapes and sizes, one key, ONE proof ---------------------------------
// The structure of arecibo's spartan::batched::BatchedRelaxedR1CSSNARK, which lurk-beta's SuperNova prover compresses with
// (/root/reference/src/proof/supernova.rs:110, 293-302): one outer (cubic) and one inner (quadratic) sum-check shared by all instances
// through powers of a challenge, every instance's two evaluation claims batched to one point, one opening under the resident key.
// = lurk_beta_amd/spartan.py: BatchedSpartanProver.prove call for call (which stays as the test mirror) = oracle/spartan_fast.py:
// prove_batched element for element; instances shorter than the largest are zero-padded, their points padded with leading zeros.
template <class F, class Proof, class Opening>
static void spartan_prove_batch(int curve, int field_id, const lurk_hip_spartan_instance* inst, size_t n, const void* label, size_t label_len, Proof* out,
                                const Opening& open, hipStream_t s) {
    void* vs = (void*)s;
    size_t max_nc = 0, max_nv = 0;
    for (size_t i = 0; i < n; i++) {
        max_nc = inst[i].num_cons > max_nc ? inst[i].num_cons : max_nc;
        max_nv = inst[i].num_vars > max_nv ? inst[i].num_vars : max_nv;
    }
    const int ell_x = sp_log2(max_nc), ell_y = sp_log2(max_nv) + 1;
    const size_t N = max_nc > max_nv ? max_nc : max_nv, LX = (size_t)1 << ell_x, LY = (size_t)1 << ell_y;
    const int ell = sp_log2(N);
    stream_pool_retain();
    SpTranscript tr;
    std::vector<std::vector<Fe<F>>> ux;
    sp_prologue_batch<F>(tr, curve, label, label_len, inst, n, ux);
    std::vector<Fe<F>> tau(ell_x);
    for (int j = 0; j < ell_x; j++) tau[j] = sp_squeeze<F>(tr.t, splabel::TAU, field_id);
    const Fe<F> rho_o = sp_squeeze<F>(tr.t, splabel::RHO_OUTER, field_id);
    auto powers = [](const Fe<F>& b, size_t count) {
        std::vector<Fe<F>> v(count);
        Fe<F> acc = fe_one<F>();
        for (size_t k = 0; k < count; k++) { v[k] = acc; acc = fe_mul<F>(acc, b); }
        return v;
    };
    auto canon = [](const std::vector<Fe<F>>& v) {
        std::vector<uint64_t> c(4 * v.size());
        for (size_t k = 0; k < v.size(); k++) fe_write_canonical<F>(c.data() + 4 * k, v[k]);
        return c;
    };
    auto challenges = [&](const std::vector<uint64_t>& buf, int rounds, std::vector<Fe<F>>& into) {
        into.resize(rounds);
        for (int j = 0; j < rounds; j++) into[j] = fe_read_canonical<F>(buf.data() + 4 * j);
    };
    auto binding = [&](std::vector<uint64_t>& keep, int rounds, const char* absorb, const char* absorb2, const char* squeeze, int n_scalars) {
        return sp_round_binding(tr.t, field_id, curve, keep, rounds, absorb, absorb2, squeeze, n_scalars);
    };
    typedef std::unique_ptr<SpScratch> Buf;
    auto mk = [&](size_t elems) { return Buf(new SpScratch(elems * 32, s)); };
    auto padded_copy = [&](const void* src, size_t have, size_t want) {  // a fresh table of `want` elements: src, then zeros
        Buf b = mk(want);
        if (want > have) LURK_HIP_CHECK(hipMemsetAsync((char*)b->p + have * 32, 0, (want - have) * 32, s));
        LURK_HIP_CHECK(hipMemcpyAsync(b->p, src, have * 32, hipMemcpyDeviceToDevice, s));
        return b;
    };
    const uint64_t zero32[4] = {0, 0, 0, 0};
    uint64_t claim_out[4];
    Buf d_tau = mk(LX);
    sp_eq<F>(field_id, tau, d_tau->p, s);
    // ---- outer sum-check over all instances: sum_i rho_o^i eq(tau) (Az_i Bz_i - (u_i Cz_i + E_i)), claim 0
    std::vector<Buf> zs(n), czs(n);
    std::vector<Fe<F>> r_x, r_y, r_z;
    std::vector<uint64_t> fin_outer(n * 16);
    {
        std::vector<Buf> keepers;
        std::vector<void*> tabs;
        for (size_t i = 0; i < n; i++) {
            const size_t nc = inst[i].num_cons, nv = inst[i].num_vars, nio = inst[i].num_io;
            zs[i] = mk(2 * nv);
            LURK_HIP_CHECK(hipMemsetAsync(zs[i]->p, 0, 2 * nv * 32, s));
            LURK_HIP_CHECK(hipMemcpyAsync(zs[i]->p, inst[i].d_w32_mont, nv * 32, hipMemcpyDeviceToDevice, s));
            LURK_HIP_CHECK(hipMemcpyAsync((char*)zs[i]->p + nv * 32, ux[i].data(), (1 + nio) * 32, hipMemcpyHostToDevice, s));
            Buf az = mk(LX), bz = mk(LX), ucze = mk(LX), tau_i = mk(LX);
            czs[i] = mk(nc);
            if (LX > nc) {
                LURK_HIP_CHECK(hipMemsetAsync((char*)az->p + nc * 32, 0, (LX - nc) * 32, s));
                LURK_HIP_CHECK(hipMemsetAsync((char*)bz->p + nc * 32, 0, (LX - nc) * 32, s));
                LURK_HIP_CHECK(hipMemsetAsync((char*)ucze->p + nc * 32, 0, (LX - nc) * 32, s));
            }
            nested_ok(lurk_hip_r1cs_multiply_vec_dev(inst[i].shape, zs[i]->p, az->p, bz->p, czs[i]->p, vs));
            nested_ok(lurk_hip_fold_vec_dev(field_id, inst[i].d_e32_mont, czs[i]->p, ux[i][0].l, nc, ucze->p, vs));
            LURK_HIP_CHECK(hipMemcpyAsync(tau_i->p, d_tau->p, LX * 32, hipMemcpyDeviceToDevice, s));  // (every instance binds its own copy)
            for (Buf* b : {&tau_i, &az, &bz, &ucze}) {
                tabs.push_back((*b)->p);
                keepers.push_back(std::move(*b));
            }
        }
        const std::vector<uint64_t> coeffs = canon(powers(rho_o, n));
        std::vector<uint64_t> keep;
        lurk_hip_keccak_round_binding b = binding(keep, ell_x, splabel::POLY, nullptr, splabel::CHALLENGE, 4);
        nested_ok(lurk_hip_sumcheck_prove_batch_dev(field_id, 3, n, tabs.data(), LX, coeffs.data(), zero32, lurk_hip_keccak_sumcheck_challenge, &b, out->polys_outer,
                                                    fin_outer.data(), claim_out, vs));
        challenges(keep, ell_x, r_x);
    }
    Buf eq_rx = mk(LX);
    sp_eq<F>(field_id, r_x, eq_rx->p, s);
    std::vector<Fe<F>> cl_a(n), cl_b(n), cl_c(n), ev_e(n), ev_w(n);
    {
        std::vector<Fe<F>> flat;
        for (size_t i = 0; i < n; i++) {
            const size_t nc = inst[i].num_cons;
            const int px = ell_x - sp_log2(nc);
            cl_a[i] = fe_read_canonical<F>(fin_outer.data() + 16 * i + 4);
            cl_b[i] = fe_read_canonical<F>(fin_outer.data() + 16 * i + 8);
            nested_ok(lurk_hip_inner_product_dev(field_id, czs[i]->p, eq_rx->p, nc, cl_c[i].l, vs));  // Cz_i (padded) at r_x: the leading entries of eq(r_x)
            ev_e[i] = sp_mle<F>(field_id, inst[i].d_e32_mont, std::vector<Fe<F>>(r_x.begin() + px, r_x.end()), s);
            fe_write_canonical<F>((char*)out->claims_outer + 96 * i, cl_a[i]);
            fe_write_canonical<F>((char*)out->claims_outer + 96 * i + 32, cl_b[i]);
            fe_write_canonical<F>((char*)out->claims_outer + 96 * i + 64, cl_c[i]);
            fe_write_canonical<F>((char*)out->evals_e + 32 * i, ev_e[i]);
            flat.push_back(cl_a[i]);
            flat.push_back(cl_b[i]);
            flat.push_back(cl_c[i]);
        }
        flat.insert(flat.end(), ev_e.begin(), ev_e.end());
        sp_absorb<F>(tr.t, splabel::CLAIMS_OUTER, flat);
    }
    const Fe<F> r = sp_squeeze<F>(tr.t, splabel::R, field_id), r2 = fe_mul<F>(r, r);
    const Fe<F> rho_i = sp_squeeze<F>(tr.t, splabel::RHO_INNER, field_id);
    // ---- inner sum-check: sum_i rho_i^i (A_i + r B_i + r^2 C_i)(r_x, .) z_i over 2^ell_y columns
    {
        std::vector<Buf> keepers;
        std::vector<void*> tabs;
        const std::vector<Fe<F>> pw = powers(rho_i, n);
        Fe<F> claim = fe_zero<F>();
        for (size_t i = 0; i < n; i++) {
            const size_t nv = inst[i].num_vars;
            Buf abc = mk(LY), zp = padded_copy(zs[i]->p, 2 * nv, LY);
            {
                SpScratch ea(2 * nv * 32, s), eb(2 * nv * 32, s), ec(2 * nv * 32, s), ab(2 * nv * 32, s);
                nested_ok(lurk_hip_r1cs_multiply_vec_dev(inst[i].shape_t, eq_rx->p, ea.p, eb.p, ec.p, vs));  // eq(r_x)'s first num_cons entries
                nested_ok(lurk_hip_fold_vec_dev(field_id, ea.p, eb.p, r.l, 2 * nv, ab.p, vs));
                nested_ok(lurk_hip_fold_vec_dev(field_id, ab.p, ec.p, r2.l, 2 * nv, abc->p, vs));
            }
            if (LY > 2 * nv) LURK_HIP_CHECK(hipMemsetAsync((char*)abc->p + 2 * nv * 32, 0, (LY - 2 * nv) * 32, s));
            const Fe<F> ci = fe_add<F>(fe_add<F>(cl_a[i], fe_mul<F>(r, cl_b[i])), fe_mul<F>(r2, cl_c[i]));
            claim = fe_add<F>(claim, fe_mul<F>(pw[i], ci));
            tabs.push_back(abc->p);
            tabs.push_back(zp->p);
            keepers.push_back(std::move(abc));
            keepers.push_back(std::move(zp));
        }
        const std::vector<uint64_t> coeffs = canon(pw);
        uint64_t claim_can[4];
        fe_write_canonical<F>(claim_can, claim);
        std::vector<uint64_t> keep, fin(n * 8);
        lurk_hip_keccak_round_binding b = binding(keep, ell_y, splabel::POLY, nullptr, splabel::CHALLENGE, 3);
        nested_ok(lurk_hip_sumcheck_prove_batch_dev(field_id, 2, n, tabs.data(), LY, coeffs.data(), claim_can, lurk_hip_keccak_sumcheck_challenge, &b, out->polys_inner,
                                                    fin.data(), claim_out, vs));
        challenges(keep, ell_y, r_y);
    }
    for (size_t i = 0; i < n; i++) {
        const int py = ell_y - (sp_log2(inst[i].num_vars) + 1);
        ev_w[i] = sp_mle<F>(field_id, inst[i].d_w32_mont, std::vector<Fe<F>>(r_y.begin() + py + 1, r_y.end()), s);
        fe_write_canonical<F>((char*)out->evals_w + 32 * i, ev_w[i]);
    }
    sp_absorb<F>(tr.t, splabel::EVALS_W, ev_w);
    // ---- all 2 n evaluation claims -> one point
    std::vector<Buf> polys(2 * n);
    std::vector<std::vector<Fe<F>>> points(2 * n);
    std::vector<Fe<F>> claims(2 * n);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = inst[i].num_cons, nv = inst[i].num_vars;
        const int py = ell_y - (sp_log2(nv) + 1), px = ell_x - sp_log2(nc);
        polys[2 * i] = padded_copy(inst[i].d_w32_mont, nv, N);
        polys[2 * i + 1] = padded_copy(inst[i].d_e32_mont, nc, N);
        points[2 * i].assign((size_t)ell - sp_log2(nv), fe_zero<F>());
        points[2 * i].insert(points[2 * i].end(), r_y.begin() + py + 1, r_y.end());
        points[2 * i + 1].assign((size_t)ell - sp_log2(nc), fe_zero<F>());
        points[2 * i + 1].insert(points[2 * i + 1].end(), r_x.begin() + px, r_x.end());
        claims[2 * i] = ev_w[i];
        claims[2 * i + 1] = ev_e[i];
    }
    const Fe<F> rho = sp_squeeze<F>(tr.t, splabel::RHO, field_id);
    std::vector<uint64_t> fin_batch(2 * n * 8);
    {
        std::vector<Buf> keepers;
        std::vector<void*> tabs;
        const std::vector<Fe<F>> pw = powers(rho, 2 * n);
        Fe<F> claim = fe_zero<F>();
        for (size_t k = 0; k < 2 * n; k++) {
            Buf e = mk(N), q = padded_copy(polys[k]->p, N, N);
            sp_eq<F>(field_id, points[k], e->p, s);
            claim = fe_add<F>(claim, fe_mul<F>(pw[k], claims[k]));
            tabs.push_back(e->p);
            tabs.push_back(q->p);
            keepers.push_back(std::move(e));
            keepers.push_back(std::move(q));
        }
        const std::vector<uint64_t> coeffs = canon(pw);
        uint64_t claim_can[4];
        fe_write_canonical<F>(claim_can, claim);
        std::vector<uint64_t> keep;
        lurk_hip_keccak_round_binding b = binding(keep, ell, splabel::POLY, nullptr, splabel::CHALLENGE, 3);
        nested_ok(lurk_hip_sumcheck_prove_batch_dev(field_id, 2, 2 * n, tabs.data(), N, coeffs.data(), claim_can, lurk_hip_keccak_sumcheck_challenge, &b, out->polys_batch,
                                                    fin_batch.data(), claim_out, vs));
        challenges(keep, ell, r_z);
    }
    std::vector<Fe<F>> evals_batch(2 * n);
    for (size_t k = 0; k < 2 * n; k++) {
        evals_batch[k] = fe_read_canonical<F>(fin_batch.data() + 8 * k + 4);  // (eq_k(r_z), poly_k(r_z)): the polynomial's
        fe_write_canonical<F>((char*)out->evals_batch + 32 * k, evals_batch[k]);
    }
    sp_absorb<F>(tr.t, splabel::EVALS_BATCH, evals_batch);
    const Fe<F> gamma = sp_squeeze<F>(tr.t, splabel::GAMMA, field_id);
    {
        std::vector<const void*> raw(2 * n), padded(2 * n);
        std::vector<size_t> raw_len(2 * n);
        for (size_t i = 0; i < n; i++) {
            raw[2 * i] = inst[i].d_w32_mont;
            raw_len[2 * i] = inst[i].num_vars;
            raw[2 * i + 1] = inst[i].d_e32_mont;
            raw_len[2 * i + 1] = inst[i].num_cons;
        }
        for (size_t k = 0; k < 2 * n; k++) padded[k] = polys[k]->p;
        open(SpOpenArgs<F>{tr, curve, field_id, N, 2 * n, raw.data(), raw_len.data(), padded.data(), gamma, evals_batch, r_z, s});
    }
    LURK_HIP_CHECK(hipStreamSynchronize(s));
}

// ---- what the entry points check before anything is launched ---------------------------------------------------------------------------
struct SpKey {
    int curve = 0, device = 0;
    size_t points = 0;
};
static SpKey sp_key_info(const lurk_hip_msm_ctx* key) {
    SpKey k;
    int bits = 0;
    if (lurk_hip_msm_ctx_info(key, &k.curve, &k.points, &bits, nullptr) != 0 || lurk_hip_msm_ctx_device(key, &k.device) != 0)
        throw HipFailure{LURK_HIP_ERR_INVALID_ARG, lurk_hip_last_error()};
    return k;
}
// the HyperKZG provers: a key on BN254 G1, in the wording of lurk_hip_hyperkzg_prove_dev
static void require_bn254_key(const SpKey& k, const char* what) {
    if (k.curve != LURK_CURVE_BN254) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string(what) + " needs a key on BN254 G1: this key is on " + curve_name(k.curve)};
}
// every scratch vector of a prover is sized from (num_cons, num_vars, num_io) while the mat-vecs write what the shapes say: the two must agree
// (the transposed shape is 2 num_vars rows over the num_cons columns, stored as num_vars = num_cons - 1, num_io = 0), and the shapes' field
// must be the scalar field of the key's curve
static void sp_check_instance(const lurk_hip_r1cs* shape, const lurk_hip_r1cs* shape_t, size_t num_cons, size_t num_vars, size_t num_io, const SpKey& k, int want_field,
                              const char* whose) {
    LURK_REQUIRE(num_cons >= 2 && (num_cons & (num_cons - 1)) == 0 && num_vars >= 2 && (num_vars & (num_vars - 1)) == 0, "num_cons and num_vars must be powers of two >= 2");
    LURK_REQUIRE(1 + num_io <= num_vars, "the public IO does not fit the second half of z");
    LURK_REQUIRE(k.points >= (num_cons > num_vars ? num_cons : num_vars), "the key has fewer points than the padded polynomials have elements");
    int f = -1, ft = -1;
    size_t c = 0, v = 0, io = 0, ct = 0, vt = 0, iot = 0;
    if (lurk_hip_r1cs_dims(shape, &f, &c, &v, &io) != 0 || lurk_hip_r1cs_dims(shape_t, &ft, &ct, &vt, &iot) != 0)
        throw HipFailure{LURK_HIP_ERR_INVALID_ARG, lurk_hip_last_error()};
    LURK_REQUIRE(c == num_cons && v == num_vars && io == num_io, std::string("shape: its (num_cons, num_vars, num_io) differ from the ") + whose);
    LURK_REQUIRE(ct == 2 * num_vars && vt + 1 + iot == num_cons, "shape_t: not the transpose of the shape (2 num_vars rows over num_cons columns)");
    if (want_field == LURK_FIELD_BN254_FR) {
        LURK_REQUIRE(f == want_field && ft == want_field, "the shapes are not over LURK_FIELD_BN254_FR, the scalar field of BN254 G1");
    } else {
        LURK_REQUIRE(f == want_field && ft == want_field, "the shapes are not over the scalar field of the key's curve");
    }
}
static void sp_check_batch(const lurk_hip_spartan_instance* instances, size_t n_instances, const SpKey& k, int want_field) {
    for (size_t i = 0; i < n_instances; i++) {
        const lurk_hip_spartan_instance& it = instances[i];
        LURK_REQUIRE(it.shape && it.shape_t && it.u32_canonical && it.d_w32_mont && it.d_e32_mont && it.comm_w_jacobian96 && it.comm_e_jacobian96, "null instance field");
        LURK_REQUIRE(it.num_io == 0 || it.x32_canonical, "null public IO");
        sp_check_instance(it.shape, it.shape_t, it.num_cons, it.num_vars, it.num_io, k, want_field, "instance's");
    }
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_spartan_prove_dev(const lurk_hip_r1cs* shape, const lurk_hip_r1cs* shape_t, size_t num_cons, size_t num_vars, size_t num_io, lurk_hip_msm_ctx* key,
                               const void* ck_c_jacobian96, const void* x32_canonical, const void* u32_canonical, const void* d_w, const void* d_e,
                               const void* comm_w_jacobian96, const void* comm_e_jacobian96, const void* label, size_t label_len, lurk_hip_spartan_proof* out,
                               void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && shape_t && key && ck_c_jacobian96 && u32_canonical && d_w && d_e && comm_w_jacobian96 && comm_e_jacobian96 && out, "null argument");
        LURK_REQUIRE(num_io == 0 || x32_canonical, "null public IO");
        LURK_REQUIRE(label || label_len == 0, "null label");
        LURK_REQUIRE(out->polys_outer && out->claims_outer && out->eval_e && out->polys_inner && out->eval_w && out->polys_batch && out->evals_batch && out->ipa_l &&
                         out->ipa_r && out->ipa_a,
                     "null output buffer");
        const SpKey k = sp_key_info(key);
        require_pasta_curve(k.curve, "lurk_hip_spartan_prove_dev");
        sp_check_instance(shape, shape_t, num_cons, num_vars, num_io, k, k.curve == LURK_CURVE_PALLAS ? LURK_FIELD_PALLAS_FQ : LURK_FIELD_PALLAS_FP, "arguments");
        DeviceGuard dg(k.device);
        with_pasta_curve(k.curve, [&](auto, auto SF) {
            using F = decltype(SF);
            spartan_prove<F>(k.curve, F::ID, shape, shape_t, num_cons, num_vars, num_io, x32_canonical, u32_canonical, d_w, d_e, comm_w_jacobian96, comm_e_jacobian96,
                             label, label_len, out, IpaOpening<F>{key, ck_c_jacobian96, out->ipa_l, out->ipa_r, out->ipa_a}, (hipStream_t)stream);
        });
    });
}

int lurk_hip_spartan_prove_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, lurk_hip_msm_ctx* key, const void* ck_c_jacobian96,
                                     const void* label, size_t label_len, lurk_hip_spartan_batch_proof* out, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(instances && n_instances >= 1 && n_instances <= 64 && key && ck_c_jacobian96 && out, "null argument, or not 1..64 instances");
        LURK_REQUIRE(label || label_len == 0, "null label");
        LURK_REQUIRE(out->polys_outer && out->claims_outer && out->evals_e && out->polys_inner && out->evals_w && out->polys_batch && out->evals_batch && out->ipa_l &&
                         out->ipa_r && out->ipa_a,
                     "null output buffer");
        const SpKey k = sp_key_info(key);
        require_pasta_curve(k.curve, "lurk_hip_spartan_prove_batch_dev");
        sp_check_batch(instances, n_instances, k, k.curve == LURK_CURVE_PALLAS ? LURK_FIELD_PALLAS_FQ : LURK_FIELD_PALLAS_FP);
        DeviceGuard dg(k.device);
        with_pasta_curve(k.curve, [&](auto, auto SF) {
            using F = decltype(SF);
            spartan_prove_batch<F>(k.curve, F::ID, instances, n_instances, label, label_len, out, IpaOpening<F>{key, ck_c_jacobian96, out->ipa_l, out->ipa_r, out->ipa_a},
                                   (hipStream_t)stream);
        });
    });
}

int lurk_hip_spartan_kzg_prove_dev(const lurk_hip_r1cs* shape, const lurk_hip_r1cs* shape_t, size_t num_cons, size_t num_vars, size_t num_io, lurk_hip_msm_ctx* key,
                                   const void* x32_canonical, const void* u32_canonical, const void* d_w, const void* d_e, const void* comm_w_jacobian96,
                                   const void* comm_e_jacobian96, const void* label, size_t label_len, lurk_hip_spartan_kzg_proof* out, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && shape_t && key && u32_canonical && d_w && d_e && comm_w_jacobian96 && comm_e_jacobian96 && out, "null argument");
        LURK_REQUIRE(num_io == 0 || x32_canonical, "null public IO");
        LURK_REQUIRE(label || label_len == 0, "null label");
        const SpKey k = sp_key_info(key);
        require_bn254_key(k, "lurk_hip_spartan_kzg_prove_dev");
        LURK_REQUIRE((num_cons > num_vars ? num_cons : num_vars) != 1, "N = max(num_cons, num_vars) = 1: the HyperKZG opening needs N >= 2");
        sp_check_instance(shape, shape_t, num_cons, num_vars, num_io, k, LURK_FIELD_BN254_FR, "arguments");
        LURK_REQUIRE(out->polys_outer && out->claims_outer && out->eval_e && out->polys_inner && out->eval_w && out->polys_batch && out->evals_batch && out->kzg_v &&
                         out->kzg_w && (out->kzg_com || (num_cons == 2 && num_vars == 2)),
                     "null output buffer");
        DeviceGuard dg(k.device);
        using F = Bn254Fr;
        spartan_prove<F>(k.curve, F::ID, shape, shape_t, num_cons, num_vars, num_io, x32_canonical, u32_canonical, d_w, d_e, comm_w_jacobian96, comm_e_jacobian96, label,
                         label_len, out, KzgOpening<F>{key, out->kzg_com, out->kzg_v, out->kzg_w}, (hipStream_t)stream);
    });
}

int lurk_hip_spartan_kzg_prove_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, lurk_hip_msm_ctx* key, const void* label, size_t label_len,
                                         lurk_hip_spartan_kzg_batch_proof* out, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(instances && n_instances >= 1 && n_instances <= 64 && key && out, "null argument, or not 1..64 instances");
        LURK_REQUIRE(label || label_len == 0, "null label");
        const SpKey k = sp_key_info(key);
        require_bn254_key(k, "lurk_hip_spartan_kzg_prove_batch_dev");
        size_t N = 0;
        for (size_t i = 0; i < n_instances; i++) N = std::max(N, std::max(instances[i].num_cons, instances[i].num_vars));
        LURK_REQUIRE(N != 1, "N = max(num_cons, num_vars) = 1: the HyperKZG opening needs N >= 2");
        sp_check_batch(instances, n_instances, k, LURK_FIELD_BN254_FR);
        LURK_REQUIRE(out->polys_outer && out->claims_outer && out->evals_e && out->polys_inner && out->evals_w && out->polys_batch && out->evals_batch && out->kzg_v &&
                         out->kzg_w && (out->kzg_com || N == 2),
                     "null output buffer");
        DeviceGuard dg(k.device);
        using F = Bn254Fr;
        spartan_prove_batch<F>(k.curve, F::ID, instances, n_instances, label, label_len, out, KzgOpening<F>{key, out->kzg_com, out->kzg_v, out->kzg_w}, (hipStream_t)stream);
    });
}
}
