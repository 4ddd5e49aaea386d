// verify.hip - the verifiers of the compressing proofs (spartan.hip's provers), and their two device building blocks.
//
// What CompressedSNARK::verify runs per curve (/root/reference/src/proof/nova.rs:358-373, supernova.rs:304-316 -> arecibo
// RelaxedR1CSSNARK::verify / BatchedRelaxedR1CSSNARK::verify): the three sum-checks replayed over the transcript, the matrices
// evaluated at (r_x, r_y) directly (no preprocessing), one inner-product-argument check under the resident key.  The PROTOCOL is this
// repository's own - oracle/spartan_fast.py: verify / verify_batched, check for check; the transcript's labels and prologue are
// spartan_transcript.hpp's, shared with the provers.
//
// Device work per verification: two eq tables, ONE launch over the shape's non-zeros (sparse_mle_kernel), the s vector of the opening
// argument (ipa_s_vector_kernel), one commitment of s under the resident key.  Everything else - the sum-check rounds, eq(tau, r_x), the
// padding factors, eval_X, b_hat in its closed form, the 2 ell + 5 scalar multiples of the final point equation - is host arithmetic.
//
// sparse_mle_kernel.  M~ = sum_i eq_x[i] sum_k val[k] eq_y[col[k]] for M = A, B, C.  Rows are classed by length and multiplied with
// eq_y as r1cs_shape.cuh has it (RowClasses, r1cs_row), rows without any entry are left out of the lists.  A
// row value (Montgomery-2^261, lazy) is multiplied by eq_x[row] taken as PLAIN limbs of its canonical Montgomery-2^256 form: the
// product a * e / 2^261 is then the Montgomery-2^256 form of the term, below 2^255.3.  The reduction to three elements:
//     lanes -> wave      six shuffle steps on the nine 29-bit limbs, a carry pass every second step (4 x 2^29 < 2^31); the sum of 64
//                        terms is below 2^261.3: its top limb (everything above bit 232) stays below 2^30
//     wave  -> workgroup the wave's sum times 2^266 mod p (one Montgomery product: 32 x the sum, below 2^255.2 again), four of them
//                        added through 108 words of LDS, then f29_to_mont256 (/ 32, canonical)
//     workgroups -> one  a second, three-workgroup kernel adds the 3 x blocks canonical partial sums (fe_add)
// Field addition is exact: the order of the reduction does not change the answer.  No floating point, no atomics.
#include <algorithm>

#include "r1cs_shape.cuh"
#include "curve.cuh"
#include "spartan_transcript.hpp"

namespace lurk {

constexpr int MLE_WAVES = FOLD_BLOCK / 64;

struct MleDev {
    R1csDev s;
    RowClassDev c;
};

// 256 lanes of one class -> the three terms of this lane (zero on every lane that does not lead a live row)
template <class P, int G, bool ANY_LEN>
__device__ __forceinline__ void mle_class(const MleDev& d, const uint32_t* list, uint32_t n, unsigned vb, unsigned nb, uint32_t tid, const Fe<P>* __restrict__ ex,
                                          const Fe<P>* __restrict__ ey, F29<P>* v) {
    const uint32_t* dict = d.s.dict;
    const uint32_t* one29 = dict + d.s.dict_size * P29_STRIDE;
    const RowSlot slot = row_slot<G>(list, n, fold_row_block(vb, nb), tid);
#pragma unroll
    for (int w = 0; w < 3; w++) v[w] = f29_zero<P>();
    if (G == 1 && !slot.live) return;
    const uint32_t row = slot.row, gl = slot.gl;
    const Fe<P> e = ex[row];
    const F29<P> eplain = f29_from_plain<P>(e.l);  // canonical Montgomery-2^256 limbs, unshifted: the product below leaves the 2^261 domain
    const bool lead = slot.live && gl == 0;
    {
        const F29<P> t = f29_mul<P>(eplain, r1cs_row<P, G, ANY_LEN, false>(d.s.a, dict, one29, d.s.a.rowptr[row], d.s.a.rowptr[row + 1], gl, ey));  // eplain tight, the row
        if (lead) v[0] = t;                                                                                                              // loose at most: < 2^254.3 + p
    }
    {
        const F29<P> t = f29_mul<P>(eplain, r1cs_row<P, G, ANY_LEN, false>(d.s.b, dict, one29, d.s.b.rowptr[row], d.s.b.rowptr[row + 1], gl, ey));
        if (lead) v[1] = t;
    }
    {
        const F29<P> t = f29_mul<P>(eplain, r1cs_row<P, G, ANY_LEN, false>(d.s.c, dict, one29, d.s.c.rowptr[row], d.s.c.rowptr[row + 1], gl, ey));
        if (lead) v[2] = t;
    }
}

template <class P>
__global__ __launch_bounds__(FOLD_BLOCK) void sparse_mle_kernel(MleDev d, const Fe<P>* __restrict__ ex, const Fe<P>* __restrict__ ey, Fe<P> k266,
                                                                 Fe<P>* __restrict__ partial) {
    __shared__ uint32_t red[MLE_WAVES][3][9];
    const unsigned j = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    F29<P> v[3];
    row_class_vblock<(int)SAT_GROUP>(d.c, j, [&](auto g, auto any_len, const uint32_t* list, uint32_t n, unsigned vb, unsigned nb) {
        mle_class<P, decltype(g)::value, decltype(any_len)::value>(d, list, n, vb, nb, tid, ex, ey, v);
    });
    // lanes -> wave
    const F29<P> k = f29_from_plain<P>(k266.l);  // 2^266 mod p: x -> 32 x in one Montgomery product
#pragma unroll
    for (int w = 0; w < 3; w++) {
        F29<P> t = v[w];
        int steps = 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int i = 0; i < 9; i++) t.l[i] += __shfl_down(t.l[i], off);
            if (++steps == 2) {
                t = f29_carry<P>(t);
                steps = 0;
            }
        }
        if ((tid & 63) == 0) {
            t = f29_mul<P>(k, t);  // 32 x the wave's sum, < 2^255.2
#pragma unroll
            for (int i = 0; i < 9; i++) red[tid >> 6][w][i] = t.l[i];
        }
    }
    __syncthreads();
    if (tid < 3) {
        F29<P> t = f29_zero<P>();
#pragma unroll
        for (int q = 0; q < MLE_WAVES; q++)
#pragma unroll
            for (int i = 0; i < 9; i++) t.l[i] += red[q][tid][i];
        partial[(size_t)3 * j + tid] = f29_to_mont256<P>(t);  // (carries, / 32, canonical)
    }
}

// out[w] = sum_b partial[3 b + w]: one workgroup per matrix
template <class P>
__global__ __launch_bounds__(FOLD_BLOCK) void sparse_mle_sum_kernel(const Fe<P>* __restrict__ partial, unsigned blocks, Fe<P>* __restrict__ out) {
    __shared__ uint4 raw[FOLD_BLOCK * 2];
    Fe<P>* sh = reinterpret_cast<Fe<P>*>(raw);
    Fe<P> acc = fe_zero<P>();
    for (unsigned b = threadIdx.x; b < blocks; b += FOLD_BLOCK) acc = fe_add<P>(acc, partial[(size_t)3 * b + blockIdx.x]);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = FOLD_BLOCK / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fe_add<P>(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// s[i] = hi[i >> lo_bits] * lo[i & (2^lo_bits - 1)]; tab = [lo table | hi table]
template <class F>
__global__ __launch_bounds__(FOLD_BLOCK) void ipa_s_vector_kernel(const Fe<F>* __restrict__ tab, int lo_bits, size_t n, Fe<F>* __restrict__ out) {
    const size_t mask = ((size_t)1 << lo_bits) - 1;
    const Fe<F>* hi = tab + ((size_t)1 << lo_bits);
    for (size_t i = (size_t)blockIdx.x * FOLD_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * FOLD_BLOCK) out[i] = fe_mul<F>(hi[i >> lo_bits], tab[i & mask]);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static const MlePlan& mle_plan(const R1csShape& sh) {
    std::lock_guard<std::mutex> lk(sh.mle_mu);
    if (sh.mle) return *sh.mle;
    auto plan = std::make_unique<MlePlan>();
    for (int w = 0; w < 3; w++) {
        if (!sh.m[w].nnz) continue;
        std::vector<uint2> ent(sh.m[w].nnz);
        LURK_HIP_CHECK(hipMemcpy(ent.data(), sh.m[w].ent.p, sh.m[w].nnz * sizeof(uint2), hipMemcpyDeviceToHost));
        for (const uint2& e : ent) plan->max_col = std::max<uint64_t>(plan->max_col, e.x);
    }
    build_row_classes(plan->cls, sh, SAT_LANE_MAX, SAT_MID_MAX, true);  // a row with no entry costs nothing
    sh.mle = std::move(plan);
    return *sh.mle;
}

// out3: A~, B~, C~ in Montgomery form (host); synchronises the stream
template <class P>
static void sparse_mle(const R1csShape& sh, const void* d_ex, size_t n_x, const void* d_ey, size_t n_y, Fe<P>* out3, hipStream_t s) {
    const MlePlan& plan = mle_plan(sh);
    LURK_REQUIRE(n_x >= sh.num_cons, "the eq table of the rows is shorter than the shape has rows");
    const size_t nnz = sh.m[0].nnz + sh.m[1].nnz + sh.m[2].nnz;
    LURK_REQUIRE(nnz == 0 || n_y > plan.max_col, "the eq table of the columns does not reach the shape's largest column");
    for (int w = 0; w < 3; w++) out3[w] = fe_zero<P>();
    MleDev d;
    d.s = dev_view(sh);
    d.c = class_view(plan.cls, (int)SAT_GROUP);
    const unsigned total = d.c.wide_blocks + d.c.mid_blocks + d.c.lane_blocks;
    if (!total) return;
    LURK_REQUIRE(d_ex && d_ey, "null eq table");
    ArenaBuf partial(((size_t)3 * total + 3) * 32, s);
    Fe<P>* d_out = (Fe<P>*)partial.p + (size_t)3 * total;
    {
        ProfScope ps("sparse_mle", s);
        hipLaunchKernelGGL((sparse_mle_kernel<P>), dim3(total), dim3(FOLD_BLOCK), 0, s, d, (const Fe<P>*)d_ex, (const Fe<P>*)d_ey, fe_from_u64<P>(1024),
                           (Fe<P>*)partial.p);
        LURK_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((sparse_mle_sum_kernel<P>), dim3(3), dim3(FOLD_BLOCK), 0, s, (const Fe<P>*)partial.p, total, d_out);
        LURK_HIP_CHECK(hipGetLastError());
    }
    LURK_HIP_CHECK(hipMemcpyAsync(out3, d_out, 96, hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
}

// all inverses with one field inversion (every input non-zero)
template <class F>
static std::vector<Fe<F>> batch_invert(const std::vector<Fe<F>>& v) {
    std::vector<Fe<F>> pre(v.size()), out(v.size());
    Fe<F> acc = fe_one<F>();
    for (size_t i = 0; i < v.size(); i++) {
        pre[i] = acc;
        acc = fe_mul<F>(acc, v[i]);
    }
    Fe<F> inv = fe_inv<F>(acc);
    for (size_t i = v.size(); i-- > 0;) {
        out[i] = fe_mul<F>(inv, pre[i]);
        inv = fe_mul<F>(inv, v[i]);
    }
    return out;
}

// the table over `bits` index bits of the challenges r[first .. first + bits): t[i] = prod_j (bit_{bits-1-j}(i) ? r : r^-1)
template <class F>
static void s_table(const std::vector<Fe<F>>& r, const std::vector<Fe<F>>& rinv, int first, int bits, Fe<F>* t) {
    t[0] = fe_one<F>();
    size_t len = 1;
    for (int j = 0; j < bits; j++) {  // every challenge appends one (lower) index bit
        for (size_t i = len; i-- > 0;) {
            const Fe<F> x = t[i];
            t[2 * i] = fe_mul<F>(x, rinv[first + j]);
            t[2 * i + 1] = fe_mul<F>(x, r[first + j]);
        }
        len *= 2;
    }
}

// r, rinv: Montgomery, ell of each; d_out: 2^ell elements.  The tables are staged before the call returns.
template <class F>
static void ipa_s_vector(const std::vector<Fe<F>>& r, const std::vector<Fe<F>>& rinv, void* d_out, hipStream_t s) {
    const int ell = (int)r.size(), hi_bits = ell / 2, lo_bits = ell - hi_bits;
    const size_t n = (size_t)1 << ell, nlo = (size_t)1 << lo_bits, nhi = (size_t)1 << hi_bits;
    std::vector<Fe<F>> tab(nlo + nhi);
    s_table<F>(r, rinv, hi_bits, lo_bits, tab.data());     // the low index bits belong to the last challenges
    s_table<F>(r, rinv, 0, hi_bits, tab.data() + nlo);
    ArenaBuf d_tab((nlo + nhi) * 32, s);
    LURK_HIP_CHECK(hipMemcpyAsync(d_tab.p, tab.data(), (nlo + nhi) * 32, hipMemcpyHostToDevice, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));  // (pageable source: the table leaves this frame)
    ProfScope ps("ipa_s_vector", s);
    const unsigned grid = std::max(1u, std::min(div_up(n, FOLD_BLOCK), grid_cap(8)));
    hipLaunchKernelGGL((ipa_s_vector_kernel<F>), dim3(grid), dim3(FOLD_BLOCK), 0, s, (const Fe<F>*)d_tab.p, lo_bits, n, (Fe<F>*)d_out);
    LURK_HIP_CHECK(hipGetLastError());
}

// ---- host arithmetic of the checks ------------------------------------------------------------------------------------------------
template <class F>
static bool scalars_reduced(const void* p, size_t n) {
    for (size_t i = 0; i < n; i++) {
        uint32_t w[8];
        memcpy(w, (const char*)p + 32 * i, 32);
        if (fe_canonical_ge_mod<F>(w)) return false;
    }
    return true;
}
// a 96-byte Jacobian over the base field B: the identity (z = 0), or reduced coordinates with Y^2 = X^3 + b Z^6 (b = 5 on both Pasta
// curves, 3 on BN254 G1)
template <class B>
static bool point_wellformed(const void* jac96, uint64_t b) {
    Jacobian<B> j;
    memcpy(&j, jac96, 96);
    if (fe_canonical_ge_mod<B>(j.x.l) || fe_canonical_ge_mod<B>(j.y.l) || fe_canonical_ge_mod<B>(j.z.l)) return false;
    if (fe_is_zero<B>(j.z)) return true;
    const Fe<B> z2 = fe_sqr<B>(j.z), z6 = fe_mul<B>(fe_sqr<B>(z2), z2);
    const Fe<B> rhs = fe_add<B>(fe_mul<B>(fe_sqr<B>(j.x), j.x), fe_mul<B>(fe_from_u64<B>(b), z6));
    return fe_eq<B>(fe_sqr<B>(j.y), rhs);
}
static bool point_wellformed(int curve, const void* jac96) {
    if (curve == LURK_CURVE_BN254) return point_wellformed<Bn254Fq>(jac96, 3);
    bool wf = false;
    with_pasta_curve(curve, [&](auto B, auto) { wf = point_wellformed<decltype(B)>(jac96, 5); });
    return wf;
}
static bool points_equal(int curve, const void* a96, const void* b96) {
    uint64_t a[8], b[8];
    nested_ok(lurk_hip_point_to_affine_canonical(curve, a, a96));
    nested_ok(lurk_hip_point_to_affine_canonical(curve, b, b96));
    return memcmp(a, b, 64) == 0;
}
// acc += [k] pt (k Montgomery)
template <class F>
static void point_mul_add(int curve, uint64_t* acc12, const void* pt96, const Fe<F>& k) {
    uint64_t two[24];
    memcpy(two, acc12, 96);
    nested_ok(lurk_hip_point_mul(curve, two + 12, pt96, k.l, 1));
    nested_ok(lurk_hip_point_sum(curve, acc12, two, 2));
}

// SumcheckProof::verify: polys = rounds x (degree + 1) canonical coefficients; false when a round's p(0) + p(1) misses the claim
template <class F>
static bool sumcheck_verify(int degree, size_t rounds, Fe<F> claim, const void* polys, const std::vector<Fe<F>>& r, Fe<F>& final_claim) {
    const int nc = degree + 1;
    bool ok = true;
    for (size_t j = 0; j < rounds; j++) {
        Fe<F> c[4];
        for (int k = 0; k < nc; k++) c[k] = fe_read_canonical<F>((const char*)polys + 32 * (j * nc + k));
        Fe<F> at1 = c[0];
        for (int k = 1; k < nc; k++) at1 = fe_add<F>(at1, c[k]);
        if (!fe_eq<F>(fe_add<F>(c[0], at1), claim)) ok = false;
        Fe<F> v = c[nc - 1];
        for (int k = nc - 2; k >= 0; k--) v = fe_add<F>(fe_mul<F>(v, r[j]), c[k]);
        claim = v;
    }
    final_claim = claim;
    return ok;
}

template <class F>
static Fe<F> eq_at(const std::vector<Fe<F>>& x, const std::vector<Fe<F>>& y) {  // prod (x y + (1 - x)(1 - y)) over the shorter length
    const Fe<F> one = fe_one<F>();
    Fe<F> acc = one;
    for (size_t i = 0; i < x.size() && i < y.size(); i++)
        acc = fe_mul<F>(acc, fe_add<F>(fe_mul<F>(x[i], y[i]), fe_mul<F>(fe_sub<F>(one, x[i]), fe_sub<F>(one, y[i]))));
    return acc;
}
template <class F>
static Fe<F> pad_factor(const Fe<F>* r, size_t count) {  // prod (1 - r_j)
    Fe<F> acc = fe_one<F>();
    for (size_t i = 0; i < count; i++) acc = fe_mul<F>(acc, fe_sub<F>(fe_one<F>(), r[i]));
    return acc;
}
// <[u | X | 0 ...], eq(point)>: entry i of eq(point) is prod_j (bit_{L-1-j}(i) ? point_j : 1 - point_j)
template <class F>
static Fe<F> eval_ux(const std::vector<Fe<F>>& ux, const Fe<F>* point, size_t L) {
    Fe<F> acc = fe_zero<F>();
    for (size_t i = 0; i < ux.size(); i++) {
        if (L < 64 && (i >> L)) break;  // (1 + num_io <= num_vars = 2^L: never taken)
        Fe<F> e = fe_one<F>();
        for (size_t j = 0; j < L; j++) {
            const size_t bit = L - 1 - j;
            e = fe_mul<F>(e, (bit < 64 && ((i >> bit) & 1)) ? point[j] : fe_sub<F>(fe_one<F>(), point[j]));
        }
        acc = fe_add<F>(acc, fe_mul<F>(ux[i], e));
    }
    return acc;
}
template <class F>
static std::vector<Fe<F>> powers_of(const Fe<F>& b, size_t count) {
    std::vector<Fe<F>> v(count);
    Fe<F> acc = fe_one<F>();
    for (size_t k = 0; k < count; k++) {
        v[k] = acc;
        acc = fe_mul<F>(acc, b);
    }
    return v;
}
// replay of a sum-check's rounds over the transcript: every round polynomial absorbed, its challenge squeezed
template <class F>
static std::vector<Fe<F>> replay_rounds(lurk_hip_keccak_transcript* t, int field_id, const void* polys, size_t rounds, int n_scalars) {
    std::vector<Fe<F>> rs(rounds);
    for (size_t j = 0; j < rounds; j++) {
        nested_ok(lurk_hip_keccak_transcript_absorb_scalars(t, splabel::POLY, strlen(splabel::POLY), (const char*)polys + 32 * j * n_scalars, (size_t)n_scalars));
        rs[j] = sp_squeeze<F>(t, splabel::CHALLENGE, field_id);
    }
    return rs;
}

// InnerProductArgument::verify.  p96: the commitment side (modified: the L / R terms are added to it); b: d_b, or eq(eq_point) in
// closed form.  Returns the failed check (0 = accepted).
template <class F>
static int ipa_verify(lurk_hip_msm_ctx* key, int curve, int field_id, size_t n, uint64_t* p96, const void* ck_c96, const void* d_b,
                      const std::vector<Fe<F>>* eq_point, const void* l96, const void* r96, const void* a_hat32, lurk_hip_ipa_challenge_fn challenge, void* user,
                      hipStream_t s) {
    const int ell = sp_log2(n);
    if (!scalars_reduced<F>(a_hat32, 1)) return LURK_VERIFY_MALFORMED;
    for (int j = 0; j < ell; j++)
        if (!point_wellformed(curve, (const char*)l96 + 96 * j) || !point_wellformed(curve, (const char*)r96 + 96 * j)) return LURK_VERIFY_MALFORMED;
    if (!point_wellformed(curve, p96)) return LURK_VERIFY_MALFORMED;
    std::vector<Fe<F>> r(ell);
    for (int j = 0; j < ell; j++) {
        uint64_t rc[4] = {0, 0, 0, 0};
        if (challenge(user, j, (const char*)l96 + 96 * j, (const char*)r96 + 96 * j, rc) != 0)
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "lurk_hip_ipa_verify_dev: the challenge callback failed"};
        if (!scalars_reduced<F>(rc, 1) || !(rc[0] | rc[1] | rc[2] | rc[3])) return LURK_VERIFY_MALFORMED;  // a zero challenge has no inverse
        r[j] = fe_read_canonical<F>(rc);
    }
    const std::vector<Fe<F>> rinv = batch_invert<F>(r);
    for (int j = 0; j < ell; j++) {
        point_mul_add<F>(curve, p96, (const char*)l96 + 96 * j, fe_sqr<F>(r[j]));
        point_mul_add<F>(curve, p96, (const char*)r96 + 96 * j, fe_sqr<F>(rinv[j]));
    }
    ArenaBuf d_s(n * 32, s);
    ipa_s_vector<F>(r, rinv, d_s.p, s);
    Fe<F> b_hat;
    if (d_b) {
        nested_ok(lurk_hip_inner_product_dev(field_id, d_s.p, d_b, n, b_hat.l, (void*)s));
    } else {
        b_hat = fe_one<F>();
        for (int j = 0; j < ell; j++) {
            const Fe<F>& z = (*eq_point)[j];
            b_hat = fe_mul<F>(b_hat, fe_add<F>(fe_mul<F>(rinv[j], fe_sub<F>(fe_one<F>(), z)), fe_mul<F>(r[j], z)));
        }
    }
    uint64_t ck_hat[12];
    nested_ok(lurk_hip_msm_ctx_run_dev(key, ck_hat, d_s.p, n, 1, (void*)s));  // (synchronises: the result is on the host)
    const Fe<F> a_hat = fe_read_canonical<F>(a_hat32);
    uint64_t rhs[12];
    nested_ok(lurk_hip_point_mul(curve, rhs, ck_hat, a_hat.l, 1));
    point_mul_add<F>(curve, rhs, ck_c96, fe_mul<F>(a_hat, b_hat));
    return points_equal(curve, p96, rhs) ? LURK_VERIFY_ACCEPTED : LURK_VERIFY_OPENING;
}

// the opening of the joint commitment: comm_joint + [c] ck_c' against the proof's L, R, a_hat, the rounds over the transcript
template <class F>
static int open_joint(SpTranscript& tr, lurk_hip_msm_ctx* key, int curve, int field_id, size_t N, uint64_t* comm_joint, const Fe<F>& c, const void* ck_c_jac96,
                      const std::vector<Fe<F>>& r_z, const void* ipa_l, const void* ipa_r, const void* ipa_a, hipStream_t s) {
    const Fe<F> r0 = sp_squeeze<F>(tr.t, splabel::IPA_R0, field_id);
    uint64_t ck_c_scaled[12];
    nested_ok(lurk_hip_point_mul(curve, ck_c_scaled, ck_c_jac96, r0.l, 1));
    point_mul_add<F>(curve, comm_joint, ck_c_scaled, c);
    std::vector<uint64_t> keep;
    lurk_hip_keccak_round_binding b = sp_round_binding(tr.t, field_id, curve, keep, sp_log2(N), splabel::IPA_L, splabel::IPA_R, splabel::IPA_CHALLENGE, 0);
    return ipa_verify<F>(key, curve, field_id, N, comm_joint, ck_c_scaled, nullptr, &r_z, ipa_l, ipa_r, ipa_a, lurk_hip_keccak_ipa_challenge, &b, s);
}

template <class F>
static std::vector<Fe<F>> load_scalars(const void* p, size_t n) {
    std::vector<Fe<F>> v(n);
    for (size_t i = 0; i < n; i++) v[i] = fe_read_canonical<F>((const char*)p + 32 * i);
    return v;
}

// What a verifier holds when the transcript has given gamma: the point r_z and the claimed evaluations of the polynomials there.  The
// two openings (the inner-product argument on the Pasta curves, HyperKZG on BN254 G1) continue from here over the same transcript.
template <class F>
struct SpFront {
    SpTranscript tr;
    Fe<F> gamma;
    std::vector<Fe<F>> r_z, eb;
};

// oracle/spartan_fast.py: verify, checks 1 to 4 (the opening's own fields are checked for form by the caller, before this).  Returns
// the failed check.
template <class F, class Proof>
static int spartan_verify_front(int curve, int field_id, const lurk_hip_r1cs* shape, size_t nc, size_t nv, size_t nio, const void* x_canonical,
                                const void* u_canonical, const void* comm_w_jac96, const void* comm_e_jac96, const void* label, size_t label_len, const Proof* pf,
                                SpFront<F>& fr, hipStream_t s) {
    const int ell_x = sp_log2(nc), ell_y = sp_log2(nv) + 1;
    const size_t N = nc > nv ? nc : nv;
    const int ell = sp_log2(N);
    SpTranscript& tr = fr.tr;
    // ---- check 1: nothing malformed enters the arithmetic
    if (!scalars_reduced<F>(u_canonical, 1) || !scalars_reduced<F>(x_canonical, nio) || !scalars_reduced<F>(pf->polys_outer, (size_t)ell_x * 4) ||
        !scalars_reduced<F>(pf->claims_outer, 3) || !scalars_reduced<F>(pf->eval_e, 1) || !scalars_reduced<F>(pf->polys_inner, (size_t)ell_y * 3) ||
        !scalars_reduced<F>(pf->eval_w, 1) || !scalars_reduced<F>(pf->polys_batch, (size_t)ell * 3) || !scalars_reduced<F>(pf->evals_batch, 2))
        return LURK_VERIFY_MALFORMED;
    if (!point_wellformed(curve, comm_w_jac96) || !point_wellformed(curve, comm_e_jac96)) return LURK_VERIFY_MALFORMED;
    stream_pool_retain();
    std::vector<Fe<F>> ux;
    sp_prologue<F>(tr, curve, label, label_len, comm_w_jac96, comm_e_jac96, u_canonical, x_canonical, nio, ux);
    std::vector<Fe<F>> tau(ell_x);
    for (int j = 0; j < ell_x; j++) tau[j] = sp_squeeze<F>(tr.t, splabel::TAU, field_id);
    // ---- check 2: the outer sum-check
    const std::vector<Fe<F>> r_x = replay_rounds<F>(tr.t, field_id, pf->polys_outer, ell_x, 4);
    Fe<F> fin;
    bool ok = sumcheck_verify<F>(3, ell_x, fe_zero<F>(), pf->polys_outer, r_x, fin);
    const std::vector<Fe<F>> co = load_scalars<F>(pf->claims_outer, 3);
    const Fe<F> eval_e = fe_read_canonical<F>(pf->eval_e);
    {
        const Fe<F> inner = fe_sub<F>(fe_sub<F>(fe_mul<F>(co[0], co[1]), fe_mul<F>(ux[0], co[2])), eval_e);
        if (!ok || !fe_eq<F>(fin, fe_mul<F>(eq_at<F>(tau, r_x), inner))) return LURK_VERIFY_OUTER;
    }
    sp_absorb<F>(tr.t, splabel::CLAIMS_OUTER, {co[0], co[1], co[2], eval_e});
    const Fe<F> r = sp_squeeze<F>(tr.t, splabel::R, field_id), r2 = fe_mul<F>(r, r);
    const Fe<F> claim_inner = fe_add<F>(fe_add<F>(co[0], fe_mul<F>(r, co[1])), fe_mul<F>(r2, co[2]));
    // ---- check 3: the inner sum-check against the matrices at (r_x, r_y)
    const std::vector<Fe<F>> r_y = replay_rounds<F>(tr.t, field_id, pf->polys_inner, ell_y, 3);
    ok = sumcheck_verify<F>(2, ell_y, claim_inner, pf->polys_inner, r_y, fin);
    const Fe<F> eval_w = fe_read_canonical<F>(pf->eval_w);
    {
        Fe<F> abc3[3];
        {
            SpScratch eq_rx(nc * 32, s), eq_ry(2 * nv * 32, s);
            sp_eq<F>(field_id, r_x, eq_rx.p, s);
            sp_eq<F>(field_id, r_y, eq_ry.p, s);
            sparse_mle<F>(shape->sh, eq_rx.p, nc, eq_ry.p, 2 * nv, abc3, s);
        }
        const Fe<F> abc = fe_add<F>(fe_add<F>(abc3[0], fe_mul<F>(r, abc3[1])), fe_mul<F>(r2, abc3[2]));
        const Fe<F> eval_x = eval_ux<F>(ux, r_y.data() + 1, (size_t)ell_y - 1);
        const Fe<F> eval_z = fe_add<F>(fe_mul<F>(fe_sub<F>(fe_one<F>(), r_y[0]), eval_w), fe_mul<F>(r_y[0], eval_x));
        if (!ok || !fe_eq<F>(fin, fe_mul<F>(abc, eval_z))) return LURK_VERIFY_INNER;
    }
    sp_absorb<F>(tr.t, splabel::EVAL_W, {eval_w});
    // ---- check 4: the two evaluation claims at one point
    std::vector<Fe<F>> x1((size_t)ell - (ell_y - 1), fe_zero<F>()), x2((size_t)ell - ell_x, fe_zero<F>());
    x1.insert(x1.end(), r_y.begin() + 1, r_y.end());
    x2.insert(x2.end(), r_x.begin(), r_x.end());
    const Fe<F> rho = sp_squeeze<F>(tr.t, splabel::RHO, field_id);
    fr.r_z = replay_rounds<F>(tr.t, field_id, pf->polys_batch, ell, 3);
    ok = sumcheck_verify<F>(2, ell, fe_add<F>(eval_w, fe_mul<F>(rho, eval_e)), pf->polys_batch, fr.r_z, fin);
    fr.eb = load_scalars<F>(pf->evals_batch, 2);
    if (!ok || !fe_eq<F>(fin, fe_add<F>(fe_mul<F>(eq_at<F>(x1, fr.r_z), fr.eb[0]), fe_mul<F>(rho, fe_mul<F>(eq_at<F>(x2, fr.r_z), fr.eb[1]))))) return LURK_VERIFY_BATCH;
    sp_absorb<F>(tr.t, splabel::EVALS_BATCH, {fr.eb[0], fr.eb[1]});
    fr.gamma = sp_squeeze<F>(tr.t, splabel::GAMMA, field_id);
    return LURK_VERIFY_ACCEPTED;
}

// the Pasta verifier: the front, then check 5, the opening of comm_W + gamma comm_E at r_z by the inner-product argument
template <class F>
static int spartan_verify(int curve, int field_id, const lurk_hip_r1cs* shape, size_t nc, size_t nv, size_t nio, lurk_hip_msm_ctx* key, const void* ck_c_jac96,
                          const void* x_canonical, const void* u_canonical, const void* comm_w_jac96, const void* comm_e_jac96, const void* label, size_t label_len,
                          const lurk_hip_spartan_proof* pf, hipStream_t s) {
    const size_t N = nc > nv ? nc : nv;
    if (!scalars_reduced<F>(pf->ipa_a, 1)) return LURK_VERIFY_MALFORMED;
    for (int j = 0; j < sp_log2(N); j++)
        if (!point_wellformed(curve, (const char*)pf->ipa_l + 96 * j) || !point_wellformed(curve, (const char*)pf->ipa_r + 96 * j)) return LURK_VERIFY_MALFORMED;
    SpFront<F> fr;
    const int failed = spartan_verify_front<F>(curve, field_id, shape, nc, nv, nio, x_canonical, u_canonical, comm_w_jac96, comm_e_jac96, label, label_len, pf, fr, s);
    if (failed != LURK_VERIFY_ACCEPTED) return failed;
    uint64_t comm_joint[12];
    memcpy(comm_joint, comm_w_jac96, 96);
    point_mul_add<F>(curve, comm_joint, comm_e_jac96, fr.gamma);
    const Fe<F> c = fe_add<F>(fr.eb[0], fe_mul<F>(fr.gamma, fr.eb[1]));
    return open_joint<F>(fr.tr, key, curve, field_id, N, comm_joint, c, ck_c_jac96, fr.r_z, pf->ipa_l, pf->ipa_r, pf->ipa_a, s);
}

// The HyperKZG tail shared by the two BN254 verifiers: C and y are the caller's combinations; the three challenges come off the transcript
// in the prover's order (sp_kzg_stage), then lurk_hip_hyperkzg_pairing_inputs runs the scalar checks and forms L and R.
static bool kzg_fields_wellformed(int ell, const void* kzg_com, const void* kzg_v, const void* kzg_w) {
    if (!scalars_reduced<Bn254Fr>(kzg_v, (size_t)3 * ell)) return false;
    for (int i = 0; i + 1 < ell; i++)
        if (!point_wellformed(LURK_CURVE_BN254, (const char*)kzg_com + 96 * i)) return false;
    for (int t = 0; t < 3; t++)
        if (!point_wellformed(LURK_CURVE_BN254, (const char*)kzg_w + 96 * t)) return false;
    return true;
}
static int kzg_open_joint(SpFront<Bn254Fr>& fr, int ell, const uint64_t* comm_joint, const Fe<Bn254Fr>& y, const void* kzg_com, const void* kzg_v, const void* kzg_w,
                          void* out_l, void* out_r) {
    using F = Bn254Fr;
    const Fe<F> r = sp_kzg_stage<F>(fr.tr.t, 0, kzg_com, (size_t)(ell - 1));
    if (fe_is_zero<F>(r)) return LURK_VERIFY_MALFORMED;
    const Fe<F> q = sp_kzg_stage<F>(fr.tr.t, 1, kzg_v, (size_t)3 * ell), d = sp_kzg_stage<F>(fr.tr.t, 2, kzg_w, 3);
    std::vector<uint64_t> x((size_t)4 * ell);
    for (int i = 0; i < ell; i++) fe_write_canonical<F>(x.data() + 4 * i, fr.r_z[i]);
    uint64_t yc[4], rc[4], qc[4], dc[4];
    fe_write_canonical<F>(yc, y);
    fe_write_canonical<F>(rc, r);
    fe_write_canonical<F>(qc, q);
    fe_write_canonical<F>(dc, d);
    int accepted = 0, hk_failed = 0;
    nested_ok(lurk_hip_hyperkzg_pairing_inputs(LURK_CURVE_BN254, ell, comm_joint, x.data(), yc, ell > 1 ? kzg_com : (const void*)comm_joint, kzg_v, kzg_w, rc, qc, dc,
                                               out_l, out_r, &accepted, &hk_failed));
    if (accepted) return LURK_VERIFY_ACCEPTED;
    return hk_failed == LURK_HYPERKZG_MALFORMED ? LURK_VERIFY_MALFORMED : LURK_VERIFY_OPENING;
}

// tests/spartan_kzg_ref.py: verify.  L and R are the identity unless the proof is accepted so far.
static int spartan_kzg_verify(const lurk_hip_r1cs* shape, size_t nc, size_t nv, size_t nio, const void* x_canonical, const void* u_canonical, const void* comm_w_jac96,
                              const void* comm_e_jac96, const void* label, size_t label_len, const lurk_hip_spartan_kzg_proof* pf, void* out_l, void* out_r,
                              hipStream_t s) {
    using F = Bn254Fr;
    const int curve = LURK_CURVE_BN254, ell = sp_log2(nc > nv ? nc : nv);
    if (!kzg_fields_wellformed(ell, pf->kzg_com, pf->kzg_v, pf->kzg_w)) return LURK_VERIFY_MALFORMED;
    SpFront<F> fr;
    const int failed = spartan_verify_front<F>(curve, F::ID, shape, nc, nv, nio, x_canonical, u_canonical, comm_w_jac96, comm_e_jac96, label, label_len, pf, fr, s);
    if (failed != LURK_VERIFY_ACCEPTED) return failed;
    uint64_t comm_joint[12];
    memcpy(comm_joint, comm_w_jac96, 96);
    point_mul_add<F>(curve, comm_joint, comm_e_jac96, fr.gamma);
    const Fe<F> y = fe_add<F>(fr.eb[0], fe_mul<F>(fr.gamma, fr.eb[1]));
    return kzg_open_joint(fr, ell, comm_joint, y, pf->kzg_com, pf->kzg_v, pf->kzg_w, out_l, out_r);
}

// oracle/spartan_fast.py: verify_batched, checks 1 to 4 (as spartan_verify_front)
template <class F, class Proof>
static int spartan_verify_batch_front(int curve, int field_id, const lurk_hip_spartan_instance* inst, size_t n, const void* label, size_t label_len, const Proof* pf,
                                      SpFront<F>& fr, hipStream_t s) {
    size_t max_nc = 0, max_nv = 0;
    for (size_t i = 0; i < n; i++) {
        max_nc = std::max(max_nc, inst[i].num_cons);
        max_nv = std::max(max_nv, inst[i].num_vars);
    }
    const int ell_x = sp_log2(max_nc), ell_y = sp_log2(max_nv) + 1;
    const size_t N = std::max(max_nc, max_nv), LX = (size_t)1 << ell_x, LY = (size_t)1 << ell_y;
    const int ell = sp_log2(N);
    // ---- check 1
    for (size_t i = 0; i < n; i++) {
        if (!scalars_reduced<F>(inst[i].u32_canonical, 1) || !scalars_reduced<F>(inst[i].x32_canonical, inst[i].num_io)) return LURK_VERIFY_MALFORMED;
        if (!point_wellformed(curve, inst[i].comm_w_jacobian96) || !point_wellformed(curve, inst[i].comm_e_jacobian96)) return LURK_VERIFY_MALFORMED;
    }
    if (!scalars_reduced<F>(pf->polys_outer, (size_t)ell_x * 4) || !scalars_reduced<F>(pf->claims_outer, 3 * n) || !scalars_reduced<F>(pf->evals_e, n) ||
        !scalars_reduced<F>(pf->polys_inner, (size_t)ell_y * 3) || !scalars_reduced<F>(pf->evals_w, n) || !scalars_reduced<F>(pf->polys_batch, (size_t)ell * 3) ||
        !scalars_reduced<F>(pf->evals_batch, 2 * n))
        return LURK_VERIFY_MALFORMED;
    stream_pool_retain();
    SpTranscript& tr = fr.tr;
    std::vector<std::vector<Fe<F>>> ux;
    sp_prologue_batch<F>(tr, curve, label, label_len, inst, n, ux);
    std::vector<Fe<F>> tau(ell_x);
    for (int j = 0; j < ell_x; j++) tau[j] = sp_squeeze<F>(tr.t, splabel::TAU, field_id);
    const Fe<F> rho_o = sp_squeeze<F>(tr.t, splabel::RHO_OUTER, field_id);
    // ---- check 2
    const std::vector<Fe<F>> r_x = replay_rounds<F>(tr.t, field_id, pf->polys_outer, ell_x, 4);
    Fe<F> fin;
    bool ok = sumcheck_verify<F>(3, ell_x, fe_zero<F>(), pf->polys_outer, r_x, fin);
    const std::vector<Fe<F>> co = load_scalars<F>(pf->claims_outer, 3 * n), ev_e = load_scalars<F>(pf->evals_e, n), ev_w = load_scalars<F>(pf->evals_w, n);
    {
        const Fe<F> tau_rx = eq_at<F>(tau, r_x);
        const std::vector<Fe<F>> pw = powers_of<F>(rho_o, n);
        Fe<F> want = fe_zero<F>();
        for (size_t i = 0; i < n; i++) {
            const int px = ell_x - sp_log2(inst[i].num_cons);
            const Fe<F> e_pad = fe_mul<F>(pad_factor<F>(r_x.data(), px), ev_e[i]);
            const Fe<F> inner = fe_sub<F>(fe_sub<F>(fe_mul<F>(co[3 * i], co[3 * i + 1]), fe_mul<F>(ux[i][0], co[3 * i + 2])), e_pad);
            want = fe_add<F>(want, fe_mul<F>(fe_mul<F>(pw[i], tau_rx), inner));
        }
        if (!ok || !fe_eq<F>(fin, want)) return LURK_VERIFY_OUTER;
    }
    {
        std::vector<Fe<F>> flat(co);
        flat.insert(flat.end(), ev_e.begin(), ev_e.end());
        sp_absorb<F>(tr.t, splabel::CLAIMS_OUTER, flat);
    }
    const Fe<F> r = sp_squeeze<F>(tr.t, splabel::R, field_id), r2 = fe_mul<F>(r, r);
    const Fe<F> rho_i = sp_squeeze<F>(tr.t, splabel::RHO_INNER, field_id);
    const std::vector<Fe<F>> pw_i = powers_of<F>(rho_i, n);
    Fe<F> claim_inner = fe_zero<F>();
    for (size_t i = 0; i < n; i++)
        claim_inner = fe_add<F>(claim_inner, fe_mul<F>(pw_i[i], fe_add<F>(fe_add<F>(co[3 * i], fe_mul<F>(r, co[3 * i + 1])), fe_mul<F>(r2, co[3 * i + 2]))));
    // ---- check 3: the bound tables are abc_i'(r_y) z_i'(r_y), both zero-padded: the truncated eq tables carry the padding factors of r_x and
    // r_y into the sparse evaluation, z_i' = pad_y z_i(sub-point) carries pad_y once more
    const std::vector<Fe<F>> r_y = replay_rounds<F>(tr.t, field_id, pf->polys_inner, ell_y, 3);
    ok = sumcheck_verify<F>(2, ell_y, claim_inner, pf->polys_inner, r_y, fin);
    {
        SpScratch eq_rx(LX * 32, s), eq_ry(LY * 32, s);
        sp_eq<F>(field_id, r_x, eq_rx.p, s);
        sp_eq<F>(field_id, r_y, eq_ry.p, s);
        Fe<F> want = fe_zero<F>();
        for (size_t i = 0; i < n; i++) {
            const size_t nc = inst[i].num_cons, nv = inst[i].num_vars;
            const int py = ell_y - (sp_log2(nv) + 1);
            Fe<F> abc3[3];
            sparse_mle<F>(inst[i].shape->sh, eq_rx.p, nc, eq_ry.p, 2 * nv, abc3, s);
            const Fe<F> abc = fe_add<F>(fe_add<F>(abc3[0], fe_mul<F>(r, abc3[1])), fe_mul<F>(r2, abc3[2]));
            const Fe<F> eval_x = eval_ux<F>(ux[i], r_y.data() + py + 1, (size_t)sp_log2(nv));
            const Fe<F>& t = r_y[py];
            const Fe<F> eval_z = fe_add<F>(fe_mul<F>(fe_sub<F>(fe_one<F>(), t), ev_w[i]), fe_mul<F>(t, eval_x));
            want = fe_add<F>(want, fe_mul<F>(fe_mul<F>(pw_i[i], abc), fe_mul<F>(pad_factor<F>(r_y.data(), py), eval_z)));
        }
        if (!ok || !fe_eq<F>(fin, want)) return LURK_VERIFY_INNER;
    }
    sp_absorb<F>(tr.t, splabel::EVALS_W, ev_w);
    // ---- check 4
    std::vector<std::vector<Fe<F>>> points(2 * n);
    std::vector<Fe<F>> claims(2 * n);
    for (size_t i = 0; i < n; i++) {
        const size_t nc = inst[i].num_cons, nv = inst[i].num_vars;
        const int py = ell_y - (sp_log2(nv) + 1), px = ell_x - sp_log2(nc);
        points[2 * i].assign((size_t)ell - sp_log2(nv), fe_zero<F>());
        points[2 * i].insert(points[2 * i].end(), r_y.begin() + py + 1, r_y.end());
        points[2 * i + 1].assign((size_t)ell - sp_log2(nc), fe_zero<F>());
        points[2 * i + 1].insert(points[2 * i + 1].end(), r_x.begin() + px, r_x.end());
        claims[2 * i] = ev_w[i];
        claims[2 * i + 1] = ev_e[i];
    }
    const Fe<F> rho = sp_squeeze<F>(tr.t, splabel::RHO, field_id);
    const std::vector<Fe<F>> pw = powers_of<F>(rho, 2 * n);
    Fe<F> claim = fe_zero<F>();
    for (size_t k = 0; k < 2 * n; k++) claim = fe_add<F>(claim, fe_mul<F>(pw[k], claims[k]));
    fr.r_z = replay_rounds<F>(tr.t, field_id, pf->polys_batch, ell, 3);
    ok = sumcheck_verify<F>(2, ell, claim, pf->polys_batch, fr.r_z, fin);
    fr.eb = load_scalars<F>(pf->evals_batch, 2 * n);
    {
        Fe<F> want = fe_zero<F>();
        for (size_t k = 0; k < 2 * n; k++) want = fe_add<F>(want, fe_mul<F>(fe_mul<F>(pw[k], eq_at<F>(points[k], fr.r_z)), fr.eb[k]));
        if (!ok || !fe_eq<F>(fin, want)) return LURK_VERIFY_BATCH;
    }
    sp_absorb<F>(tr.t, splabel::EVALS_BATCH, fr.eb);
    fr.gamma = sp_squeeze<F>(tr.t, splabel::GAMMA, field_id);
    return LURK_VERIFY_ACCEPTED;
}

// check 5 of a batch, the statement's side: comm_joint = sum_k gamma^k comm_k over (comm_W_0, comm_E_0, comm_W_1, ...), c = sum_k gamma^k evals_batch[k]
template <class F>
static Fe<F> batch_joint(int curve, const lurk_hip_spartan_instance* inst, size_t n, const SpFront<F>& fr, uint64_t* comm_joint) {
    const std::vector<Fe<F>> pg = powers_of<F>(fr.gamma, 2 * n);
    memcpy(comm_joint, inst[0].comm_w_jacobian96, 96);
    Fe<F> c = fr.eb[0];
    for (size_t k = 1; k < 2 * n; k++) {
        point_mul_add<F>(curve, comm_joint, (k & 1) ? inst[k / 2].comm_e_jacobian96 : inst[k / 2].comm_w_jacobian96, pg[k]);
        c = fe_add<F>(c, fe_mul<F>(pg[k], fr.eb[k]));
    }
    return c;
}
static size_t batch_n(const lurk_hip_spartan_instance* inst, size_t n) {
    size_t N = 0;
    for (size_t i = 0; i < n; i++) N = std::max(N, std::max(inst[i].num_cons, inst[i].num_vars));
    return N;
}

template <class F>
static int spartan_verify_batch(int curve, int field_id, const lurk_hip_spartan_instance* inst, size_t n, lurk_hip_msm_ctx* key, const void* ck_c_jac96,
                                const void* label, size_t label_len, const lurk_hip_spartan_batch_proof* pf, hipStream_t s) {
    const size_t N = batch_n(inst, n);
    if (!scalars_reduced<F>(pf->ipa_a, 1)) return LURK_VERIFY_MALFORMED;
    for (int j = 0; j < sp_log2(N); j++)
        if (!point_wellformed(curve, (const char*)pf->ipa_l + 96 * j) || !point_wellformed(curve, (const char*)pf->ipa_r + 96 * j)) return LURK_VERIFY_MALFORMED;
    SpFront<F> fr;
    const int failed = spartan_verify_batch_front<F>(curve, field_id, inst, n, label, label_len, pf, fr, s);
    if (failed != LURK_VERIFY_ACCEPTED) return failed;
    uint64_t comm_joint[12];
    const Fe<F> c = batch_joint<F>(curve, inst, n, fr, comm_joint);
    return open_joint<F>(fr.tr, key, curve, field_id, N, comm_joint, c, ck_c_jac96, fr.r_z, pf->ipa_l, pf->ipa_r, pf->ipa_a, s);
}

// tests/spartan_kzg_ref.py: verify_batched
static int spartan_kzg_verify_batch(const lurk_hip_spartan_instance* inst, size_t n, const void* label, size_t label_len, const lurk_hip_spartan_kzg_batch_proof* pf,
                                    void* out_l, void* out_r, hipStream_t s) {
    using F = Bn254Fr;
    const int curve = LURK_CURVE_BN254, ell = sp_log2(batch_n(inst, n));
    if (!kzg_fields_wellformed(ell, pf->kzg_com, pf->kzg_v, pf->kzg_w)) return LURK_VERIFY_MALFORMED;
    SpFront<F> fr;
    const int failed = spartan_verify_batch_front<F>(curve, F::ID, inst, n, label, label_len, pf, fr, s);
    if (failed != LURK_VERIFY_ACCEPTED) return failed;
    uint64_t comm_joint[12];
    const Fe<F> y = batch_joint<F>(curve, inst, n, fr, comm_joint);
    return kzg_open_joint(fr, ell, comm_joint, y, pf->kzg_com, pf->kzg_v, pf->kzg_w, out_l, out_r);
}

struct KeyInfo {
    int curve = 0, field_id = 0, device = 0;
    size_t points = 0;
};
static KeyInfo key_info(const lurk_hip_msm_ctx* key) {
    KeyInfo k;
    int bits = 0;
    if (lurk_hip_msm_ctx_info(key, &k.curve, &k.points, &bits, nullptr) != 0 || lurk_hip_msm_ctx_device(key, &k.device) != 0)
        throw HipFailure{LURK_HIP_ERR_INVALID_ARG, lurk_hip_last_error()};
    require_pasta_curve(k.curve, "the verifiers of the opening argument and of the compressing SNARK");
    k.field_id = k.curve == LURK_CURVE_PALLAS ? LURK_FIELD_PALLAS_FQ : LURK_FIELD_PALLAS_FP;
    return k;
}
static bool pow2_at_least_2(size_t v) { return v >= 2 && (v & (v - 1)) == 0; }
static void check_instance_shape(const lurk_hip_r1cs* shape, size_t nc, size_t nv, size_t nio, const KeyInfo& k) {
    LURK_REQUIRE(pow2_at_least_2(nc) && pow2_at_least_2(nv), "num_cons and num_vars must be powers of two >= 2");
    LURK_REQUIRE(1 + nio <= nv, "the public IO does not fit the second half of z");
    LURK_REQUIRE(k.points >= (nc > nv ? nc : nv), "the key has fewer points than the padded polynomials have elements");
    int f = -1;
    size_t c = 0, v = 0, io = 0;
    if (lurk_hip_r1cs_dims(shape, &f, &c, &v, &io) != 0) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, lurk_hip_last_error()};
    LURK_REQUIRE(c == nc && v == nv && io == nio, "shape: its (num_cons, num_vars, num_io) differ from the arguments");
    LURK_REQUIRE(f == k.field_id, "the shape is not over the scalar field of the key's curve");
    LURK_REQUIRE(shape->sh.device == k.device, "the shape and the key are resident on different devices");
}

// the BN254 verifiers take no key: the device is the shape's, the field must be BN254's scalar field
static void check_kzg_instance_shape(const lurk_hip_r1cs* shape, size_t nc, size_t nv, size_t nio, int device) {
    LURK_REQUIRE(pow2_at_least_2(nc) && pow2_at_least_2(nv), "num_cons and num_vars must be powers of two >= 2");
    LURK_REQUIRE(1 + nio <= nv, "the public IO does not fit the second half of z");
    int f = -1;
    size_t c = 0, v = 0, io = 0;
    if (lurk_hip_r1cs_dims(shape, &f, &c, &v, &io) != 0) throw HipFailure{LURK_HIP_ERR_INVALID_ARG, lurk_hip_last_error()};
    LURK_REQUIRE(c == nc && v == nv && io == nio, "shape: its (num_cons, num_vars, num_io) differ from the arguments");
    LURK_REQUIRE(f == LURK_FIELD_BN254_FR, "the shape is not over LURK_FIELD_BN254_FR, the scalar field of BN254 G1");
    LURK_REQUIRE(shape->sh.device == device, "the shapes are resident on different devices");
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_r1cs_sparse_mle_dev(const lurk_hip_r1cs* shape, const void* d_eq_x, size_t n_x, const void* d_eq_y, size_t n_y, void* out_abc96_mont,
                                 void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && out_abc96_mont, "null argument");
        const R1csShape& sh = shape->sh;
        DeviceGuard dg(sh.device);
        alignas(16) uint64_t out[12];
        with_field(sh.field_id, [&](auto F) { sparse_mle<decltype(F)>(sh, d_eq_x, n_x, d_eq_y, n_y, (Fe<decltype(F)>*)out, (hipStream_t)stream); });
        memcpy(out_abc96_mont, out, 96);
    });
}

int lurk_hip_ipa_s_vector_dev(int field_id, const void* challenges32_canonical, int ell, void* d_out32_mont, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        LURK_REQUIRE(ell >= 0 && ell <= 30, "ell out of range (0 .. 30)");
        LURK_REQUIRE(d_out32_mont && (ell == 0 || challenges32_canonical), "null argument");
        with_field(field_id, [&](auto tag) {
            using F = decltype(tag);
            LURK_REQUIRE(scalars_reduced<F>(challenges32_canonical, (size_t)ell), "a challenge is not reduced modulo the field order");
            std::vector<Fe<F>> r = load_scalars<F>(challenges32_canonical, (size_t)ell);
            for (const Fe<F>& x : r) LURK_REQUIRE(!fe_is_zero<F>(x), "a zero challenge has no inverse");
            ipa_s_vector<F>(r, batch_invert<F>(r), d_out32_mont, (hipStream_t)stream);
        });
    });
}

int lurk_hip_sumcheck_verify(int field_id, int degree, size_t rounds, const void* claim32_canonical, const void* polys, const void* challenges32_canonical,
                             void* out_final32_canonical, int* ok) {
    return host_guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        LURK_REQUIRE(degree == 2 || degree == 3, "degree must be 2 or 3");
        LURK_REQUIRE(claim32_canonical && out_final32_canonical && ok && (rounds == 0 || (polys && challenges32_canonical)), "null argument");
        with_field(field_id, [&](auto tag) {
            using F = decltype(tag);
            *ok = 0;
            memset(out_final32_canonical, 0, 32);
            if (!scalars_reduced<F>(claim32_canonical, 1) || !scalars_reduced<F>(polys, rounds * (degree + 1)) || !scalars_reduced<F>(challenges32_canonical, rounds))
                return;
            Fe<F> fin;
            const bool good = sumcheck_verify<F>(degree, rounds, fe_read_canonical<F>(claim32_canonical), polys, load_scalars<F>(challenges32_canonical, rounds), fin);
            if (!good) return;
            fe_write_canonical<F>(out_final32_canonical, fin);
            *ok = 1;
        });
    });
}

int lurk_hip_ipa_verify_dev(lurk_hip_msm_ctx* key, size_t n, const void* p_jacobian96, const void* ck_c_jacobian96, const void* d_b32_mont,
                            const void* eq_point32_canonical, const void* l_jacobian96, const void* r_jacobian96, const void* a_hat32,
                            lurk_hip_ipa_challenge_fn challenge, void* user, int* accepted, int* failed_check, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(key && p_jacobian96 && ck_c_jacobian96 && a_hat32 && challenge && accepted, "null argument");
        LURK_REQUIRE(n >= 1 && (n & (n - 1)) == 0, "n must be a power of two");
        LURK_REQUIRE(n == 1 || (l_jacobian96 && r_jacobian96), "null L / R");
        LURK_REQUIRE(d_b32_mont || n == 1 || eq_point32_canonical, "neither b nor the point of eq");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_VERIFY_MALFORMED;
        const KeyInfo k = key_info(key);
        LURK_REQUIRE(n <= k.points, "the key has fewer points than n");
        DeviceGuard dg(k.device);
        stream_pool_retain();
        uint64_t p[12];
        memcpy(p, p_jacobian96, 96);
        int failed = LURK_VERIFY_MALFORMED;
        with_pasta_curve(k.curve, [&](auto, auto SF) {
            using F = decltype(SF);
            std::vector<Fe<F>> z;
            if (!d_b32_mont) {
                if (!scalars_reduced<F>(eq_point32_canonical, (size_t)sp_log2(n))) return;
                z = load_scalars<F>(eq_point32_canonical, (size_t)sp_log2(n));
            }
            failed = ipa_verify<F>(key, k.curve, k.field_id, n, p, ck_c_jacobian96, d_b32_mont, &z, l_jacobian96, r_jacobian96, a_hat32, challenge, user,
                                   (hipStream_t)stream);
        });
        *accepted = failed == LURK_VERIFY_ACCEPTED;
        if (failed_check) *failed_check = failed;
    });
}

int lurk_hip_spartan_verify_dev(const lurk_hip_r1cs* shape, size_t num_cons, size_t num_vars, size_t num_io, lurk_hip_msm_ctx* key, const void* ck_c_jacobian96,
                                const void* x32_canonical, const void* u32_canonical, const void* comm_w_jacobian96, const void* comm_e_jacobian96,
                                const void* label, size_t label_len, const lurk_hip_spartan_proof* proof, int* accepted, int* failed_check, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && key && ck_c_jacobian96 && u32_canonical && comm_w_jacobian96 && comm_e_jacobian96 && proof && accepted, "null argument");
        LURK_REQUIRE(num_io == 0 || x32_canonical, "null public IO");
        LURK_REQUIRE(label || label_len == 0, "null label");
        LURK_REQUIRE(proof->polys_outer && proof->claims_outer && proof->eval_e && proof->polys_inner && proof->eval_w && proof->polys_batch && proof->evals_batch &&
                         proof->ipa_l && proof->ipa_r && proof->ipa_a,
                     "null proof buffer");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_VERIFY_MALFORMED;
        const KeyInfo k = key_info(key);
        check_instance_shape(shape, num_cons, num_vars, num_io, k);
        DeviceGuard dg(k.device);
        int failed = LURK_VERIFY_MALFORMED;
        with_pasta_curve(k.curve, [&](auto, auto SF) {
            failed = spartan_verify<decltype(SF)>(k.curve, k.field_id, shape, num_cons, num_vars, num_io, key, ck_c_jacobian96, x32_canonical, u32_canonical,
                                                  comm_w_jacobian96, comm_e_jacobian96, label, label_len, proof, (hipStream_t)stream);
        });
        *accepted = failed == LURK_VERIFY_ACCEPTED;
        if (failed_check) *failed_check = failed;
    });
}

int lurk_hip_spartan_verify_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, lurk_hip_msm_ctx* key, const void* ck_c_jacobian96,
                                      const void* label, size_t label_len, const lurk_hip_spartan_batch_proof* proof, int* accepted, int* failed_check,
                                      void* stream) {
    return guarded([&] {
        LURK_REQUIRE(instances && n_instances >= 1 && n_instances <= 64 && key && ck_c_jacobian96 && proof && accepted, "null argument, or not 1..64 instances");
        LURK_REQUIRE(label || label_len == 0, "null label");
        LURK_REQUIRE(proof->polys_outer && proof->claims_outer && proof->evals_e && proof->polys_inner && proof->evals_w && proof->polys_batch && proof->evals_batch &&
                         proof->ipa_l && proof->ipa_r && proof->ipa_a,
                     "null proof buffer");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_VERIFY_MALFORMED;
        const KeyInfo k = key_info(key);
        for (size_t i = 0; i < n_instances; i++) {
            const lurk_hip_spartan_instance& it = instances[i];
            LURK_REQUIRE(it.shape && it.u32_canonical && it.comm_w_jacobian96 && it.comm_e_jacobian96, "null instance field");
            LURK_REQUIRE(it.num_io == 0 || it.x32_canonical, "null public IO");
            check_instance_shape(it.shape, it.num_cons, it.num_vars, it.num_io, k);
        }
        DeviceGuard dg(k.device);
        int failed = LURK_VERIFY_MALFORMED;
        with_pasta_curve(k.curve, [&](auto, auto SF) {
            failed = spartan_verify_batch<decltype(SF)>(k.curve, k.field_id, instances, n_instances, key, ck_c_jacobian96, label, label_len, proof, (hipStream_t)stream);
        });
        *accepted = failed == LURK_VERIFY_ACCEPTED;
        if (failed_check) *failed_check = failed;
    });
}

int lurk_hip_spartan_kzg_verify_dev(const lurk_hip_r1cs* shape, size_t num_cons, size_t num_vars, size_t num_io, const void* x32_canonical, const void* u32_canonical,
                                    const void* comm_w_jacobian96, const void* comm_e_jacobian96, const void* label, size_t label_len,
                                    const lurk_hip_spartan_kzg_proof* proof, void* out_l_jacobian96, void* out_r_jacobian96, int* accepted, int* failed_check,
                                    void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && u32_canonical && comm_w_jacobian96 && comm_e_jacobian96 && proof && out_l_jacobian96 && out_r_jacobian96 && accepted, "null argument");
        LURK_REQUIRE(num_io == 0 || x32_canonical, "null public IO");
        LURK_REQUIRE(label || label_len == 0, "null label");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_VERIFY_MALFORMED;
        memset(out_l_jacobian96, 0, 96);
        memset(out_r_jacobian96, 0, 96);
        LURK_REQUIRE((num_cons > num_vars ? num_cons : num_vars) != 1, "N = max(num_cons, num_vars) = 1: the HyperKZG opening needs N >= 2");
        check_kzg_instance_shape(shape, num_cons, num_vars, num_io, shape->sh.device);
        LURK_REQUIRE(proof->polys_outer && proof->claims_outer && proof->eval_e && proof->polys_inner && proof->eval_w && proof->polys_batch && proof->evals_batch &&
                         proof->kzg_v && proof->kzg_w && (proof->kzg_com || (num_cons == 2 && num_vars == 2)),
                     "null proof buffer");
        DeviceGuard dg(shape->sh.device);
        const int failed = spartan_kzg_verify(shape, num_cons, num_vars, num_io, x32_canonical, u32_canonical, comm_w_jacobian96, comm_e_jacobian96, label, label_len, proof,
                                              out_l_jacobian96, out_r_jacobian96, (hipStream_t)stream);
        *accepted = failed == LURK_VERIFY_ACCEPTED;
        if (failed_check) *failed_check = failed;
    });
}

int lurk_hip_spartan_kzg_verify_batch_dev(const lurk_hip_spartan_instance* instances, size_t n_instances, const void* label, size_t label_len,
                                          const lurk_hip_spartan_kzg_batch_proof* proof, void* out_l_jacobian96, void* out_r_jacobian96, int* accepted,
                                          int* failed_check, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(instances && n_instances >= 1 && n_instances <= 64 && proof && out_l_jacobian96 && out_r_jacobian96 && accepted,
                     "null argument, or not 1..64 instances");
        LURK_REQUIRE(label || label_len == 0, "null label");
        *accepted = 0;
        if (failed_check) *failed_check = LURK_VERIFY_MALFORMED;
        memset(out_l_jacobian96, 0, 96);
        memset(out_r_jacobian96, 0, 96);
        for (size_t i = 0; i < n_instances; i++) {
            const lurk_hip_spartan_instance& it = instances[i];
            LURK_REQUIRE(it.shape && it.u32_canonical && it.comm_w_jacobian96 && it.comm_e_jacobian96, "null instance field");
            LURK_REQUIRE(it.num_io == 0 || it.x32_canonical, "null public IO");
        }
        const size_t N = batch_n(instances, n_instances);
        LURK_REQUIRE(N != 1, "N = max(num_cons, num_vars) = 1: the HyperKZG opening needs N >= 2");
        const int device = instances[0].shape->sh.device;
        for (size_t i = 0; i < n_instances; i++)
            check_kzg_instance_shape(instances[i].shape, instances[i].num_cons, instances[i].num_vars, instances[i].num_io, device);
        LURK_REQUIRE(proof->polys_outer && proof->claims_outer && proof->evals_e && proof->polys_inner && proof->evals_w && proof->polys_batch && proof->evals_batch &&
                         proof->kzg_v && proof->kzg_w && (proof->kzg_com || N == 2),
                     "null proof buffer");
        DeviceGuard dg(device);
        const int failed = spartan_kzg_verify_batch(instances, n_instances, label, label_len, proof, out_l_jacobian96, out_r_jacobian96, (hipStream_t)stream);
        *accepted = failed == LURK_VERIFY_ACCEPTED;
        if (failed_check) *failed_check = failed;
    });
}

}  // extern "C"
