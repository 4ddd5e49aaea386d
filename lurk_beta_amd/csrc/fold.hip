// fold.hip - the device-resident part of one relaxed-R1CS folding step.
//
// Replaces, for the arithmetic only, what arecibo's NIFS::prove does on the CPU between the two commitments
// of a step (caller: RecursiveSNARK::prove_step, /root/reference/src/proof/nova.rs:291-293; arecibo itself is
// an un-vendored git dependency, /root/reference/Cargo.toml:128, so this follows the published Nova
// construction and oracle/oracle.c restates it - parity unpinned, no golden vectors upstream):
//   R1CSShape::multiply_vec   (A z, B z, C z)                          -> lurk_hip_r1cs_multiply_vec_dev
//   R1CSShape::commit_T       T = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - u2 CZ1 -> lurk_hip_r1cs_cross_term_dev
//   RelaxedR1CSWitness::fold  W <- W1 + r W2,  E <- E1 + r T            -> lurk_hip_fold_vec_dev
// With these the witness vectors never leave HBM between commit(W), commit(T) and the next step.
//
// Layout.  A shape keeps its three CSR matrices resident: row pointers (u32), and per non-zero ONE 8-byte
// record {column, coefficient id}.  R1CS coefficients repeat massively (+-1, small constants), so the 32-byte
// values are replaced by ids into a dictionary of distinct coefficients built once at creation (radix-2^29
// limbs, 48-byte records, read through L2): 8 B per non-zero instead of 36 B.  z = [W | u | X] as arecibo lays
// it out; all field elements cross the ABI as 32-byte Montgomery(2^256) values.
//
// Kernels: one lane per row (the step circuit's rows hold 3-4 entries; neighbouring lanes read neighbouring
// CSR records); the few long rows (more than FOLD_LONG entries - bit decompositions: ~255) are listed at creation and walked
// by FOLD_GROUP lanes per row.  The row's inner product and its bounds: r1cs_shape.cuh, r1cs_row.  The cross-term kernel runs
// the six inner products of a row (A, B, C times z1, z2) from one pass over the matrices and finishes T as a four-term lazy
// row: AZ1*BZ2 + AZ2*BZ1 + (-u1)*CZ2 + (-u2)*CZ1.
// Both kernels are bound by the random 32-byte gathers from z (HBM / L2), not by arithmetic.
#include <memory>
#include <unordered_map>

#include "common.hpp"
#include "dispatch.hpp"
#include "r1cs_bn254fq.hpp"
#include "r1cs_shape.cuh"

// Fields.  The kernels below are templates over the field pack.  This unit instantiates them over the three fields of with_field; over
// Bn254Fq (the BN254 base field: Grumpkin's scalar field) they are instantiated by fold_bn254fq.hip, which includes this file under
// LURK_FOLD_BN254FQ_TU and defines the *_bn254fq functions of r1cs_bn254fq.hpp - this unit only calls those.
// The lazy-accumulation bounds for p = BN254_P (0x30644e72...d87cfd47, 2^253.6: above BN254_R by 2^127, below both Pasta moduli).  Every
// bound of the row code is an UPPER bound that p enters through p < 2^254.1 alone, so each carries over to the smaller modulus as stated:
//   dot29_mac        columns of products of tight limbs (< 2^58 each, 9 per term and column): 45 products + the reduction's 10 terms
//                    < 55 * 2^58 < 2^64.  Independent of p; row_mac normalises every fourth term (36 products per column in between).
//   32 (-u) 2^256    fe_neg returns a canonical value < p; f29_from_mont256 shifts by 5: tight, < 32 p < 2^258.6 (< 2^259 as stated).
//   r1cs_row         a term is coefficient (canonical, < p) x element (< 32 p) / 2^261 < p^2 / 2^256 < 2^251.2 (< 2^253 as stated); 64
//                    terms and the re-entered partial sum stay < 2^259 + p, a group's 256-entry sum < 256 * 2^252 + 16 p < 2^261; and
//                    dot29_finish returns < A / 2^261 + p, tight.  f29_to_mont256: (a r256 + m p) / 2^261 < 2 p for a < 2^261, which
//                    fe_cond_sub2 + fe_cond_sub bring below p.
// What does depend on the modulus is the FORM of the product: Bn254Fq is not 1 mod 2^29, so f29_p1_form is false and f29_mul30 /
// dot29_finish take the general rows (field29_mul_asm_bn254fq.cuh, f29_reduce) - the signed / p1 rows of field29.cuh are not reachable.
namespace lurk {


// The cross term and the two folds are links of the step's serial chain (cross term -> commit(T) -> r -> folds -> next cross term) and
// are bound by HBM latency, not by issue slots; what shares the device with them is an accumulation of the NEXT step's commit(W2)
// (step.hip: LURK_MSM_SUBMIT_FOLLOW), whose waves are older and - at equal priority - served first by the instruction arbiter:
// measured round 6, a 60 us fold took 320 us and the cross term 590 instead of 410.  Raised wave priority lets these waves issue when
// their loads come back (3: the class of commit(T)'s own short kernels; a followed commitment's tail runs at 2, accumulations at 0-1).
__device__ __forceinline__ void fold_wave_prio() { __builtin_amdgcn_s_setprio(3); }

#ifndef LURK_FOLD_MIN_WAVES
#define LURK_FOLD_MIN_WAVES 1  // (HIP: minimum waves per SIMD the cross-term kernels are compiled for)
#endif

template <class P>
__device__ __forceinline__ void fold_store(Fe<P>* dst, const F29<P>& v) {
    *dst = f29_to_mont256<P>(v);
}

// This lane's row in workgroup bid of the nb of its kind, and the bounds of the row's three combinations.
//   LONG = false  one lane per row (XCD-aware); false: no row here, or a long one that is left to the other kind
//   LONG = true   FOLD_GROUP lanes per entry of long_rows, in list order (fold_row_block is not applied to these few blocks); every
//                 lane walks a row (r1cs_shape.cuh: row_slot), `lead` is the lane that holds and stores the row's values
template <bool LONG>
__device__ __forceinline__ bool fold_lane_row(const R1csDev& s, unsigned bid, unsigned nb, size_t& row, uint32_t& gl, bool& lead, uint32_t* lo, uint32_t* hi) {
    if (!LONG) {
        row = fold_row_block(bid, nb) * FOLD_BLOCK + threadIdx.x;
        gl = 0;
        lead = true;
        return row < s.rows && !fold_is_long(s, row, lo, hi);
    }
    const RowSlot t = row_slot<FOLD_GROUP>(s.long_rows, s.n_long, bid, threadIdx.x);
    row = t.row;
    gl = t.gl;
    lead = t.live && t.gl == 0;
    fold_is_long(s, row, lo, hi);
    return true;
}

// LONG = false: one lane per row, long rows skipped;  LONG = true: FOLD_GROUP lanes per entry of long_rows
template <class P, bool LONG>
__global__ __launch_bounds__(FOLD_BLOCK) void r1cs_multiply_vec_kernel(R1csDev s, const Fe<P>* __restrict__ z, Fe<P>* __restrict__ az,
                                                                         Fe<P>* __restrict__ bz, Fe<P>* __restrict__ cz) {
    constexpr int G = LONG ? FOLD_GROUP : 1;
    const uint32_t* one29 = s.dict + s.dict_size * P29_STRIDE;  // the Montgomery one closes the dictionary
    uint32_t lo[3], hi[3], gl;
    size_t row;
    bool lead;
    if (!fold_lane_row<LONG>(s, blockIdx.x, gridDim.x, row, gl, lead, lo, hi)) return;
    F29<P> r = r1cs_row<P, G, LONG, false>(s.a, s.dict, one29, lo[0], hi[0], gl, z);
    if (lead) fold_store<P>(az + row, r);
    r = r1cs_row<P, G, LONG, false>(s.b, s.dict, one29, lo[1], hi[1], gl, z);
    if (lead) fold_store<P>(bz + row, r);
    r = r1cs_row<P, G, LONG, false>(s.c, s.dict, one29, lo[2], hi[2], gl, z);
    if (lead) fold_store<P>(cz + row, r);
}

// -u1, -u2 (u_i = z_i[num_vars]) are negated and converted by every lane that finishes a row: two broadcast loads and two
// limb repackings, so that a call keeps no state outside its arguments (concurrent calls on one shape are independent)
// bid / nb: this workgroup's index among the nb workgroups of its kind (the long-row and the short-row blocks of ONE launch)
template <class P, bool LONG>
__device__ __forceinline__ void r1cs_cross_term_body(const R1csDev& s, const Fe<P>* __restrict__ z1, const Fe<P>* __restrict__ z2, size_t u_index,
                                                     Fe<P>* __restrict__ t, unsigned bid, unsigned nb) {
    constexpr int G = LONG ? FOLD_GROUP : 1;
    const uint32_t* one29 = s.dict + s.dict_size * P29_STRIDE;
    const Fe<P>* zs[2] = {z1, z2};
    uint32_t lo[3], hi[3], gl;
    F29<P> a[2], b[2], c[2];
    size_t row;
    bool lead;
    if (!fold_lane_row<LONG>(s, bid, nb, row, gl, lead, lo, hi)) return;
    // one vector at a time (a second pass re-reads the 8-byte records from L2 but halves the live accumulators:
    // 3 waves/SIMD instead of 2 with spills); T is built up as the row values arrive
#pragma unroll
    for (int v = 0; v < 2; v++) {
        a[v] = r1cs_row<P, G, LONG, false>(s.a, s.dict, one29, lo[0], hi[0], gl, zs[v]);
        b[v] = r1cs_row<P, G, LONG, false>(s.b, s.dict, one29, lo[1], hi[1], gl, zs[v]);
    }
    Dot29<P> acc;
    dot29_init<P>(acc);
    dot29_mac<P>(acc, a[0], b[1]);
    dot29_mac<P>(acc, a[1], b[0]);
#pragma unroll
    for (int v = 0; v < 2; v++) c[v] = r1cs_row<P, G, LONG, false>(s.c, s.dict, one29, lo[2], hi[2], gl, zs[v]);
    if (!lead) return;
    dot29_mac<P>(acc, f29_from_mont256<P>(fe_neg<P>(z1[u_index])), c[1]);  // 32 (-u) 2^256: lazy Montgomery-2^261 form, tight, < 2^259
    dot29_mac<P>(acc, f29_from_mont256<P>(fe_neg<P>(z2[u_index])), c[0]);
    fold_store<P>(t + row, dot29_finish<P>(acc));
}
// ONE launch: the first long_blocks workgroups take the few long rows (bit decompositions: ~255 entries, FOLD_GROUP lanes per row - a
// latency-bound handful of waves), the rest one short row per lane.  As two launches on one stream the long-row kernel ran ALONE first:
// 0.14 ms of a 0.42 ms cross term at rc = 100 with the device nearly idle (profiles/r04_step_timeline_rc100.txt), and commit(T) - which
// waits for T - started that much later.
template <class P>
__global__ __launch_bounds__(FOLD_BLOCK, LURK_FOLD_MIN_WAVES) void r1cs_cross_term_kernel(R1csDev s, const Fe<P>* __restrict__ z1, const Fe<P>* __restrict__ z2,
                                                                       size_t u_index, Fe<P>* __restrict__ t, unsigned long_blocks) {
    fold_wave_prio();
    if (blockIdx.x < long_blocks) r1cs_cross_term_body<P, true>(s, z1, z2, u_index, t, blockIdx.x, long_blocks);
    else r1cs_cross_term_body<P, false>(s, z1, z2, u_index, t, blockIdx.x - long_blocks, gridDim.x - long_blocks);
}

// ---- the cross term with the running products cached (round 6) ---------------------------------------------------------------------
// A z1, B z1, C z1 fold linearly with the running instance (A (z1 + r z2) = A z1 + r A z2), so a folding context keeps them resident
// beside z1 and E (step.hip) and a step gathers from z2 ALONE: three inner products per row instead of six, half the dependent
// 32-byte gather chains and half the Montgomery conversions of r1cs_cross_term_kernel - the kernel is bound by exactly those (L1 tag
// path 55 %, VALU 47 %: profiles/r04_cross_term_pmc.txt).  The cached rows arrive as three coalesced 32-byte reads per lane; A z2, B z2,
// C z2 leave the same way for finish(r), which folds them into the cache in the launch that folds z and E (fold_vecs_kernel).
// The fold of the cache itself rides in the same kernel (prev != nullptr): the products left by the PREVIOUS step and that step's
// challenge, cached row <- cached row + r_prev * previous row, stored back in place and used at once - the step's finish(r) then has
// nothing on the chain between the transcript and the next cross term (the folds of z and E, which the cross term does not read, run on
// a side stream: step.hip), and the three cached vectors are read once per step instead of twice.
template <class P>
struct CachedProducts {
    Fe<P>* a1;  // A z1, B z1, C z1: read, and written back when prev_* are given
    Fe<P>* b1;
    Fe<P>* c1;
    const Fe<P>* prev_a;  // A z2, B z2, C z2 of the previous step (or nullptr: nothing to fold in)
    const Fe<P>* prev_b;
    const Fe<P>* prev_c;
    Fe<P> r_prev;  // the previous step's challenge (Montgomery)
    Fe<P> u1;      // the running u AFTER that fold (Montgomery): the host folds scalars itself
};
template <class P>
__device__ __forceinline__ Fe<P> cached_row(Fe<P>* cur, const Fe<P>* prev, const Fe<P>& r, size_t row) {
    Fe<P> v = cur[row];
    if (prev) {
        v = fe_add<P>(v, fe_mul<P>(r, prev[row]));
        cur[row] = v;
    }
    return v;
}
template <class P, bool LONG>
__device__ __forceinline__ void r1cs_cross_term_cached_body(const R1csDev& s, const Fe<P>* __restrict__ z2, const CachedProducts<P>& cp, size_t u_index,
                                                            Fe<P>* __restrict__ t, Fe<P>* __restrict__ az2, Fe<P>* __restrict__ bz2,
                                                            Fe<P>* __restrict__ cz2, unsigned bid, unsigned nb) {
    constexpr int G = LONG ? FOLD_GROUP : 1;
    const uint32_t* one29 = s.dict + s.dict_size * P29_STRIDE;
    uint32_t lo[3], hi[3], gl;
    size_t row;
    bool store;
    if (!fold_lane_row<LONG>(s, bid, nb, row, gl, store, lo, hi)) return;
    // One product at a time, each folded into T's four-term lazy row and stored as soon as it is complete: only ONE row value is live
    // beside the accumulator (three of them at once cost the kernel its third wave per SIMD: 200 registers against 168).
    Dot29<P> acc;
    dot29_init<P>(acc);
    F29<P> v = r1cs_row<P, G, LONG, false>(s.a, s.dict, one29, lo[0], hi[0], gl, z2);
    if (store) {
        dot29_mac<P>(acc, v, f29_from_mont256<P>(cached_row<P>(cp.b1, cp.prev_b, cp.r_prev, row)));  // A z2 o B z1
        fold_store<P>(az2 + row, v);
    }
    v = r1cs_row<P, G, LONG, false>(s.b, s.dict, one29, lo[1], hi[1], gl, z2);
    if (store) {
        dot29_mac<P>(acc, f29_from_mont256<P>(cached_row<P>(cp.a1, cp.prev_a, cp.r_prev, row)), v);  // A z1 o B z2
        fold_store<P>(bz2 + row, v);
    }
    v = r1cs_row<P, G, LONG, false>(s.c, s.dict, one29, lo[2], hi[2], gl, z2);
    if (!store) return;
    dot29_mac<P>(acc, f29_from_mont256<P>(fe_neg<P>(cp.u1)), v);                                                                          // - u1 C z2
    dot29_mac<P>(acc, f29_from_mont256<P>(fe_neg<P>(z2[u_index])), f29_from_mont256<P>(cached_row<P>(cp.c1, cp.prev_c, cp.r_prev, row)));  // - u2 C z1
    fold_store<P>(cz2 + row, v);
    fold_store<P>(t + row, dot29_finish<P>(acc));
}
template <class P>
__global__ __launch_bounds__(FOLD_BLOCK, LURK_FOLD_MIN_WAVES) void r1cs_cross_term_cached_kernel(R1csDev s, const Fe<P>* __restrict__ z2, CachedProducts<P> cp,
                                                                              size_t u_index, Fe<P>* __restrict__ t, Fe<P>* __restrict__ az2,
                                                                              Fe<P>* __restrict__ bz2, Fe<P>* __restrict__ cz2, unsigned long_blocks) {
    fold_wave_prio();
    if (blockIdx.x < long_blocks) r1cs_cross_term_cached_body<P, true>(s, z2, cp, u_index, t, az2, bz2, cz2, blockIdx.x, long_blocks);
    else r1cs_cross_term_cached_body<P, false>(s, z2, cp, u_index, t, az2, bz2, cz2, blockIdx.x - long_blocks, gridDim.x - long_blocks);
}

// out = a + r b (r: Montgomery 2^256, broadcast).  A pure 96 B / element stream (two reads, one write): a lane takes FOLD_VEC_E
// elements FOLD_BLOCK apart, issues all of their 128-bit loads before the first product (8 loads in flight per lane; with one
// element per trip of a grid-stride loop the kernel sat at 45-53 % of HBM, waiting on each pair of loads in turn), and the grid
// covers the vector exactly once.
constexpr int FOLD_VEC_E = 2;
template <class P>
__global__ __launch_bounds__(FOLD_BLOCK) void fold_vec_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, Fe<P> r, size_t n,
                                                                uint4* __restrict__ out) {
    fold_wave_prio();
    const size_t base = (size_t)blockIdx.x * (FOLD_BLOCK * FOLD_VEC_E) + threadIdx.x;
    uint4 al[FOLD_VEC_E], ah[FOLD_VEC_E], bl[FOLD_VEC_E], bh[FOLD_VEC_E];
#pragma unroll
    for (int e = 0; e < FOLD_VEC_E; e++) {
        const size_t i = base + (size_t)e * FOLD_BLOCK;
        if (i < n) {
            al[e] = a[2 * i];
            ah[e] = a[2 * i + 1];
            bl[e] = b[2 * i];
            bh[e] = b[2 * i + 1];
        }
    }
#pragma unroll
    for (int e = 0; e < FOLD_VEC_E; e++) {
        const size_t i = base + (size_t)e * FOLD_BLOCK;
        if (i >= n) continue;
        Fe<P> x, y;
        x.l[0] = al[e].x; x.l[1] = al[e].y; x.l[2] = al[e].z; x.l[3] = al[e].w; x.l[4] = ah[e].x; x.l[5] = ah[e].y; x.l[6] = ah[e].z; x.l[7] = ah[e].w;
        y.l[0] = bl[e].x; y.l[1] = bl[e].y; y.l[2] = bl[e].z; y.l[3] = bl[e].w; y.l[4] = bh[e].x; y.l[5] = bh[e].y; y.l[6] = bh[e].z; y.l[7] = bh[e].w;
        x = fe_add<P>(x, fe_mul<P>(r, y));
        out[2 * i] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
        out[2 * i + 1] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
    }
}

// Up to FOLD_VECS_MAX folds out_k = a_k + r b_k in ONE launch (the step's finish(r): [W | u | X], E and the three cached products): a
// workgroup belongs to one vector (first_block[k] <= blockIdx.x < first_block[k + 1]) and does what fold_vec_kernel does for it.  Five
// launches of 30 MB each are each bound by their own ramp-up (fold_vec at rc = 100: 49 % of HBM); one launch of 150 MB is not.
constexpr int FOLD_VECS_MAX = 8;
struct FoldVecs {
    const uint4* a[FOLD_VECS_MAX];
    const uint4* b[FOLD_VECS_MAX];
    uint4* out[FOLD_VECS_MAX];
    size_t n[FOLD_VECS_MAX];
    unsigned first_block[FOLD_VECS_MAX + 1];
    int count;
};
template <class P>
__global__ __launch_bounds__(FOLD_BLOCK) void fold_vecs_kernel(FoldVecs v, Fe<P> r) {
    fold_wave_prio();
    int k = 0;
#pragma unroll
    for (int j = 1; j < FOLD_VECS_MAX; j++)
        if (j < v.count && blockIdx.x >= v.first_block[j]) k = j;
    const uint4* __restrict__ a = v.a[k];
    const uint4* __restrict__ b = v.b[k];
    uint4* __restrict__ out = v.out[k];
    const size_t n = v.n[k];
    const size_t base = (size_t)(blockIdx.x - v.first_block[k]) * (FOLD_BLOCK * FOLD_VEC_E) + threadIdx.x;
    uint4 al[FOLD_VEC_E], ah[FOLD_VEC_E], bl[FOLD_VEC_E], bh[FOLD_VEC_E];
#pragma unroll
    for (int e = 0; e < FOLD_VEC_E; e++) {
        const size_t i = base + (size_t)e * FOLD_BLOCK;
        if (i < n) {
            al[e] = a[2 * i];
            ah[e] = a[2 * i + 1];
            bl[e] = b[2 * i];
            bh[e] = b[2 * i + 1];
        }
    }
#pragma unroll
    for (int e = 0; e < FOLD_VEC_E; e++) {
        const size_t i = base + (size_t)e * FOLD_BLOCK;
        if (i >= n) continue;
        Fe<P> x, y;
        x.l[0] = al[e].x; x.l[1] = al[e].y; x.l[2] = al[e].z; x.l[3] = al[e].w; x.l[4] = ah[e].x; x.l[5] = ah[e].y; x.l[6] = ah[e].z; x.l[7] = ah[e].w;
        y.l[0] = bl[e].x; y.l[1] = bl[e].y; y.l[2] = bl[e].z; y.l[3] = bl[e].w; y.l[4] = bh[e].x; y.l[5] = bh[e].y; y.l[6] = bh[e].z; y.l[7] = bh[e].w;
        x = fe_add<P>(x, fe_mul<P>(r, y));
        out[2 * i] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
        out[2 * i + 1] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
    }
}

// out[j] = sum_k c_k (j < len_k ? P_k[j] : 0) for j < n_out: the joint polynomial of the BN254 compressing provers (spartan.hip) out of
// vectors of different lengths, without their zero-padded copies.  A pure stream bound by HBM: 32 B (sum_k len_k + n_out) per launch,
// every input read once, the output written once, nothing cleared - W + gamma E at 2^20 x 2^20 moves 96 MiB where two memsets, two
// copies and fold_vec move 288 MiB in five launches.  The conventions of fold_vec_kernel: a lane takes FOLD_PADDED_E elements
// FOLD_BLOCK apart and issues the 128-bit loads of one term for all of them before the first product (8 in flight per lane), the grid
// covers the output exactly once; like fold_vecs_kernel it adds canonically (fe_add), no lazy accumulation.  The terms (pointer,
// length, Montgomery coefficient) are uniform reads of a small device table: up to 2 x 64 instances do not fit the kernel arguments.
constexpr int FOLD_PADDED_E = 4;
constexpr int FOLD_PADDED_MAX = 128;
struct FoldPaddedTerm {
    const uint4* p;
    uint64_t len;
    uint32_t c[8];
};
template <class P>
__global__ __launch_bounds__(FOLD_BLOCK) void fold_padded_kernel(const FoldPaddedTerm* __restrict__ terms, int count, size_t n_out, uint4* __restrict__ out) {
    fold_wave_prio();
    const size_t block0 = (size_t)blockIdx.x * (FOLD_BLOCK * FOLD_PADDED_E), base = block0 + threadIdx.x;
    Fe<P> acc[FOLD_PADDED_E];
#pragma unroll
    for (int e = 0; e < FOLD_PADDED_E; e++) acc[e] = fe_zero<P>();
    for (int k = 0; k < count; k++) {
        const size_t len = terms[k].len;
        if (block0 >= len) continue;  // (uniform over the workgroup: this stretch of the term is padding)
        const uint4* __restrict__ p = terms[k].p;
        Fe<P> c;
#pragma unroll
        for (int i = 0; i < 8; i++) c.l[i] = terms[k].c[i];
        uint4 lo[FOLD_PADDED_E], hi[FOLD_PADDED_E];
#pragma unroll
        for (int e = 0; e < FOLD_PADDED_E; e++) {
            const size_t i = base + (size_t)e * FOLD_BLOCK;
            if (i < len) {
                lo[e] = p[2 * i];
                hi[e] = p[2 * i + 1];
            }
        }
#pragma unroll
        for (int e = 0; e < FOLD_PADDED_E; e++) {
            const size_t i = base + (size_t)e * FOLD_BLOCK;
            if (i >= len) continue;
            Fe<P> y;
            y.l[0] = lo[e].x; y.l[1] = lo[e].y; y.l[2] = lo[e].z; y.l[3] = lo[e].w; y.l[4] = hi[e].x; y.l[5] = hi[e].y; y.l[6] = hi[e].z; y.l[7] = hi[e].w;
            acc[e] = fe_add<P>(acc[e], fe_mul<P>(c, y));
        }
    }
#pragma unroll
    for (int e = 0; e < FOLD_PADDED_E; e++) {
        const size_t i = base + (size_t)e * FOLD_BLOCK;
        if (i >= n_out) continue;
        out[2 * i] = make_uint4(acc[e].l[0], acc[e].l[1], acc[e].l[2], acc[e].l[3]);
        out[2 * i + 1] = make_uint4(acc[e].l[4], acc[e].l[5], acc[e].l[6], acc[e].l[7]);
    }
}

// workgroups of the long rows: FOLD_GROUP lanes per row, in list order (0 without a long row)
static unsigned fold_long_blocks(const R1csShape& sh) { return div_up(sh.n_long * FOLD_GROUP, FOLD_BLOCK); }

// ---- host side ---------------------------------------------------------------------------------------------
struct Key32 {
    uint64_t w[4];
    bool operator==(const Key32& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
};
struct Key32Hash {
    size_t operator()(const Key32& k) const {
        uint64_t h = k.w[0] * 0x9E3779B97F4A7C15ull;
        h ^= (k.w[1] + 0xBF58476D1CE4E5B9ull) * 0x94D049BB133111EBull;
        h ^= (k.w[2] + 0x2545F4914F6CDD1Dull) * 0xD6E8FEB86659FD93ull;
        h ^= (k.w[3] + 0x9E3779B97F4A7C15ull) * 0xC2B2AE3D27D4EB4Full;
        return (size_t)(h ^ (h >> 29));
    }
};

template <class P>
static void dict_record(const uint64_t* mont256, uint32_t* rec) {
    Fe<P> v;
    for (int i = 0; i < 4; i++) { v.l[2 * i] = (uint32_t)mont256[i]; v.l[2 * i + 1] = (uint32_t)(mont256[i] >> 32); }
    for (int d = 0; d < 5; d++) v = fe_add<P>(v, v);  // c 2^256 -> c 2^261 mod p, canonical
    F29<P> f = f29_from_plain<P>(v.l);
    for (int i = 0; i < P29_STRIDE; i++) rec[i] = i < 9 ? f.l[i] : 0u;
}

static void upload_matrix(R1csShape& sh, int which, const uint64_t* indptr, const uint64_t* indices, const void* data, size_t ncols,
                          std::unordered_map<Key32, uint32_t, Key32Hash>& ids, std::vector<uint32_t>& dict_words) {
    const size_t rows = sh.num_cons;
    LURK_REQUIRE(indptr && indptr[0] == 0, "indptr must start at 0");
    const size_t nnz = indptr[rows];
    LURK_REQUIRE(nnz < ((size_t)1 << 32), "more than 2^32 - 1 non-zeros");
    LURK_REQUIRE(nnz == 0 || (indices && data), "null indices / data");
    std::vector<uint32_t> rp(rows + 1);
    for (size_t i = 0; i <= rows; i++) {
        LURK_REQUIRE(i == 0 || indptr[i] >= indptr[i - 1], "indptr must be non-decreasing");
        rp[i] = (uint32_t)indptr[i];
    }
    std::vector<uint2> ent(nnz);
    const uint64_t* d = (const uint64_t*)data;
    for (size_t k = 0; k < nnz; k++) {
        LURK_REQUIRE(indices[k] < ncols, "column index out of range");
        Key32 key{{d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]}};
        auto it = ids.find(key);
        if (it == ids.end()) {
            uint32_t id = (uint32_t)ids.size();
            it = ids.emplace(key, id).first;
            dict_words.resize(dict_words.size() + P29_STRIDE);
            uint32_t* rec = dict_words.data() + (size_t)id * P29_STRIDE;
            with_scalar_field(sh.field_id, [&](auto F) { dict_record<decltype(F)>(key.w, rec); });
        }
        ent[k] = make_uint2((uint32_t)indices[k], it->second);
    }
    CsrDev& m = sh.m[which];
    m.nnz = nnz;
    m.rowptr.alloc(rp.size() * 4);
    m.ent.alloc(nnz * 8);
    LURK_HIP_CHECK(hipMemcpy(m.rowptr.p, rp.data(), rp.size() * 4, hipMemcpyHostToDevice));
    if (nnz) LURK_HIP_CHECK(hipMemcpy(m.ent.p, ent.data(), nnz * 8, hipMemcpyHostToDevice));
}

template <class P>
static void multiply_vec(const R1csShape& sh, const void* d_z, void* az, void* bz, void* cz, hipStream_t s) {
    if (!sh.num_cons) return;
    ProfScope ps("r1cs_multiply_vec", s);
    const R1csDev d = dev_view(sh);
    if (sh.n_long)  // first: its few latency-bound waves then run beside the lane-per-row launch that follows
        hipLaunchKernelGGL((r1cs_multiply_vec_kernel<P, true>), dim3(fold_long_blocks(sh)), dim3(FOLD_BLOCK), 0, s, d,
                           (const Fe<P>*)d_z, (Fe<P>*)az, (Fe<P>*)bz, (Fe<P>*)cz);
    hipLaunchKernelGGL((r1cs_multiply_vec_kernel<P, false>), dim3(class_blocks(sh.num_cons, 1)), dim3(FOLD_BLOCK), 0, s, d, (const Fe<P>*)d_z,
                       (Fe<P>*)az, (Fe<P>*)bz, (Fe<P>*)cz);
    LURK_HIP_CHECK(hipGetLastError());
}
template <class P>
static void cross_term(const R1csShape& sh, const void* d_z1, const void* d_z2, void* d_t, hipStream_t s) {
    if (!sh.num_cons) return;
    ProfScope ps("r1cs_cross_term", s);
    const R1csDev d = dev_view(sh);
    const unsigned long_blocks = fold_long_blocks(sh);
    hipLaunchKernelGGL((r1cs_cross_term_kernel<P>), dim3(long_blocks + class_blocks(sh.num_cons, 1)), dim3(FOLD_BLOCK), 0, s, d, (const Fe<P>*)d_z1,
                       (const Fe<P>*)d_z2, sh.num_vars, (Fe<P>*)d_t, long_blocks);
    LURK_HIP_CHECK(hipGetLastError());
}
template <class P>
static void cross_term_cached(const R1csShape& sh, const void* d_z2, void* az1, void* bz1, void* cz1, const void* u1_32, const void* prev_a, const void* prev_b,
                              const void* prev_c, const void* r_prev32, void* d_t, void* az2, void* bz2, void* cz2, hipStream_t s) {
    if (!sh.num_cons) return;
    ProfScope ps("r1cs_cross_term", s);
    const R1csDev d = dev_view(sh);
    const unsigned long_blocks = fold_long_blocks(sh);
    CachedProducts<P> cp;
    cp.a1 = (Fe<P>*)az1;
    cp.b1 = (Fe<P>*)bz1;
    cp.c1 = (Fe<P>*)cz1;
    cp.prev_a = (const Fe<P>*)prev_a;
    cp.prev_b = (const Fe<P>*)prev_b;
    cp.prev_c = (const Fe<P>*)prev_c;
    cp.r_prev = fe_zero<P>();
    if (r_prev32) memcpy(cp.r_prev.l, r_prev32, 32);
    memcpy(cp.u1.l, u1_32, 32);
    hipLaunchKernelGGL((r1cs_cross_term_cached_kernel<P>), dim3(long_blocks + class_blocks(sh.num_cons, 1)), dim3(FOLD_BLOCK), 0, s, d, (const Fe<P>*)d_z2, cp,
                       sh.num_vars, (Fe<P>*)d_t, (Fe<P>*)az2, (Fe<P>*)bz2, (Fe<P>*)cz2, long_blocks);
    LURK_HIP_CHECK(hipGetLastError());
}
template <class P>
static void fold_vecs(int count, const void* const* a, const void* const* b, const size_t* n, void* const* out, const void* r32, hipStream_t s) {
    FoldVecs v;
    memset(&v, 0, sizeof(v));
    unsigned blocks = 0;
    for (int k = 0; k < count; k++) {
        if (!n[k]) continue;
        v.a[v.count] = (const uint4*)a[k];
        v.b[v.count] = (const uint4*)b[k];
        v.out[v.count] = (uint4*)out[k];
        v.n[v.count] = n[k];
        v.first_block[v.count] = blocks;
        blocks += div_up(n[k], (size_t)FOLD_BLOCK * FOLD_VEC_E);
        v.count++;
    }
    if (!v.count) return;
    v.first_block[v.count] = blocks;
    Fe<P> r;
    memcpy(r.l, r32, 32);
    ProfScope ps("fold_vec", s);
    hipLaunchKernelGGL((fold_vecs_kernel<P>), dim3(blocks), dim3(FOLD_BLOCK), 0, s, v, r);
    LURK_HIP_CHECK(hipGetLastError());
}
template <class P>
static void fold_vec(const void* a, const void* b, const void* r32, size_t n, void* out, hipStream_t s) {
    if (!n) return;
    Fe<P> r;
    memcpy(r.l, r32, 32);
    ProfScope ps("fold_vec", s);
    const unsigned blocks = div_up(n, (size_t)FOLD_BLOCK * FOLD_VEC_E);
    hipLaunchKernelGGL((fold_vec_kernel<P>), dim3(blocks), dim3(FOLD_BLOCK), 0, s, (const uint4*)a, (const uint4*)b, r, n, (uint4*)out);
    LURK_HIP_CHECK(hipGetLastError());
}

// the terms are staged through the stream's arena; the stream is synchronised once (pageable source: the table leaves this frame)
template <class P>
static void fold_padded(int count, const void* const* vecs, const size_t* lens, const void* coeffs32, size_t n_out, void* out, hipStream_t s) {
    std::vector<FoldPaddedTerm> terms;
    for (int k = 0; k < count; k++) {
        if (!lens[k]) continue;  // a zero-length vector is all padding
        FoldPaddedTerm t;
        t.p = (const uint4*)vecs[k];
        t.len = lens[k];
        memcpy(t.c, (const char*)coeffs32 + 32 * (size_t)k, 32);
        terms.push_back(t);
    }
    ArenaBuf d_terms((terms.size() + 1) * sizeof(FoldPaddedTerm), s);
    if (!terms.empty()) {
        LURK_HIP_CHECK(hipMemcpyAsync(d_terms.p, terms.data(), terms.size() * sizeof(FoldPaddedTerm), hipMemcpyHostToDevice, s));
        LURK_HIP_CHECK(hipStreamSynchronize(s));
    }
    ProfScope ps("fold_padded", s);
    const unsigned blocks = div_up(n_out, (size_t)FOLD_BLOCK * FOLD_PADDED_E);
    hipLaunchKernelGGL((fold_padded_kernel<P>), dim3(blocks), dim3(FOLD_BLOCK), 0, s, (const FoldPaddedTerm*)d_terms.p, (int)terms.size(), n_out, (uint4*)out);
    LURK_HIP_CHECK(hipGetLastError());
}

#ifdef LURK_FOLD_BN254FQ_TU  // fold_bn254fq.hip: the instantiations over the BN254 base field, a code object of their own
void multiply_vec_bn254fq(const R1csShape& sh, const void* d_z, void* az, void* bz, void* cz, hipStream_t s) { multiply_vec<Bn254Fq>(sh, d_z, az, bz, cz, s); }
void cross_term_bn254fq(const R1csShape& sh, const void* d_z1, const void* d_z2, void* d_t, hipStream_t s) { cross_term<Bn254Fq>(sh, d_z1, d_z2, d_t, s); }
void cross_term_cached_bn254fq(const R1csShape& sh, const void* d_z2, void* az1, void* bz1, void* cz1, const void* u1_32, const void* prev_a, const void* prev_b,
                               const void* prev_c, const void* r_prev32, void* d_t, void* az2, void* bz2, void* cz2, hipStream_t s) {
    cross_term_cached<Bn254Fq>(sh, d_z2, az1, bz1, cz1, u1_32, prev_a, prev_b, prev_c, r_prev32, d_t, az2, bz2, cz2, s);
}
void fold_vecs_bn254fq(int count, const void* const* a, const void* const* b, const size_t* n, void* const* out, const void* r32, hipStream_t s) {
    fold_vecs<Bn254Fq>(count, a, b, n, out, r32, s);
}
void fold_vec_bn254fq(const void* a, const void* b, const void* r32, size_t n, void* out, hipStream_t s) { fold_vec<Bn254Fq>(a, b, r32, n, out, s); }

}  // namespace lurk
#else
// lurk_hip_r1cs_create and lurk_hip_r1cs_create_for_curve: the caller has checked field_id
static void r1cs_create_over(lurk_hip_r1cs** out, int field_id, size_t num_cons, size_t num_vars, size_t num_io, const uint64_t* a_indptr,
                             const uint64_t* a_indices, const void* a_data, const uint64_t* b_indptr, const uint64_t* b_indices, const void* b_data,
                             const uint64_t* c_indptr, const uint64_t* c_indices, const void* c_data) {
    LURK_REQUIRE(num_vars + 1 + num_io < ((size_t)1 << 32), "z has more than 2^32 - 1 entries");
    auto h = std::make_unique<lurk_hip_r1cs>();
    R1csShape& sh = h->sh;
    sh.field_id = field_id;
    sh.num_cons = num_cons;
    sh.num_vars = num_vars;
    sh.num_io = num_io;
    LURK_HIP_CHECK(hipGetDevice(&sh.device));
    std::unordered_map<Key32, uint32_t, Key32Hash> ids;
    std::vector<uint32_t> dict_words;
    const size_t ncols = num_vars + 1 + num_io;
    upload_matrix(sh, 0, a_indptr, a_indices, a_data, ncols, ids, dict_words);
    upload_matrix(sh, 1, b_indptr, b_indices, b_data, ncols, ids, dict_words);
    upload_matrix(sh, 2, c_indptr, c_indices, c_data, ncols, ids, dict_words);
    sh.dict_size = ids.size();
    {   // closing record: the Montgomery one (1 * 2^256 mod p as the ABI stores it)
        dict_words.resize(dict_words.size() + P29_STRIDE);
        uint32_t* rec = dict_words.data() + sh.dict_size * P29_STRIDE;
        uint64_t one[4];
        with_scalar_field(field_id, [&](auto F) {
            Fe<decltype(F)> o = fe_one<decltype(F)>();
            memcpy(one, o.l, 32);
            dict_record<decltype(F)>(one, rec);
        });
    }
    {   // rows the lane-per-row kernels leave to the wave-per-row ones
        std::vector<uint32_t> lr;
        for (size_t i = 0; i < num_cons; i++)
            if (a_indptr[i + 1] - a_indptr[i] > FOLD_LONG || b_indptr[i + 1] - b_indptr[i] > FOLD_LONG || c_indptr[i + 1] - c_indptr[i] > FOLD_LONG)
                lr.push_back((uint32_t)i);
        sh.n_long = lr.size();
        sh.long_rows.alloc(lr.size() * 4);
        if (!lr.empty()) LURK_HIP_CHECK(hipMemcpy(sh.long_rows.p, lr.data(), lr.size() * 4, hipMemcpyHostToDevice));
    }
    sh.dict.alloc(dict_words.size() * 4);
    if (!dict_words.empty()) LURK_HIP_CHECK(hipMemcpy(sh.dict.p, dict_words.data(), dict_words.size() * 4, hipMemcpyHostToDevice));
    *out = h.release();
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_r1cs_create(lurk_hip_r1cs** out, int field_id, size_t num_cons, size_t num_vars, size_t num_io, const uint64_t* a_indptr,
                         const uint64_t* a_indices, const void* a_data, const uint64_t* b_indptr, const uint64_t* b_indices, const void* b_data,
                         const uint64_t* c_indptr, const uint64_t* c_indices, const void* c_data) {
    return guarded([&] {
        LURK_REQUIRE(out, "null output handle");
        *out = nullptr;
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        r1cs_create_over(out, field_id, num_cons, num_vars, num_io, a_indptr, a_indices, a_data, b_indptr, b_indices, b_data, c_indptr, c_indices, c_data);
    });
}

int lurk_hip_r1cs_create_for_curve(lurk_hip_r1cs** out, int curve, size_t num_cons, size_t num_vars, size_t num_io, const uint64_t* a_indptr,
                                   const uint64_t* a_indices, const void* a_data, const uint64_t* b_indptr, const uint64_t* b_indices, const void* b_data,
                                   const uint64_t* c_indptr, const uint64_t* c_indices, const void* c_data) {
    return guarded([&] {
        LURK_REQUIRE(out, "null output handle");
        *out = nullptr;
        r1cs_create_over(out, curve_scalar_field_id(curve), num_cons, num_vars, num_io, a_indptr, a_indices, a_data, b_indptr, b_indices, b_data, c_indptr, c_indices,
                         c_data);
    });
}

int lurk_hip_r1cs_destroy(lurk_hip_r1cs* shape) {
    if (!shape) return 0;
    return guarded([&] {
        DeviceGuard dg(shape->sh.device);
        delete shape;
    });
}

int lurk_hip_r1cs_dims(const lurk_hip_r1cs* shape, int* field_id, size_t* num_cons, size_t* num_vars, size_t* num_io) {
    return guarded([&] {
        LURK_REQUIRE(shape, "null shape");
        if (field_id) *field_id = shape->sh.field_id;
        if (num_cons) *num_cons = shape->sh.num_cons;
        if (num_vars) *num_vars = shape->sh.num_vars;
        if (num_io) *num_io = shape->sh.num_io;
    });
}

int lurk_hip_r1cs_device(const lurk_hip_r1cs* shape, int* device) {
    return guarded([&] {
        LURK_REQUIRE(shape && device, "null argument");
        *device = shape->sh.device;
    });
}

int lurk_hip_r1cs_info(const lurk_hip_r1cs* shape, size_t* nnz_a, size_t* nnz_b, size_t* nnz_c, size_t* distinct_coefficients) {
    return guarded([&] {
        LURK_REQUIRE(shape, "null shape");
        if (nnz_a) *nnz_a = shape->sh.m[0].nnz;
        if (nnz_b) *nnz_b = shape->sh.m[1].nnz;
        if (nnz_c) *nnz_c = shape->sh.m[2].nnz;
        if (distinct_coefficients) *distinct_coefficients = shape->sh.dict_size;
    });
}

int lurk_hip_r1cs_multiply_vec_dev(const lurk_hip_r1cs* shape, const void* d_z, void* d_az, void* d_bz, void* d_cz, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && d_z && d_az && d_bz && d_cz, "null argument");
        DeviceGuard dg(shape->sh.device);
        const R1csShape& sh = shape->sh;
        if (sh.field_id == LURK_FIELD_BN254_FQ) multiply_vec_bn254fq(sh, d_z, d_az, d_bz, d_cz, (hipStream_t)stream);
        else with_field(sh.field_id, [&](auto F) { multiply_vec<decltype(F)>(sh, d_z, d_az, d_bz, d_cz, (hipStream_t)stream); });
    });
}

int lurk_hip_r1cs_cross_term_dev(lurk_hip_r1cs* shape, const void* d_z1, const void* d_z2, void* d_t, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && d_z1 && d_z2 && d_t, "null argument");
        DeviceGuard dg(shape->sh.device);
        const R1csShape& sh = shape->sh;
        if (sh.field_id == LURK_FIELD_BN254_FQ) cross_term_bn254fq(sh, d_z1, d_z2, d_t, (hipStream_t)stream);
        else with_field(sh.field_id, [&](auto F) { cross_term<decltype(F)>(sh, d_z1, d_z2, d_t, (hipStream_t)stream); });
    });
}

int lurk_hip_r1cs_cross_term_cached_dev(lurk_hip_r1cs* shape, const void* d_z2, void* d_az1, void* d_bz1, void* d_cz1, const void* u1_32_mont,
                                        const void* d_az2_prev, const void* d_bz2_prev, const void* d_cz2_prev, const void* r_prev32_mont, void* d_t,
                                        void* d_az2, void* d_bz2, void* d_cz2, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(shape && d_z2 && d_az1 && d_bz1 && d_cz1 && u1_32_mont && d_t && d_az2 && d_bz2 && d_cz2, "null argument");
        const bool prev = d_az2_prev || d_bz2_prev || d_cz2_prev || r_prev32_mont;
        LURK_REQUIRE(!prev || (d_az2_prev && d_bz2_prev && d_cz2_prev && r_prev32_mont), "the previous step's products and its challenge go together");
        LURK_REQUIRE(!prev || (d_az2_prev != d_az2 && d_bz2_prev != d_bz2 && d_cz2_prev != d_cz2), "the previous products are read while the new ones are written: two buffers");
        DeviceGuard dg(shape->sh.device);
        const R1csShape& sh = shape->sh;
        if (sh.field_id == LURK_FIELD_BN254_FQ) {
            cross_term_cached_bn254fq(sh, d_z2, d_az1, d_bz1, d_cz1, u1_32_mont, d_az2_prev, d_bz2_prev, d_cz2_prev, r_prev32_mont, d_t, d_az2, d_bz2, d_cz2,
                                      (hipStream_t)stream);
            return;
        }
        with_field(sh.field_id, [&](auto F) {
            cross_term_cached<decltype(F)>(sh, d_z2, d_az1, d_bz1, d_cz1, u1_32_mont, d_az2_prev, d_bz2_prev, d_cz2_prev, r_prev32_mont, d_t, d_az2, d_bz2, d_cz2,
                                           (hipStream_t)stream);
        });
    });
}

}  // extern "C"

// The body of lurk_hip_fold_vecs_dev over the scalar fields of all four curves (r1cs_bn254fq.hpp): a folding context calls it directly.
// (Defined here, where the public call always stood: the order in which this unit instantiates its kernels, and with it its code object, stays.)
namespace lurk {
void fold_vecs_scalar_field(int field_id, int count, const void* const* d_a, const void* const* d_b, const size_t* n, void* const* d_out, const void* r32_mont,
                            hipStream_t s) {
    LURK_REQUIRE(count >= 0 && count <= FOLD_VECS_MAX, "at most 8 vectors per launch");
    LURK_REQUIRE(count == 0 || (d_a && d_b && n && d_out), "null argument");
    LURK_REQUIRE(r32_mont, "null challenge");
    size_t blocks = 0;
    for (int k = 0; k < count; k++) {
        LURK_REQUIRE(n[k] == 0 || (d_a[k] && d_b[k] && d_out[k]), "null buffer");
        blocks += div_up(n[k], (size_t)FOLD_BLOCK * FOLD_VEC_E);
    }
    LURK_REQUIRE(blocks < ((size_t)1 << 31), "too many elements for one launch");
    if (field_id == LURK_FIELD_BN254_FQ) fold_vecs_bn254fq(count, d_a, d_b, n, d_out, r32_mont, s);
    else with_field(field_id, [&](auto F) { fold_vecs<decltype(F)>(count, d_a, d_b, n, d_out, r32_mont, s); });
}
}  // namespace lurk

extern "C" {

int lurk_hip_fold_vecs_dev(int field_id, int count, const void* const* d_a, const void* const* d_b, const size_t* n, void* const* d_out,
                           const void* r32_mont, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");  // (the fourth field is a folding context's alone: step.hip)
        fold_vecs_scalar_field(field_id, count, d_a, d_b, n, d_out, r32_mont, (hipStream_t)stream);
    });
}

int lurk_hip_fold_padded_dev(int field_id, int count, const void* const* d_vecs, const size_t* lens, const void* coeffs32_mont, size_t n_out, void* d_out,
                             void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        LURK_REQUIRE(count >= 1, "count must be at least 1");
        LURK_REQUIRE(count <= FOLD_PADDED_MAX, "at most 128 vectors per launch");
        LURK_REQUIRE(d_vecs && lens && coeffs32_mont && d_out, "null argument");
        LURK_REQUIRE(n_out >= 1 && div_up(n_out, (size_t)FOLD_BLOCK * FOLD_PADDED_E) < (1u << 31) && n_out < ((size_t)1 << 40), "n_out out of range");
        const char* o = (const char*)d_out;
        for (int k = 0; k < count; k++) {
            LURK_REQUIRE(lens[k] == 0 || d_vecs[k], "a null vector with a non-zero length");
            LURK_REQUIRE(lens[k] <= n_out, "a vector is longer than n_out");
            const char* v = (const char*)d_vecs[k];
            LURK_REQUIRE(lens[k] == 0 || o + n_out * 32 <= v || v + lens[k] * 32 <= o, "the output may not overlap an input");
        }
        with_field(field_id, [&](auto F) { fold_padded<decltype(F)>(count, d_vecs, lens, coeffs32_mont, n_out, d_out, (hipStream_t)stream); });
    });
}

// host-pointer forms (small inputs, tests, the C++ mirror): copy in, run, copy out
int lurk_hip_r1cs_multiply_vec(const lurk_hip_r1cs* shape, const void* z, void* az, void* bz, void* cz) {
    return guarded([&] {
        LURK_REQUIRE(shape && z && az && bz && cz, "null argument");
        DeviceGuard dg(shape->sh.device);
        const R1csShape& sh = shape->sh;
        const size_t ncols = sh.num_vars + 1 + sh.num_io, m = sh.num_cons;
        DevBuf d_z(ncols * 32), d_a(m * 32), d_b(m * 32), d_c(m * 32);
        LURK_HIP_CHECK(hipMemcpy(d_z.p, z, ncols * 32, hipMemcpyHostToDevice));
        LURK_REQUIRE(lurk_hip_r1cs_multiply_vec_dev(shape, d_z.p, d_a.p, d_b.p, d_c.p, nullptr) == 0, lurk_hip_last_error());
        LURK_HIP_CHECK(hipDeviceSynchronize());
        LURK_HIP_CHECK(hipMemcpy(az, d_a.p, m * 32, hipMemcpyDeviceToHost));
        LURK_HIP_CHECK(hipMemcpy(bz, d_b.p, m * 32, hipMemcpyDeviceToHost));
        LURK_HIP_CHECK(hipMemcpy(cz, d_c.p, m * 32, hipMemcpyDeviceToHost));
    });
}

int lurk_hip_r1cs_cross_term(lurk_hip_r1cs* shape, const void* z1, const void* z2, void* t) {
    return guarded([&] {
        LURK_REQUIRE(shape && z1 && z2 && t, "null argument");
        DeviceGuard dg(shape->sh.device);
        const R1csShape& sh = shape->sh;
        const size_t ncols = sh.num_vars + 1 + sh.num_io, m = sh.num_cons;
        DevBuf d_z1(ncols * 32), d_z2(ncols * 32), d_t(m * 32);
        LURK_HIP_CHECK(hipMemcpy(d_z1.p, z1, ncols * 32, hipMemcpyHostToDevice));
        LURK_HIP_CHECK(hipMemcpy(d_z2.p, z2, ncols * 32, hipMemcpyHostToDevice));
        LURK_REQUIRE(lurk_hip_r1cs_cross_term_dev(shape, d_z1.p, d_z2.p, d_t.p, nullptr) == 0, lurk_hip_last_error());
        LURK_HIP_CHECK(hipDeviceSynchronize());
        LURK_HIP_CHECK(hipMemcpy(t, d_t.p, m * 32, hipMemcpyDeviceToHost));
    });
}

int lurk_hip_fold_vec(int field_id, const void* a, const void* b, const void* r32_mont, size_t n, void* out) {
    return guarded([&] {
        LURK_REQUIRE(n == 0 || (a && b && out), "null buffer");
        DevBuf d_a(n * 32), d_b(n * 32), d_o(n * 32);
        if (n) {
            LURK_HIP_CHECK(hipMemcpy(d_a.p, a, n * 32, hipMemcpyHostToDevice));
            LURK_HIP_CHECK(hipMemcpy(d_b.p, b, n * 32, hipMemcpyHostToDevice));
        }
        LURK_REQUIRE(lurk_hip_fold_vec_dev(field_id, d_a.p, d_b.p, r32_mont, n, d_o.p, nullptr) == 0, lurk_hip_last_error());
        LURK_HIP_CHECK(hipDeviceSynchronize());
        if (n) LURK_HIP_CHECK(hipMemcpy(out, d_o.p, n * 32, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"

// the body of lurk_hip_fold_vec_dev, likewise
namespace lurk {
void fold_vec_scalar_field(int field_id, const void* d_a, const void* d_b, const void* r32_mont, size_t n, void* d_out, hipStream_t s) {
    LURK_REQUIRE(n == 0 || (d_a && d_b && d_out), "null buffer");
    LURK_REQUIRE(r32_mont, "null challenge");
    if (field_id == LURK_FIELD_BN254_FQ) fold_vec_bn254fq(d_a, d_b, r32_mont, n, d_out, s);
    else with_field(field_id, [&](auto F) { fold_vec<decltype(F)>(d_a, d_b, r32_mont, n, d_out, s); });
}
}  // namespace lurk

extern "C" {

int lurk_hip_fold_vec_dev(int field_id, const void* d_a, const void* d_b, const void* r32_mont, size_t n, void* d_out, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        fold_vec_scalar_field(field_id, d_a, d_b, r32_mont, n, d_out, (hipStream_t)stream);
    });
}

}  // extern "C"
#endif  // LURK_FOLD_BN254FQ_TU
