// ntt29.cuh - the butterfly of the NTT's wave-resident passes (ntt.hip: ntt_wave_pass_kernel) on the radix-2^29 layer
// (field29.cuh).  In a header of its own so that tests/host_harness can run the passes' value sequence on the host with every
// bound below asserted (LURK_F29_CHECK); the kernel is the only product user.
//
// Bounds (asserted in the host-harness build):
//   u on entry      tight limbs, value < 2^260 (a fresh product < 2^255 + p, or the packed image between passes < 2^255.1,
//                   grown by < 2^256.1 per stage: eight stages stay below 2^259.3)
//   w               a stage twiddle in CANONICAL Montgomery-2^261 form (< p, ntt_twiddle29)
//   x = w v         a fresh product: tight limbs, value < 2^260 p / 2^261 + p < 2^255 + p, so every limb is <= the matching limb
//                   of ntt_bias4.  (With the lazy image f29_from_mont256(w) < 32 p the product reached 1.5 * 2^256 > 4p: the top
//                   limb's subtraction wrapped and came out right only while u's top limb absorbed it.)
//   outputs         tight limbs
#pragma once
#include "field29.cuh"

namespace lurk {

// 4p with its limbs re-balanced like f29_bias (limb_i += 2^30, limb_{i+1} -= 2): subtracting a TIGHT value below 2^256 limb-wise
// never underflows.  The butterflies' subtrahend is always a fresh product (< 2^255 + p), so this small bias replaces the
// general 64p one and a value grows by < 2^256.1 per stage: eight stages stay below 2^259.3 with no reduction in between.
template <class F>
LURK_HD constexpr uint32_t ntt_bias4(int i) {
    uint64_t carry = 0;
    uint32_t limb = 0;
    for (int k = 0; k <= i; k++) {
        uint64_t x = (uint64_t)f29_mod<F>(k) * 4u + carry;
        limb = (uint32_t)(x & F29_MASK);
        carry = x >> 29;
        if (k == 8) limb = (uint32_t)x;
    }
    uint32_t v = limb;
    if (i < 8) v += 1u << 30;
    if (i > 0) v -= 2u;
    return v;
}
// a twiddle of the omega^i table (Montgomery 2^256, canonical) -> the same element in canonical Montgomery-2^261 form: w 2^5 mod p
template <class F>
LURK_HD F29<F> ntt_twiddle29(Fe<F> w) {
#pragma unroll
    for (int i = 0; i < 5; i++) w = fe_add<F>(w, w);
    return f29_from_plain<F>(w.l);
}
// (u, v) <- (u + x, u - x) for the product x = w v: u tight-limbed on entry (value < 2^260), x tight with every limb <= the
// matching limb of ntt_bias4 (a fresh product: < 2^255 + p); both results carried (tight limbs), lazily reduced: each grows by
// < 2^256.1
template <class F>
LURK_HD void ntt_bfly_x(F29<F>& u, F29<F>& v, const F29<F>& x) {
    F29_ASSERT_LIMBS(u, 29, "ntt_bfly u");
    F29_ASSERT_TOP(u, 28, "ntt_bfly u (value >= 2^260)");
    F29_ASSERT_LIMBS(x, 29, "ntt_bfly w v");
    F29<F> d;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        F29_ASSERT(ntt_bias4<F>(i) >= x.l[i], "ntt_bfly: product limb above the 4p bias");
        d.l[i] = u.l[i] + (ntt_bias4<F>(i) - x.l[i]);
    }
    v = f29_carry<F>(d);
    u = f29_carry<F>(f29_add<F>(u, x));
    F29_ASSERT_LIMBS(u, 29, "ntt_bfly u + w v");
    F29_ASSERT_LIMBS(v, 29, "ntt_bfly u - w v");
}
// (u, v) <- (u + w v, u - w v); v tight, w canonical (ntt_twiddle29)
template <class F>
LURK_HD void ntt_bfly(F29<F>& u, F29<F>& v, const F29<F>& w) {
    const F29<F> x = f29_mul<F>(v, w);  // tight, < 2^255 + p
    ntt_bfly_x<F>(u, v, x);
}

}  // namespace lurk
