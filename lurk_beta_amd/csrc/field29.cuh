// field29.cuh - the radix-2^29 arithmetic layer used INSIDE the hot kernels.
//
// gfx950 issues a carry fold (v_addc_co_u32, any form) at 4.1 cycles per wave-instruction - nearly the
// 4.6 of the v_mad_u64_u32 whose carry it folds (profiles/r01_microbench_instr_rates.txt).  With nine
// 29-bit limbs a whole column of partial products fits the 64-bit mad accumulator, so a product needs no
// carry folds: 135 mads instead of 104 mad+fold pairs (Pasta), 162 instead of 128 pairs (BN254).
//
// Representation: F29 = 9 limbs, Montgomery form with R' = 2^261 (value = x * 2^261 mod p, kept LAZILY
// in [0, 2^261), not reduced below p).  Limb bounds are part of every function's contract:
//   "tight"  every limb < 2^29   (products' outputs, f29_carry outputs, converted inputs)
//   "loose"  every limb < 2^31   (limb-wise sums / differences of tight values)
// f29_mul needs one operand tight and the other loose (or both with limbs < 2^30): 9 * 2^60 + 9 * 2^58
// + carry < 2^64.  Its output value is a*b / 2^261 + (< p): limbs 0..7 are always tight, the top limb is tight when
// a*b < 2^261 (2^261 - p), e.g. both operands < 2^261 and one < 2^260 (two all-ones tight operands give a top limb >= 2^29).  Nothing at the C ABI changes: values cross into this layer with f29_from_mont256
// (x * 2^256 -> x * 2^261 is a 5-bit shift, folded into the limb repacking) and leave it with
// f29_to_mont256 (one product with 2^256, then a canonical reduction).
//
// Two entry points to the product.  f29_mul keeps the contract above.  f29_mul30 is the product of the hot loops, whose operands
// are always carried first: it needs 9 * la * lb + 5 * 2^58 + carry < 2^63 for la, lb the largest limbs of a and b - tight x
// (limbs < 2^30) fits, tight x loose and 2^30 x 2^30 do NOT.  On the moduli that are 1 mod 2^29 (both Pasta fields) it runs
// the blocks of field29_mul_asm_p1.cuh, which carry the accumulator one below its true value through the reduction columns and so
// drop the nine mads by modulus limb 0: 126 mads per product, 90 per squaring, the same limbs out (gen_field29_asm.py, gen_mul).
// f29_sqr30 (operand tight) and dot29_finish2 (rows of at most two tight terms) take the same form.  On every other modulus the
// three are the plain functions.  -DLURK_F29_P1=0 compiles the plain form everywhere (A/B runs).
//
// Signed operands (same moduli): f29_mul_s, f29_sqr_s and dot29_row2_s take limbs that are signed 32-bit values.  Contract, stated in
// full and asserted at "signed operands" below: limbs 0..7 in (-2^29, 2^29) and the top limb in (-2^30, 2^30); every column of a
// product or a two-term row then has magnitude below 2^63; |a b| < 2^522 gives limbs 0..7 tight, a signed top limb, |t| < 2^261 + p.
#pragma once
#include "field.cuh"

#ifndef LURK_F29_P1
#define LURK_F29_P1 1
#endif

// LURK_F29_CHECK (host builds of the test harness only): every limb / accumulator bound the radix-2^29
// code relies on is asserted at run time.
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
#include <cstdio>
#include <cstdlib>
#define F29_CHECKS_ACTIVE 1
#define F29_ASSERT_LIMBS(v, bits, what)                                                        \
    do {                                                                                       \
        for (int _i = 0; _i < 9; _i++)                                                         \
            if ((uint64_t)(v).l[_i] >> (bits)) { printf("F29 bound violated: %s limb %d = %u (>= 2^%d)\n", what, _i, (v).l[_i], bits); abort(); } \
    } while (0)
#define F29_ASSERT(cond, what)                                                                 \
    do {                                                                                       \
        if (!(cond)) { printf("F29 bound violated: %s\n", what); abort(); }                     \
    } while (0)
#define F29_ASSERT_TOP(v, bits, what)                                                          \
    do {                                                                                       \
        if ((uint64_t)(v).l[8] >> (bits)) { printf("F29 bound violated: %s top limb = %u (>= 2^%d)\n", what, (v).l[8], bits); abort(); } \
    } while (0)
#else
#define F29_ASSERT_LIMBS(v, bits, what) ((void)0)
#define F29_ASSERT_TOP(v, bits, what) ((void)0)
#define F29_ASSERT(cond, what) ((void)0)
#define F29_CHECKS_ACTIVE 0
#endif


namespace lurk {

template <class P>
struct F29 {
    uint32_t l[9];
};

constexpr uint32_t F29_MASK = (1u << 29) - 1u;

// modulus limbs in radix 2^29 (constexpr from the 8 x 32 description)
template <class P>
LURK_HD constexpr uint32_t f29_mod(int i) {
    // bits [29 i, 29 i + 29) of the 256-bit modulus
    const int bit = 29 * i, limb = bit >> 5, sh = bit & 31;
    uint64_t v = limb < 8 ? P::mod(limb) : 0u;
    if (limb + 1 < 8) v |= (uint64_t)P::mod(limb + 1) << 32;
    return (uint32_t)(v >> sh) & F29_MASK;
}
template <class P>
LURK_HD constexpr uint32_t f29_inv() {  // -p^-1 mod 2^29 (from the 32-bit constant)
    return P::INV & F29_MASK;
}

// The Pasta primes are 2^254 + eps with eps < 2^126 and p == 1 mod 2^29; shortcuts here and in curve29.cuh lean on that shape.  The
// BN254 primes (0.756 * 2^254, no zero limbs, p != 1 mod 2^29) take the general forms.
template <class P>
LURK_HD constexpr bool f29_pasta_shape() {
    return P::NBITS == 255 && f29_mod<P>(0) == 1u && f29_mod<P>(5) == 0u && f29_mod<P>(6) == 0u && f29_mod<P>(7) == 0u;
}
// the reduction that carries its accumulator one below the true value (f29_mul30, f29_sqr30, dot29_finish2) applies
template <class P>
LURK_HD constexpr bool f29_p1_form() {
    return LURK_F29_P1 != 0 && f29_pasta_shape<P>() && f29_inv<P>() == F29_MASK;
}

template <class P>
LURK_HD F29<P> f29_zero() {
    F29<P> z;
#pragma unroll
    for (int i = 0; i < 9; i++) z.l[i] = 0;
    return z;
}

// one carry pass: loose -> tight limbs (value unchanged; the top limb keeps everything above bit 232)
template <class P>
LURK_HD F29<P> f29_carry(const F29<P>& a) {
    F29<P> r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t x = a.l[i] + c;  // < 2^31 + 2^3
        r.l[i] = x & F29_MASK;
        c = x >> 29;
    }
    r.l[8] = a.l[8] + c;
    return r;
}

// limb-wise sum (tight + tight -> limbs < 2^30; tight + loose -> loose only if the caller knows the bound)
template <class P>
LURK_HD F29<P> f29_add(const F29<P>& a, const F29<P>& b) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}
// BIAS = 64p with its limbs re-balanced so that limbs 0..7 lie in [2^30, 2^30 + 2^29) and the top limb is
// ~2^28: limb_i += 2^30 and limb_{i+1} -= 2 (2^30 * 2^(29 i) = 2 * 2^(29 (i+1))).  Subtracting limb-wise any
// b whose limbs are at most the bias's never underflows: limbs 0..7 <= 2^30 - 2, and the top limb at most 2^28 - 2 (Pasta) or
// 0xc19139a (both BN254 fields), e.g. b tight with value < 2^259.5.
template <class P>
LURK_HD constexpr uint32_t f29_bias(int i) {
    uint64_t carry = 0;
    uint32_t limb = 0;
    for (int k = 0; k <= i; k++) {
        uint64_t x = (uint64_t)f29_mod<P>(k) * 64u + carry;
        limb = (uint32_t)(x & F29_MASK);
        carry = x >> 29;
        if (k == 8) limb = (uint32_t)x;  // top limb keeps the overflow (64p < 2^261)
    }
    uint32_t v = limb;
    if (i < 8) v += 1u << 30;  // lend to this limb ...
    if (i > 0) v -= 2u;        // ... what limb i-1 borrowed from it
    return v;
}
// a - b (mod p, lazily).  Contract: every limb of b at most the matching bias limb (above; asserted under LURK_F29_CHECK);
// a tight: result limbs < 2^31 (loose); a with limbs < 2^30: limbs < 2^31 + 2^29.  Value a - b + 64p <= a + 64p.
template <class P>
LURK_HD F29<P> f29_sub(const F29<P>& a, const F29<P>& b) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        F29_ASSERT(f29_bias<P>(i) >= b.l[i], "f29_sub: subtrahend limb above the bias (value >= 64p or limbs not tight)");
        r.l[i] = a.l[i] + (f29_bias<P>(i) - b.l[i]);
    }
    return r;
}
template <class P>
LURK_HD F29<P> f29_dbl(const F29<P>& a) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] << 1;
    return r;
}

// portable product (host / reference for the asm block): t = a*b / 2^261 mod p, limbs tight
template <class P>
LURK_HD F29<P> f29_mul_portable(const F29<P>& a, const F29<P>& b) {
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = 0;
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    {
        uint64_t ma = 0, mb = 0;
        for (int i = 0; i < 9; i++) { ma = a.l[i] > ma ? a.l[i] : ma; mb = b.l[i] > mb ? b.l[i] : mb; }
        // 9 products + 9 reduction terms (< 2^58 each) + the running carry must fit 64 bits
        F29_ASSERT((unsigned __int128)ma * mb * 9 + ((unsigned __int128)10 << 58) < ((unsigned __int128)1 << 64), "f29_mul column overflow");
    }
#endif
#pragma unroll
    for (int k = 0; k < 17; k++) {
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); i++) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); i <= (k - 1 < 8 ? k - 1 : 8); i++) acc += (uint64_t)m[i] * f29_mod<P>(k - i);
        if (k <= 8) {
            m[k] = ((uint32_t)acc * f29_inv<P>()) & F29_MASK;
            acc += (uint64_t)m[k] * f29_mod<P>(0);
        } else {
            t.l[k - 9] = (uint32_t)acc & F29_MASK;
        }
        acc >>= 29;
    }
    t.l[8] = (uint32_t)acc;
    return t;
}

// portable f29_mul30 (what the blocks of field29_mul_asm_p1.cuh compute, column for column): acc holds H = A - 1 through the
// reduction columns.  p_0 = 1 and -p^-1 = 2^29 - 1 give m_k = (-A) mod 2^29 = ~H mod 2^29, and A + m_k * p_0 >> 29 = ceil(A / 2^29)
// = (H >> 29) + 1 with a signed shift (H = -1 for A = 0): nothing is multiplied by p_0, and the m_k and the output limbs are
// f29_mul_portable's.  The signed shift wants every reduction column below 2^63.
template <class P>
LURK_HD F29<P> f29_mul30_portable(const F29<P>& a, const F29<P>& b) {
    if constexpr (!f29_p1_form<P>()) {
        return f29_mul_portable<P>(a, b);
    } else {
        uint32_t m[9];
        F29<P> t;
        uint64_t acc = ~(uint64_t)0;
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
        {
            uint64_t ma = 0, mb = 0;
            for (int i = 0; i < 9; i++) { ma = a.l[i] > ma ? a.l[i] : ma; mb = b.l[i] > mb ? b.l[i] : mb; }
            // 9 products + 5 reduction terms (< 2^58 each: modulus limbs 1..4 and 8) + the running carry (< 2^36) below 2^63
            F29_ASSERT((unsigned __int128)ma * mb * 9 + ((unsigned __int128)5 << 58) + ((unsigned __int128)1 << 36) < ((unsigned __int128)1 << 63), "f29_mul column overflow");
        }
#endif
#pragma unroll
        for (int k = 0; k < 17; k++) {
#pragma unroll
            for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); i++) acc += (uint64_t)a.l[i] * b.l[k - i];
#pragma unroll
            for (int i = (k > 8 ? k - 8 : 0); i <= (k - 1 < 8 ? k - 1 : 8); i++) acc += (uint64_t)m[i] * f29_mod<P>(k - i);
            if (k <= 8) {
                F29_ASSERT((int64_t)acc >= -1, "f29_mul column overflow");
                m[k] = ~(uint32_t)acc & F29_MASK;
                acc = (uint64_t)((int64_t)acc >> 29);
                if (k == 8) acc += 1;
            } else {
                t.l[k - 9] = (uint32_t)acc & F29_MASK;
                acc >>= 29;
            }
        }
        t.l[8] = (uint32_t)acc;
        return t;
    }
}

// ---- signed operands (the moduli of f29_p1_form only): the products of xyzz29_madd_s (curve29.cuh) ------------------------------
// A limb is an int32 held in the uint32 of F29 (two's complement).  Operand classes:
//   "s-tight"  limbs 0..7 in [0, 2^29), the top limb signed and keeping the rest: what a signed product, a signed row or
//              f29_carry_s gives; every unsigned tight value with a top limb below 2^30 is one
//   "s-diff"   limbs 0..7 in (-2^29, 2^29), top limb signed: the limb-wise difference of two s-tight values, or the limb-wise
//              negation of one - no bias is added and no carry pass follows
// and in both the top limb lies in (-2^30, 2^30): |value| < 2^262.  F29S_ASSERT_OPERAND asserts exactly this.
// Columns: a column of a product holds at most 7 terms below 2^58 and 2 with a top limb below 2^59 (column 16 is top x top alone,
// below 2^60), a two-term row twice that: with the five reduction terms (m_k < 2^29 times modulus limbs 1..4 and 8) and the carry
// from the column below, |column| < 22 * 2^58 + 5 * 2^58 + 2^36 < 2^63, which the signed shifts need.  The operand-by-operand
// products are signed (v_mad_i64_i32), the m_k * modulus limb ones unsigned onto the same 64-bit two's complement accumulator.
// The form is f29_mul30_portable's: H = A - 1 is carried through the reduction columns; m_k = (-A) mod 2^29 = ~H mod 2^29 and
// (A + m_k) / 2^29 - 1 = ceil(A / 2^29) - 1 = H >> 29 hold for negative A as well when the shift is arithmetic.
// Values: t = (a b + m p) / 2^261 with 0 <= m < 2^261, so a b / 2^261 <= t < a b / 2^261 + p; |a b| < 2^522 gives |t| < 2^261 + p
// and a top limb in [-2^29, 2^29 + 2^22].  The output is s-tight.
#if F29_CHECKS_ACTIVE
#define F29S_ASSERT_OPERAND(v, what)                                                                                                   \
    do {                                                                                                                               \
        for (int _i = 0; _i < 9; _i++) {                                                                                               \
            const int64_t _l = (int32_t)(v).l[_i], _b = (int64_t)1 << (_i < 8 ? 29 : 30);                                             \
            if (_l <= -_b || _l >= _b) { printf("F29 bound violated: %s limb %d = %lld (signed operand class)\n", what, _i, (long long)_l); abort(); } \
        }                                                                                                                              \
    } while (0)
#else
#define F29S_ASSERT_OPERAND(v, what) ((void)0)
#endif
template <class P>
LURK_HD F29<P> f29_mul_s_portable(const F29<P>& a, const F29<P>& b) {
    static_assert(f29_p1_form<P>(), "the signed products exist for the moduli that are 1 mod 2^29 only");
    F29S_ASSERT_OPERAND(a, "f29_mul_s a");
    F29S_ASSERT_OPERAND(b, "f29_mul_s b");
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = ~(uint64_t)0;  // H = (true accumulator) - 1
#pragma unroll
    for (int k = 0; k < 17; k++) {
#if F29_CHECKS_ACTIVE
        unsigned __int128 mag = ((unsigned __int128)5 << 58) + ((unsigned __int128)1 << 36);
        for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); i++) {
            const int64_t pr = (int64_t)(int32_t)a.l[i] * (int32_t)b.l[k - i];
            mag += (unsigned __int128)(pr < 0 ? -pr : pr);
        }
        F29_ASSERT(mag < ((unsigned __int128)1 << 63), "f29_mul_s column overflow");
#endif
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); i++) acc += (uint64_t)((int64_t)(int32_t)a.l[i] * (int32_t)b.l[k - i]);
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); i <= (k - 1 < 8 ? k - 1 : 8); i++) acc += (uint64_t)m[i] * f29_mod<P>(k - i);
        if (k <= 8) {
            m[k] = ~(uint32_t)acc & F29_MASK;
            acc = (uint64_t)((int64_t)acc >> 29);
            if (k == 8) acc += 1;
        } else {
            t.l[k - 9] = (uint32_t)acc & F29_MASK;
            acc = (uint64_t)((int64_t)acc >> 29);
        }
    }
    F29_ASSERT((int64_t)acc >= -((int64_t)1 << 29) && (int64_t)acc <= ((int64_t)1 << 29) + ((int64_t)1 << 22), "f29_mul_s: |a b| >= 2^522");
    t.l[8] = (uint32_t)acc;
    return t;
}
template <class P>
LURK_HD F29<P> f29_sqr_s_portable(const F29<P>& a) {  // (the squaring block issues the cross products once against 2a: the same columns)
    return f29_mul_s_portable<P>(a, a);
}

}  // namespace lurk
#include "field29_mul_asm.cuh"
#include "field29_mul_asm_bn254fq.cuh"
#include "field29_mul_asm_p1.cuh"
#include "field29_mul_asm_p1s.cuh"
namespace lurk {

// the signed products (contract above); Pasta fields only
template <class P>
LURK_HD F29<P> f29_mul_s(const F29<P>& a, const F29<P>& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return f29_mul_s_asm<P>(a, b);
#else
    return f29_mul_s_portable<P>(a, b);
#endif
}
template <class P>
LURK_HD F29<P> f29_sqr_s(const F29<P>& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return f29_sqr_s_asm<P>(a);
#else
    return f29_sqr_s_portable<P>(a);
#endif
}

// one operand tight and the other loose, or both with limbs < 2^30
template <class P>
LURK_HD F29<P> f29_mul(const F29<P>& a, const F29<P>& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return f29_mul_asm<P>(a, b);
#else
    return f29_mul_portable<P>(a, b);
#endif
}
// the narrower contract (top of the file): 9 * la * lb + 5 * 2^58 + carry < 2^63, e.g. a tight and every limb of b < 2^30
template <class P>
LURK_HD F29<P> f29_mul30(const F29<P>& a, const F29<P>& b) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (f29_p1_form<P>()) return f29_mul_p1_asm<P>(a, b);
    else return f29_mul_asm<P>(a, b);
#else
    return f29_mul30_portable<P>(a, b);
#endif
}
// a must be tight, or have limbs < 2^30 at most (the squaring block multiplies a by its doubled copy)
template <class P>
LURK_HD F29<P> f29_sqr(const F29<P>& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return f29_sqr_asm<P>(a);
#else
    return f29_mul_portable<P>(a, a);
#endif
}
// a must be tight: the square under f29_mul30's contract (the doubled copy has limbs < 2^30)
template <class P>
LURK_HD F29<P> f29_sqr30(const F29<P>& a) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (f29_p1_form<P>()) return f29_sqr_p1_asm<P>(a);
    else return f29_sqr_asm<P>(a);
#else
    return f29_mul30_portable<P>(a, a);
#endif
}

// a^(p-2): the inverse in the Montgomery(2^261) domain (0 -> 0).  a tight with value < 2^260 (the squarings then stay below
// 2^259 + p; from about 2^261 on they grow without bound); result tight.  Square-and-multiply over the bits of
// p - 2, the same in every lane: 254 squarings and one product per set bit (the Pasta primes are 2^254 + a 126-bit tail, so ~65).
// On a lane this is ~0.15 ms where the 8 x 32 fe_inv takes ~0.6 (one wave per SIMD, dependent products).
template <class P>
LURK_HD F29<P> f29_invert(const F29<P>& a) {
    uint32_t e[8];
    uint32_t borrow = 2;
    for (int i = 0; i < 8; i++) {
        const uint64_t x = (uint64_t)P::mod(i) - borrow;
        e[i] = (uint32_t)x;
        borrow = (uint32_t)(x >> 63);
    }
    int top = 255;
    while (top > 0 && !((e[top >> 5] >> (top & 31)) & 1u)) top--;
    F29<P> acc = a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int b = top - 1; b >= 0; b--) {
        acc = f29_sqr30<P>(acc);
        if ((e[b >> 5] >> (b & 31)) & 1u) acc = f29_mul30<P>(acc, a);
    }
    return acc;
}

// ---- lazy inner products: sum_i a_i * b_i with ONE Montgomery reduction -------------------------------
// 17 unreduced 64-bit column sums take the 81 partial products of every term with no carry handling; 45
// products of tight limbs (< 2^58 each) fit a column together with the reduction's own terms.
template <class P>
struct Dot29 {
    uint64_t c[17];
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    unsigned __int128 shadow[17];  // exact column sums: the 64-bit ones must never wrap
#endif
};
template <class P>
LURK_HD void dot29_init(Dot29<P>& A) {
#pragma unroll
    for (int k = 0; k < 17; k++) A.c[k] = 0;
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    for (int k = 0; k < 17; k++) A.shadow[k] = 0;
#endif
}
// A += a * b  (both tight: 81 products of < 2^58)
template <class P>
LURK_HD void dot29_mac(Dot29<P>& A, const F29<P>& a, const F29<P>& b) {
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j < 9; j++) A.c[i + j] += (uint64_t)a.l[i] * b.l[j];
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) A.shadow[i + j] += (unsigned __int128)a.l[i] * b.l[j];
    // room for the reduction's own terms (9 products < 2^58 + carry) must remain
    for (int k = 0; k < 17; k++) F29_ASSERT(A.shadow[k] + ((unsigned __int128)10 << 58) < ((unsigned __int128)1 << 64), "dot29 column overflow");
#endif
}
// push every column's excess above 29 bits into the next column (value unchanged)
template <class P>
LURK_HD void dot29_carry(Dot29<P>& A) {
#pragma unroll
    for (int k = 0; k < 16; k++) {
        A.c[k + 1] += A.c[k] >> 29;
        A.c[k] &= F29_MASK;
    }
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    for (int k = 0; k < 17; k++) A.shadow[k] = A.c[k];
#endif
}
// t = A / 2^261 mod p, tight, value < A / 2^261 + p
template <class P>
LURK_HD F29<P> dot29_finish(const Dot29<P>& A) {
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = 0;
#pragma unroll
    for (int k = 0; k < 17; k++) {
        acc += A.c[k];
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); i <= (k - 1 < 8 ? k - 1 : 8); i++) acc += (uint64_t)m[i] * f29_mod<P>(k - i);
        if (k <= 8) {
            m[k] = ((uint32_t)acc * f29_inv<P>()) & F29_MASK;
            acc += (uint64_t)m[k] * f29_mod<P>(0);
        } else {
            t.l[k - 9] = (uint32_t)acc & F29_MASK;
        }
        acc >>= 29;
    }
    t.l[8] = (uint32_t)acc;
    return t;
}

// dot29_finish for a row of at most TWO products of tight operands (18 * 2^58 per column: the Y3 rows of curve29.cuh).  Every
// column plus the reduction's own terms stays below 2^63, so the moduli that are 1 mod 2^29 take the form of f29_mul30_portable:
// nothing is multiplied by modulus limb 0.  The same limbs out as dot29_finish.
template <class P>
LURK_HD F29<P> dot29_finish2(const Dot29<P>& A) {
    if constexpr (!f29_p1_form<P>()) {
        return dot29_finish<P>(A);
    } else {
        uint32_t m[9];
        F29<P> t;
        uint64_t acc = ~(uint64_t)0;  // H = (true accumulator) - 1
#if defined(LURK_F29_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
        for (int k = 0; k < 17; k++)
            F29_ASSERT(A.shadow[k] + ((unsigned __int128)5 << 58) + ((unsigned __int128)1 << 36) < ((unsigned __int128)1 << 63), "dot29 column overflow");
#endif
#pragma unroll
        for (int k = 0; k < 17; k++) {
            acc += A.c[k];
#pragma unroll
            for (int i = (k > 8 ? k - 8 : 0); i <= (k - 1 < 8 ? k - 1 : 8); i++) acc += (uint64_t)m[i] * f29_mod<P>(k - i);
            if (k <= 8) {
                F29_ASSERT((int64_t)acc >= -1, "dot29 column overflow");
                m[k] = ~(uint32_t)acc & F29_MASK;
                acc = (uint64_t)((int64_t)acc >> 29);
                if (k == 8) acc += 1;
            } else {
                t.l[k - 9] = (uint32_t)acc & F29_MASK;
                acc >>= 29;
            }
        }
        t.l[8] = (uint32_t)acc;
        return t;
    }
}

// The two-term row of signed operands (the Y3 row of xyzz29_madd_s): a * b + c * d with ONE reduction, the contract of
// f29_mul_s_portable (every |column| < 2^63, asserted; |a b + c d| < 2^522 gives an s-tight t with |t| < 2^261 + p).  Compiled
// from this text on the device too: the signed 32 x 32 + 64 products become v_mad_i64_i32, 162 + 45 mads.
template <class P>
LURK_HD F29<P> dot29_row2_s(const F29<P>& a, const F29<P>& b, const F29<P>& c, const F29<P>& d) {
    static_assert(f29_p1_form<P>(), "the signed row exists for the moduli that are 1 mod 2^29 only");
    F29S_ASSERT_OPERAND(a, "dot29_row2_s a");
    F29S_ASSERT_OPERAND(b, "dot29_row2_s b");
    F29S_ASSERT_OPERAND(c, "dot29_row2_s c");
    F29S_ASSERT_OPERAND(d, "dot29_row2_s d");
    uint64_t col[17];
#pragma unroll
    for (int k = 0; k < 17; k++) col[k] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++)
#pragma unroll
        for (int j = 0; j < 9; j++)
            col[i + j] += (uint64_t)((int64_t)(int32_t)a.l[i] * (int32_t)b.l[j]) + (uint64_t)((int64_t)(int32_t)c.l[i] * (int32_t)d.l[j]);
#if F29_CHECKS_ACTIVE
    for (int k = 0; k < 17; k++) {
        unsigned __int128 mag = ((unsigned __int128)5 << 58) + ((unsigned __int128)1 << 36);
        for (int i = (k > 8 ? k - 8 : 0); i <= (k < 8 ? k : 8); i++) {
            const int64_t p1 = (int64_t)(int32_t)a.l[i] * (int32_t)b.l[k - i], p2 = (int64_t)(int32_t)c.l[i] * (int32_t)d.l[k - i];
            mag += (unsigned __int128)(p1 < 0 ? -p1 : p1) + (unsigned __int128)(p2 < 0 ? -p2 : p2);
        }
        F29_ASSERT(mag < ((unsigned __int128)1 << 63), "dot29_row2_s column overflow");
    }
#endif
    uint32_t m[9];
    F29<P> t;
    uint64_t acc = ~(uint64_t)0;  // H = (true accumulator) - 1
#pragma unroll
    for (int k = 0; k < 17; k++) {
        acc += col[k];
#pragma unroll
        for (int i = (k > 8 ? k - 8 : 0); i <= (k - 1 < 8 ? k - 1 : 8); i++) acc += (uint64_t)m[i] * f29_mod<P>(k - i);
        if (k <= 8) {
            m[k] = ~(uint32_t)acc & F29_MASK;
            acc = (uint64_t)((int64_t)acc >> 29);
            if (k == 8) acc += 1;
        } else {
            t.l[k - 9] = (uint32_t)acc & F29_MASK;
            acc = (uint64_t)((int64_t)acc >> 29);
        }
    }
    F29_ASSERT((int64_t)acc >= -((int64_t)1 << 29) && (int64_t)acc <= ((int64_t)1 << 29) + ((int64_t)1 << 22), "dot29_row2_s: |a b + c d| >= 2^522");
    t.l[8] = (uint32_t)acc;
    return t;
}

// 8 x 32 Montgomery(2^256) -> 9 x 29 Montgomery(2^261): value * 32, i.e. limbs of (x << 5); tight.
template <class P>
LURK_HD F29<P> f29_from_mont256(const Fe<P>& x) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i - 5;  // bit of x where limb i starts (may be negative for i = 0)
        uint64_t v;
        if (bit < 0) {
            v = (uint64_t)x.l[0] << 5;
        } else {
            const int limb = bit >> 5, sh = bit & 31;
            v = limb < 8 ? x.l[limb] : 0u;
            if (limb + 1 < 8) v |= (uint64_t)x.l[limb + 1] << 32;
            v >>= sh;
        }
        r.l[i] = (uint32_t)v & F29_MASK;
    }
    return r;
}
// plain 8 x 32 integer -> 9 x 29 limbs of the same integer (no shift); tight
template <class P>
LURK_HD F29<P> f29_from_plain(const uint32_t* x) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, limb = bit >> 5, sh = bit & 31;
        uint64_t v = limb < 8 ? x[limb] : 0u;
        if (limb + 1 < 8) v |= (uint64_t)x[limb + 1] << 32;
        r.l[i] = (uint32_t)(v >> sh) & F29_MASK;
    }
    return r;
}
// tight 9 x 29 limbs (value < 2^256 after reduction) -> 8 x 32 words
template <class P>
LURK_HD void f29_pack(const F29<P>& a, uint32_t* out) {
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const int bit = 32 * w, i = bit / 29, sh = bit % 29;
        uint64_t v = (uint64_t)a.l[i] >> sh;
        if (i + 1 < 9) v |= (uint64_t)a.l[i + 1] << (29 - sh);
        if (i + 2 < 9) v |= (uint64_t)a.l[i + 2] << (58 - sh);
        out[w] = (uint32_t)v;
    }
}
// 2^256 mod p as plain limbs: multiplying by it in the 2^261 domain divides by 32
template <class P>
LURK_HD F29<P> f29_const_r256() {
    uint32_t r[8];
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = P::r(i);
    return f29_from_plain<P>(r);
}
// lazy Montgomery(2^261) value -> canonical Montgomery(2^256) 8 x 32 (the layout of the C ABI)
template <class P>
LURK_HD Fe<P> f29_to_mont256(const F29<P>& a) {
    F29<P> u = f29_mul30<P>(f29_carry<P>(a), f29_const_r256<P>());  // a / 32: tight limbs, value < 2^255 + p < 4p
    uint32_t w[8];
    f29_pack<P>(u, w);
    fe_cond_sub2<P>(w);
    fe_cond_sub<P>(w);
    Fe<P> r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = w[i];
    return r;
}

}  // namespace lurk
