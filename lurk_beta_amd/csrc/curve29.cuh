// curve29.cuh - XYZZ mixed addition on the radix-2^29 layer (field29.cuh): the inner loop of the MSM
// bucket accumulation.  Same group law and same exceptional cases as curve.cuh::xyzz_madd; only the
// representation of the accumulator differs.  Inside the MSM pipeline results stay on this layer (Plane29
// records, below) until the last level of the bucket reduction; xyzz29_to_xyzz turns one into an ordinary
// Montgomery(2^256) XYZZ point, bit-compatible with everything outside it.
//
// Bound discipline (checked by tests/host_harness with LURK_F29_CHECK): the accumulator coordinates are
// "R-bounded" at every loop boundary: tight limbs (< 2^29, top limb < 2^27) and value < 2^259.
// Inside a mixed addition values grow through lazy subtractions (each adds the 64p bias, < 2^260); every
// such value is carried (limbs tight again) before it is multiplied, and the two stored sums X3, Y3 are
// brought back under 2^259 with f29_reduce (subtract a multiple of p read off the top limb: to below 2^255.1 for every modulus here).
// So every product of the group law has tight operands (or one with limbs < 2^30) and goes through f29_mul30 / f29_sqr30, and the
// Y3 rows (two tight terms) through dot29_finish2: reduction columns below 2^63, which the Pasta blocks without the mads by
// modulus limb 0 need (field29.cuh).  The exceptions are in the doublings, u * u (2^30 x 2^30) and m * (s - x) (tight x loose): they
// call the wide f29_mul.
//
// On the Pasta fields the task loops (msm_task_accumulate29_raw) run the mixed addition on SIGNED limbs instead, xyzz29_madd_s below:
// differences are limb-wise signed differences that are multiplied as they stand, the accumulator is "S-bounded" (limbs 0..7 tight,
// a signed top limb, |value| < 2^259) between additions, and a task's sum becomes R-bounded once, after its last addition.  Stored
// records are R-bounded under either form.  xyzz29_madd itself is still what msm_small.hip, ipa.hip, the hot-bucket share of
// msm_bucket_direct.hip and every BN254 / Grumpkin instantiation call.
#pragma once
#include "curve.cuh"
#include "field29.cuh"

#ifndef LURK_ACC_Y3_ROW
#define LURK_ACC_Y3_ROW 1
#endif
#ifndef LURK_ACC_AFFINE_FIRST
#define LURK_ACC_AFFINE_FIRST 1
#endif
// how the two rare doubling branches are compiled (out of line by default: see xyzz29_double_affine)
#ifndef LURK_F29_RARE_ATTR
#define LURK_F29_RARE_ATTR __attribute__((noinline))
#endif

namespace lurk {

// signed carry pass: limbs are int32 in (-2^31, 2^31); result tight, top limb keeps the rest (must be >= 0)
template <class P>
LURK_HD F29<P> f29_carry_signed(const int32_t* t) {
    F29<P> r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int32_t x = t[i] + c;
        r.l[i] = (uint32_t)x & F29_MASK;
        c = x >> 29;  // arithmetic shift
    }
    r.l[8] = (uint32_t)(t[8] + c);
    return r;
}

// (f29_pasta_shape, which two shortcuts below lean on, is field29.cuh's)

// v (tight limbs, top limb any u32 < 2^31) -> equivalent value < 2^255.1 with tight limbs.
// Pasta: p = 2^254 + eps, eps < 2^126 (limbs 0..4), so  v - k p = (v mod 2^254) - k eps  with k = v >> 254;
// adding p once keeps it positive:  (v mod 2^254) + 2^254 - (k - 1) eps.
template <class P>
LURK_HD F29<P> f29_reduce_pasta(const F29<P>& v) {
    const uint32_t k = v.l[8] >> 22;                    // floor(v / 2^254)  (< 2^9)
    const uint32_t km1 = k ? k - 1 : 0;                 // k = 0: value is already < 2^254, add nothing, subtract nothing
    // e = (k-1) * eps as normalised 29-bit limbs (eps limbs = modulus limbs 0..4)
    int32_t t[9];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        c += (uint64_t)km1 * f29_mod<P>(i);
        t[i] = (int32_t)v.l[i] - (int32_t)((uint32_t)c & F29_MASK);
        c >>= 29;
    }
    t[5] = (int32_t)v.l[5] - (int32_t)(uint32_t)c;      // remaining carry of (k-1) eps (< 2^9)
    t[6] = (int32_t)v.l[6];
    t[7] = (int32_t)v.l[7];
    t[8] = (int32_t)(v.l[8] & ((1u << 22) - 1u)) + (k ? (int32_t)(1u << 22) : 0);
    return f29_carry_signed<P>(t);
}
// Any modulus of 253 or 254 bits: v - q p with q an under-estimate of floor(v / p) taken from the top limb alone.  With T = v.l[8]
// (= floor(v / 2^232) < 2^31) and D = (p >> 232) + 1 (so D 2^232 > p), q = floor(T mu / 2^53), mu = floor(2^53 / D):
//   q <= T / D <= v / p                         the difference is never negative;
//   q >  T / D - 2  (T mu / 2^53 > T / D - T / 2^53, one more for the floor) and T > v / 2^232 - 1, hence
//   v - q p < v (1 - p / (D 2^232)) + p / D + 2 p <= v / D + p / D + 2 p < 2^263 / 2^21 + 2^233 + 2 p < 2^255.1   (D > 2^21, 2 p < 2^255).
// q < 2^10, so q p's running carry stays below 2^39; the limb differences are in (-2^29, 2^29) and the top one in (-2^31, 2^31).
template <class P>
LURK_HD F29<P> f29_reduce_general(const F29<P>& v) {
    constexpr uint32_t D = (P::mod(7) >> 8) + 1u;                       // bits 232.. of p, rounded up
    static_assert(D > (1u << 21) && D <= (1u << 22), "f29_reduce_general: the modulus must have 253 or 254 bits");
    constexpr uint64_t mu = ((uint64_t)1 << 53) / D;                    // < 2^32
    F29_ASSERT(v.l[8] < (1u << 31), "f29_reduce: top limb >= 2^31");
    const uint32_t q = (uint32_t)(((uint64_t)v.l[8] * mu) >> 53);
    int32_t t[9];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)q * f29_mod<P>(i);
        t[i] = (int32_t)v.l[i] - (int32_t)((uint32_t)c & F29_MASK);
        c >>= 29;
    }
    c += (uint64_t)q * f29_mod<P>(8);
    t[8] = (int32_t)v.l[8] - (int32_t)(uint32_t)c;                      // >= the borrows of the limbs below: v - q p >= 0
    const F29<P> r = f29_carry_signed<P>(t);
    F29_ASSERT(r.l[8] < (1u << 24), "f29_reduce: result not below 2^256");
    return r;
}
template <class P>
LURK_HD F29<P> f29_reduce(const F29<P>& v) {
    if constexpr (f29_pasta_shape<P>()) return f29_reduce_pasta<P>(v);
    else return f29_reduce_general<P>(v);
}

template <class P>
struct Xyzz29 {
    F29<P> x, y, zz, zzz;
};

template <class P>
LURK_HD Xyzz<P> xyzz29_to_xyzz(const Xyzz29<P>& a, bool is_identity) {
    if (is_identity) return xyzz_identity<P>();
    Xyzz<P> r;
    r.x = f29_to_mont256<P>(a.x);
    r.y = f29_to_mont256<P>(a.y);
    r.zz = f29_to_mont256<P>(a.zz);
    r.zzz = f29_to_mont256<P>(a.zzz);
    return r;
}
template <class P>
LURK_HD void xyzz29_from_xyzz(const Xyzz<P>& a, Xyzz29<P>& r, bool& is_identity) {
    is_identity = xyzz_is_identity<P>(a);
    r.x = f29_from_mont256<P>(a.x);
    r.y = f29_from_mont256<P>(a.y);
    r.zz = f29_from_mont256<P>(a.zz);
    r.zzz = f29_from_mont256<P>(a.zzz);
}

// value == 0 mod p ?  for a carried value v < 2^261, so v = k p with k < 256 (128 for the Pasta primes).  k is read off the lowest
// limb: k = v.l[0] * p^-1 mod 2^29 (Pasta: p == 1 mod 2^29, k = v.l[0]).  f29_maybe_multiple_of_p is the cheap pre-filter (almost
// every value fails it), f29_is_multiple_of_p the exact comparison behind it.
template <class P>
LURK_HD uint32_t f29_multiple_candidate(const F29<P>& v) {
    if constexpr (f29_pasta_shape<P>()) return v.l[0];
    else return (v.l[0] * ((0u - f29_inv<P>()) & F29_MASK)) & F29_MASK;  // -(-p^-1) = p^-1 mod 2^29
}
template <class P>
LURK_HD bool f29_maybe_multiple_of_p(const F29<P>& v) {
    return f29_multiple_candidate<P>(v) < (f29_pasta_shape<P>() ? 128u : 256u);
}
template <class P>
LURK_HD bool f29_is_multiple_of_p(const F29<P>& v) {
    const uint32_t k = f29_multiple_candidate<P>(v);
    uint64_t c = 0;
    bool eq = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (uint64_t)k * f29_mod<P>(i);
        eq = eq && (v.l[i] == ((uint32_t)c & F29_MASK));
        c >>= 29;
    }
    c += (uint64_t)k * f29_mod<P>(8);
    return eq && (uint64_t)v.l[8] == c;
}

// exceptional case of the mixed addition: acc and (+/-)q share their x and y, the sum is 2(+/-q): affine
// doubling (a = 0 on the Pasta curves, BN254 G1 and Grumpkin).  Rare, so out of line; arguments and result by value so that the
// caller's accumulator never has its address taken (it must stay in registers).
template <class P>
LURK_HD LURK_F29_RARE_ATTR Xyzz29<P> xyzz29_double_affine(F29<P> qx, F29<P> qy_signed) {
    const F29<P> u = f29_dbl<P>(qy_signed);                      // limbs < 2^30, value < 2^260
    const F29<P> v = f29_mul<P>(u, u);                             // < 2^259 + p  (2^30 x 2^30: the wide product)
    const F29<P> w = f29_mul30<P>(u, v);
    const F29<P> s = f29_mul30<P>(qx, v);
    const F29<P> xx = f29_sqr30<P>(qx);
    const F29<P> m = f29_carry<P>(f29_add<P>(f29_dbl<P>(xx), xx));  // 3 x^2, tight
    const F29<P> m2 = f29_sqr30<P>(m);
    Xyzz29<P> r;
    r.x = f29_reduce<P>(f29_carry<P>(f29_sub<P>(m2, f29_dbl<P>(s))));
    const F29<P> t1 = f29_mul<P>(m, f29_sub<P>(s, r.x));            // tight x loose: the wide product
    const F29<P> t2 = f29_mul30<P>(w, qy_signed);
    r.y = f29_reduce<P>(f29_carry<P>(f29_sub<P>(t1, t2)));
    r.zz = v;
    r.zzz = w;
    return r;
}

// acc += (+/-) q.  q is the 64-byte table record (Montgomery 2^256 limbs); acc_id tracks the identity.
// ACC_AFFINE: the caller knows zz = zzz = 1 (the accumulator holds exactly one base so far), which saves the four
// products with zz / zzz: 4 M + 2 S instead of 8 M + 2 S.  Every task's first real addition is of this kind, and the
// loop position is the same in all lanes of a wave, so the specialisation costs no divergence.
template <class P, bool ACC_AFFINE = false>
LURK_HD void xyzz29_madd(Xyzz29<P>& acc, bool& acc_id, const Affine<P>& q, bool negate) {
    if (affine_is_identity<P>(q)) return;
    const F29<P> qx = f29_from_mont256<P>(q.x);  // 32 x~ < 2^259, tight
    const F29<P> qy = f29_from_mont256<P>(q.y);
    if (acc_id) {
        acc.x = qx;
        acc.y = negate ? f29_reduce<P>(f29_carry<P>(f29_sub<P>(f29_zero<P>(), qy))) : qy;  // 64p - y, brought under 2^255.1
        Fe<P> one = fe_one<P>();
        acc.zz = f29_from_mont256<P>(one);
        acc.zzz = acc.zz;
        acc_id = false;
        return;
    }
    F29_ASSERT_LIMBS(acc.x, 29, "acc.x"); F29_ASSERT_TOP(acc.x, 27, "acc.x");
    F29_ASSERT_LIMBS(acc.y, 29, "acc.y"); F29_ASSERT_TOP(acc.y, 27, "acc.y");
    F29_ASSERT_LIMBS(acc.zz, 29, "acc.zz"); F29_ASSERT_TOP(acc.zz, 27, "acc.zz");
    F29_ASSERT_LIMBS(acc.zzz, 29, "acc.zzz"); F29_ASSERT_TOP(acc.zzz, 27, "acc.zzz");
    const F29<P> u2 = ACC_AFFINE ? qx : f29_mul30<P>(qx, acc.zz);    // < 2^257.2  (affine: < 2^259)
    const F29<P> s2 = ACC_AFFINE ? qy : f29_mul30<P>(qy, acc.zzz);
    const F29<P> p = f29_carry<P>(f29_sub<P>(u2, acc.x));  // U2 - X1 + 64p  < 2^260.3
    // r = S2 - Y1 for +q; for -q the true r is -(S2 + Y1): keep r' = S2 + Y1 and flip the sign of (Q - X3) below
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        F29_ASSERT(f29_bias<P>(i) >= acc.y.l[i], "madd: Y1 limb above the bias");
        r.l[i] = s2.l[i] + (negate ? acc.y.l[i] : f29_bias<P>(i) - acc.y.l[i]);
    }
    r = f29_carry<P>(r);
    if (f29_maybe_multiple_of_p<P>(p) && f29_is_multiple_of_p<P>(p)) {
        if (f29_maybe_multiple_of_p<P>(r) && f29_is_multiple_of_p<P>(r)) {  // r (or r' = -r) == 0: equal points
            const F29<P> qys = negate ? f29_reduce<P>(f29_carry<P>(f29_sub<P>(f29_zero<P>(), qy))) : qy;
            acc = xyzz29_double_affine<P>(qx, qys);
        } else {
            acc_id = true;  // opposite points
        }
        return;
    }
    const F29<P> pp = f29_sqr30<P>(p);          // < 2^259.7
    const F29<P> ppp = f29_mul30<P>(p, pp);        // < 2^259.1
    const F29<P> qq = f29_mul30<P>(acc.x, pp);     // < 2^257.8
    const F29<P> r2 = f29_sqr30<P>(r);          // < 2^259.7
    // X3 = R^2 - PPP - 2Q   (two lazy subtractions: limbs < 2^32, value < 2^261.5)
    F29<P> x3 = f29_sub<P>(f29_sub<P>(r2, ppp), f29_dbl<P>(qq));
    x3 = f29_reduce<P>(f29_carry<P>(x3));        // < 2^255.1, tight
    // D = Q - X3 (or X3 - Q when r' = -r)
    F29<P> d;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        F29_ASSERT(f29_bias<P>(i) >= qq.l[i] && f29_bias<P>(i) >= x3.l[i], "madd: Q / X3 limb above the bias");
        d.l[i] = negate ? x3.l[i] + (f29_bias<P>(i) - qq.l[i]) : qq.l[i] + (f29_bias<P>(i) - x3.l[i]);
    }
#if LURK_ACC_Y3_ROW
    // Y3 = R D - Y1 PPP as ONE lazy row: R * D + (64p - Y1) * PPP, a single Montgomery reduction
    // (operands tight: 18 products of < 2^58 per column); value < 2^259.7 + p
    Dot29<P> row;
    dot29_init<P>(row);
    dot29_mac<P>(row, r, f29_carry<P>(d));
    dot29_mac<P>(row, f29_carry<P>(f29_sub<P>(f29_zero<P>(), acc.y)), ppp);
    // (the f29_reduce is not optional: in the affine-accumulator form r and p reach 2^260.6, the row 2^521.4, so Y3 can exceed
    // 64p = 2^260 and the next addition's 64p - Y1 would go negative - seen on the GPU and reproduced on the host with points
    // 640..642 of the synthetic key; in the general form Y3 stays below 2^259.96, but dropping the reduce there measured no gain)
    F29<P> y3 = f29_reduce<P>(dot29_finish2<P>(row));
#else
    const F29<P> t1 = f29_mul<P>(r, d);            // r tight (< 2^260.3), d loose (< 2^260.1): < 2^259.5
    const F29<P> t2 = f29_mul30<P>(acc.y, ppp);    // < 2^257.2
    F29<P> y3 = f29_reduce<P>(f29_carry<P>(f29_sub<P>(t1, t2)));
#endif
    acc.x = x3;
    acc.y = y3;
    if (ACC_AFFINE) {
        acc.zz = f29_reduce<P>(pp);              // < 2^255.1 (the loop invariant wants < 2^259)
        acc.zzz = f29_reduce<P>(ppp);
    } else {
        acc.zz = f29_mul30<P>(acc.zz, pp);         // < 2^257.8
        acc.zzz = f29_mul30<P>(acc.zzz, ppp);      // < 2^257.2
    }
}

// ---- the mixed addition on SIGNED limbs (Pasta fields: f29_p1_form) ---------------------------------------------------------------
// The unsigned form above pays for every difference with the 64p bias and a carry pass, and for the growth by 64p per subtraction
// with two f29_reduce.  Here a difference is the limb-wise signed difference of its operands ("s-diff", field29.cuh) and is
// multiplied as it stands by the signed product blocks; only X3, a sum of three products, takes one signed carry pass.
// Loop invariant ("S-bounded"): each accumulator coordinate is s-tight with |value| < 2^259, i.e. a top limb in [-2^27, 2^27)
// (F29S_ASSERT_ACC).  With P' = 2^254, R' = 2^261 = 128 P' and |a b / R'| + p bounding a product, one general addition gives from
// |X1|, |Y1|, |ZZ|, |ZZZ| < 32 P' and qx, qy < 32 P':  |U2|, |S2| < 9 P';  |p|, |r| < 41 P';  PP, R2 < 14.2 P';  |PPP| < 5.6 P';
// |Q| < 4.6 P';  |X3| < 14.2 + 5.6 + 9.2 = 29 P';  |D| < 33.6 P';  |Y3| < (41 * 33.6 + 32 * 5.6) / 128 + 1 < 13.2 P';
// |ZZ'| < 4.6 P', |ZZZ'| < 2.4 P': S-bounded again, and every operand of a product has |value| < 2^262 and a top limb in
// (-2^30, 2^30).  The affine + affine form (once per task) has |p|, |r| < 64 P' and would leave |X3| up to 43 P': its X3 and Y3
// leave through f29_norm_s, as every task sum does after its last addition, so that stored records stay R-bounded.
#ifndef LURK_ACC_SIGNED
#define LURK_ACC_SIGNED 1
#endif
#if F29_CHECKS_ACTIVE
#define F29S_ASSERT_ACC(v, what)                                                                                                  \
    do {                                                                                                                          \
        F29_ASSERT_LIMBS8(v, what);                                                                                               \
        const int32_t _t = (int32_t)(v).l[8];                                                                                     \
        if (_t < -(1 << 27) || _t >= (1 << 27)) { printf("F29 bound violated: %s top limb = %d (|value| >= 2^259)\n", what, _t); abort(); } \
    } while (0)
#define F29_ASSERT_LIMBS8(v, what)                                                                                                \
    do {                                                                                                                          \
        for (int _i = 0; _i < 8; _i++)                                                                                            \
            if ((v).l[_i] >> 29) { printf("F29 bound violated: %s limb %d = %u (>= 2^29)\n", what, _i, (v).l[_i]); abort(); }    \
    } while (0)
#else
#define F29S_ASSERT_ACC(v, what) ((void)0)
#define F29_ASSERT_LIMBS8(v, what) ((void)0)
#endif
// limb-wise a - b and -a on signed limbs (two's complement in the uint32 of F29): s-tight operands give an s-diff value
template <class P>
LURK_HD F29<P> f29_sub_s(const F29<P>& a, const F29<P>& b) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] - b.l[i];
    return r;
}
template <class P>
LURK_HD F29<P> f29_neg_s(const F29<P>& a) {
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = 0u - a.l[i];
    return r;
}
// signed carry pass over signed limbs in (-2^31 + 2^3, 2^31 - 2^3): s-tight, the signed top limb keeps the rest
template <class P>
LURK_HD F29<P> f29_carry_s(const F29<P>& a) {
    F29<P> r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t x = a.l[i] + c;
        r.l[i] = x & F29_MASK;
        c = (uint32_t)((int32_t)x >> 29);  // arithmetic shift
    }
    r.l[8] = a.l[8] + c;
    return r;
}
// S-bounded (or any signed-limb value with |value| < 2^260 and limbs 0..7 in (-2^30, 2^30)) -> the R-bounded representative of the
// same residue: + 64p (f29_bias: > 2^260, limbs 0..7 in [2^30, 2^30 + 2^29)) makes every limb and the value positive, below 2^261;
// one carry pass makes it tight with a top limb below 2^29, f29_reduce brings it below 2^255.1.
template <class P>
LURK_HD F29<P> f29_norm_s(const F29<P>& a) {
    F29<P> t;
#pragma unroll
    for (int i = 0; i < 9; i++) t.l[i] = a.l[i] + f29_bias<P>(i);
    const F29<P> u = f29_carry<P>(t);
    F29_ASSERT(u.l[8] < (1u << 29), "f29_norm_s: |value| >= 2^260");
    return f29_reduce<P>(u);
}
// v == 0 mod p ? for an s-diff value with |v| < 64p, so v = k p with -64 < k < 64 and, p being 1 mod 2^29, k = v mod 2^29 read off
// limb 0.  The pre-filter looks at limb 0 alone (a window of 128 residues out of 2^29); the exact comparison behind it adds 64p,
// carries and compares as the unsigned form does.
template <class P>
LURK_HD bool f29_maybe_multiple_of_p_s(const F29<P>& v) {
    return ((v.l[0] + 64u) & F29_MASK) < 128u;
}
template <class P>
LURK_HD bool f29_is_multiple_of_p_s(const F29<P>& v) {
    F29<P> t;
#pragma unroll
    for (int i = 0; i < 9; i++) t.l[i] = v.l[i] + f29_bias<P>(i);  // v + 64p, limbs in (2^29, 2^31)
    t = f29_carry<P>(t);
    F29_ASSERT(t.l[8] < (1u << 29), "f29_is_multiple_of_p_s: |v| >= 64p");
    return f29_is_multiple_of_p<P>(t);
}

// acc += (+/-) q with the accumulator S-bounded (above) before and after: the group law and the exceptional cases of xyzz29_madd.
// The sign of the base is applied once, to qy.  8 M + 2 S with the Y3 row as one reduction, as the unsigned form.
template <class P, bool ACC_AFFINE = false>
LURK_HD void xyzz29_madd_s(Xyzz29<P>& acc, bool& acc_id, const Affine<P>& q, bool negate) {
    if (affine_is_identity<P>(q)) return;
    const F29<P> qx = f29_from_mont256<P>(q.x);  // 32 x~ < 2^259, tight
    const F29<P> qy = f29_from_mont256<P>(q.y);
    const F29<P> qys = negate ? f29_neg_s<P>(qy) : qy;  // s-diff
    if (acc_id) {
        acc.x = qx;
        acc.y = negate ? f29_carry_s<P>(qys) : qy;  // s-tight, |value| < 2^259
        Fe<P> one = fe_one<P>();
        acc.zz = f29_from_mont256<P>(one);
        acc.zzz = acc.zz;
        acc_id = false;
        return;
    }
    F29S_ASSERT_ACC(acc.x, "acc.x"); F29S_ASSERT_ACC(acc.y, "acc.y"); F29S_ASSERT_ACC(acc.zz, "acc.zz"); F29S_ASSERT_ACC(acc.zzz, "acc.zzz");
    const F29<P> u2 = ACC_AFFINE ? qx : f29_mul_s<P>(qx, acc.zz);
    const F29<P> s2 = ACC_AFFINE ? qys : f29_mul_s<P>(qys, acc.zzz);
    const F29<P> p = f29_sub_s<P>(u2, acc.x);  // s-diff, |p| < 41 P' (affine form: < 64 P')
    // (affine form: S2 is qys itself, an s-diff value, so the limbs of S2 - Y1 reach (-2^30, 2^29): carried, once per task)
    const F29<P> r = ACC_AFFINE ? f29_carry_s<P>(f29_sub_s<P>(s2, acc.y)) : f29_sub_s<P>(s2, acc.y);
    if (f29_maybe_multiple_of_p_s<P>(p) && f29_is_multiple_of_p_s<P>(p)) {
        if (f29_maybe_multiple_of_p_s<P>(r) && f29_is_multiple_of_p_s<P>(r)) {  // equal points: the doubling takes a normalised y
            const F29<P> qyn = negate ? f29_reduce<P>(f29_carry<P>(f29_sub<P>(f29_zero<P>(), qy))) : qy;
            acc = xyzz29_double_affine<P>(qx, qyn);
            acc.zz = f29_reduce<P>(acc.zz);  // (2y)^2 / R' + (< p) may pass 2^259; the other three are R-bounded, hence S-bounded
        } else {
            acc_id = true;  // opposite points
        }
        return;
    }
    const F29<P> pp = f29_sqr_s<P>(p);
    const F29<P> ppp = f29_mul_s<P>(p, pp);
    const F29<P> qq = f29_mul_s<P>(acc.x, pp);
    const F29<P> r2 = f29_sqr_s<P>(r);
    // X3 = R^2 - PPP - 2Q: limbs 0..7 in (-3 * 2^29, 2^29), so one signed carry pass before it is multiplied
    F29<P> x3;
#pragma unroll
    for (int i = 0; i < 9; i++) x3.l[i] = r2.l[i] - ppp.l[i] - (qq.l[i] << 1);
    x3 = f29_carry_s<P>(x3);
    const F29<P> d = f29_sub_s<P>(qq, x3);  // s-diff
    // Y3 = R D - Y1 PPP as one signed row
    F29<P> y3 = dot29_row2_s<P>(r, d, f29_neg_s<P>(acc.y), ppp);
    if (ACC_AFFINE) {
        acc.x = f29_norm_s<P>(x3);  // |X3| < 43 P' here (the invariant wants 32 P'): once per task
        acc.y = f29_norm_s<P>(y3);
        acc.zz = f29_reduce<P>(pp);  // < 33 P', and never negative (a square's output lies in [p^2 / R', p^2 / R' + p))
        acc.zzz = f29_norm_s<P>(ppp);
    } else {
        acc.x = x3;
        acc.y = y3;
        acc.zz = f29_mul_s<P>(acc.zz, pp);
        acc.zzz = f29_mul_s<P>(acc.zzz, ppp);
    }
    F29S_ASSERT_ACC(acc.x, "acc.x out"); F29S_ASSERT_ACC(acc.y, "acc.y out"); F29S_ASSERT_ACC(acc.zz, "acc.zz out"); F29S_ASSERT_ACC(acc.zzz, "acc.zzz out");
}
// a task's sum after its last addition: the R-bounded record plane_store asks for
template <class P>
LURK_HD void xyzz29_norm_s(Xyzz29<P>& acc) {
    acc.x = f29_norm_s<P>(acc.x);
    acc.y = f29_norm_s<P>(acc.y);
    acc.zz = f29_norm_s<P>(acc.zz);
    acc.zzz = f29_norm_s<P>(acc.zzz);
}

// Doubling of an R-bounded XYZZ29 point that is not the identity (dbl-2008-s-1, a = 0: 6 M + 3 S), result R-bounded: the link of
// the doubling chains that build a window table (msm_precompute.hip).  The bounds are xyzz29_double_affine's with the two
// products by zz / zzz of xyzz29_madd; a prime-order curve has no point with y = 0.
template <class P>
LURK_HD Xyzz29<P> xyzz29_dbl(const Xyzz29<P>& a) {
    const F29<P> u = f29_dbl<P>(a.y);                            // limbs < 2^30, value < 2^260
    const F29<P> v = f29_mul<P>(u, u);                             // < 2^259 + p  (2^30 x 2^30: the wide product)
    const F29<P> w = f29_mul30<P>(u, v);
    const F29<P> s = f29_mul30<P>(a.x, v);
    const F29<P> xx = f29_sqr30<P>(a.x);
    const F29<P> m = f29_carry<P>(f29_add<P>(f29_dbl<P>(xx), xx));  // 3 x^2, tight
    const F29<P> m2 = f29_sqr30<P>(m);
    Xyzz29<P> r;
    r.x = f29_reduce<P>(f29_carry<P>(f29_sub<P>(m2, f29_dbl<P>(s))));
    const F29<P> t1 = f29_mul<P>(m, f29_sub<P>(s, r.x));            // tight x loose: the wide product
    const F29<P> t2 = f29_mul30<P>(w, a.y);
    r.y = f29_reduce<P>(f29_carry<P>(f29_sub<P>(t1, t2)));
    r.zz = f29_mul30<P>(v, a.zz);
    r.zzz = f29_mul30<P>(w, a.zzz);
    return r;
}

// Doubling of a general XYZZ29 point: only reached when two equal partial sums meet in a reduction tree - rare, so it goes
// through the 32-bit-limb group law (out of line; arguments and result by value, see xyzz29_double_affine).
template <class P>
LURK_HD LURK_F29_RARE_ATTR Xyzz29<P> xyzz29_double_general(Xyzz29<P> a) {
    const Xyzz<P> d = xyzz_dbl<P>(xyzz29_to_xyzz<P>(a, false));
    Xyzz29<P> r;
    bool id;
    xyzz29_from_xyzz<P>(d, r, id);  // a doubled point of a prime-order curve is never the identity
    return r;
}

// acc += q, both on the radix-2^29 layer (add-2008-s: 12 M + 2 S), identities tracked by the flags.  The nodes of the reduction
// trees of the small-commitment path (msm_small.hip).  Bounds as in xyzz29_madd: both inputs R-bounded (tight limbs, value < 2^259),
// the result R-bounded again; p and r are carried differences (< 2^260.3), X3 and Y3 leave through f29_reduce.
template <class P>
LURK_HD void xyzz29_add(Xyzz29<P>& acc, bool& acc_id, const Xyzz29<P>& q, bool q_id) {
    if (q_id) return;
    if (acc_id) {
        acc = q;
        acc_id = false;
        return;
    }
    F29_ASSERT_LIMBS(acc.x, 29, "add acc.x"); F29_ASSERT_TOP(acc.x, 27, "add acc.x");
    F29_ASSERT_LIMBS(acc.y, 29, "add acc.y"); F29_ASSERT_TOP(acc.y, 27, "add acc.y");
    F29_ASSERT_LIMBS(acc.zz, 29, "add acc.zz"); F29_ASSERT_TOP(acc.zz, 27, "add acc.zz");
    F29_ASSERT_LIMBS(acc.zzz, 29, "add acc.zzz"); F29_ASSERT_TOP(acc.zzz, 27, "add acc.zzz");
    F29_ASSERT_LIMBS(q.x, 29, "add q.x"); F29_ASSERT_TOP(q.x, 27, "add q.x");
    F29_ASSERT_LIMBS(q.y, 29, "add q.y"); F29_ASSERT_TOP(q.y, 27, "add q.y");
    F29_ASSERT_LIMBS(q.zz, 29, "add q.zz"); F29_ASSERT_TOP(q.zz, 27, "add q.zz");
    F29_ASSERT_LIMBS(q.zzz, 29, "add q.zzz"); F29_ASSERT_TOP(q.zzz, 27, "add q.zzz");
    const F29<P> u1 = f29_mul30<P>(acc.x, q.zz);     // < 2^257.2, tight
    const F29<P> u2 = f29_mul30<P>(q.x, acc.zz);
    const F29<P> s1 = f29_mul30<P>(acc.y, q.zzz);
    const F29<P> s2 = f29_mul30<P>(q.y, acc.zzz);
    const F29<P> p = f29_carry<P>(f29_sub<P>(u2, u1));  // U2 - U1 + 64p < 2^260.3
    const F29<P> r = f29_carry<P>(f29_sub<P>(s2, s1));
    if (f29_maybe_multiple_of_p<P>(p) && f29_is_multiple_of_p<P>(p)) {
        if (f29_maybe_multiple_of_p<P>(r) && f29_is_multiple_of_p<P>(r)) acc = xyzz29_double_general<P>(acc);  // equal points
        else acc_id = true;                                                                     // opposite points
        return;
    }
    const F29<P> pp = f29_sqr30<P>(p);               // < 2^259.7
    const F29<P> ppp = f29_mul30<P>(p, pp);          // < 2^259.1
    const F29<P> qq = f29_mul30<P>(u1, pp);          // < 2^256
    const F29<P> r2 = f29_sqr30<P>(r);               // < 2^259.7
    F29<P> x3 = f29_sub<P>(f29_sub<P>(r2, ppp), f29_dbl<P>(qq));
    x3 = f29_reduce<P>(f29_carry<P>(x3));          // < 2^255.1, tight
    F29<P> d;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        F29_ASSERT(f29_bias<P>(i) >= x3.l[i], "add: X3 limb above the bias");
        d.l[i] = qq.l[i] + (f29_bias<P>(i) - x3.l[i]);
    }
    // Y3 = R (Q - X3) - S1 PPP as one lazy row (see xyzz29_madd): value < 2^259.9 + p before the reduce
    Dot29<P> row;
    dot29_init<P>(row);
    dot29_mac<P>(row, r, f29_carry<P>(d));
    dot29_mac<P>(row, f29_carry<P>(f29_sub<P>(f29_zero<P>(), s1)), ppp);
    const F29<P> y3 = f29_reduce<P>(dot29_finish2<P>(row));
    const F29<P> zz12 = f29_mul30<P>(acc.zz, q.zz);  // < 2^257.2
    const F29<P> zzz12 = f29_mul30<P>(acc.zzz, q.zzz);
    acc.x = x3;
    acc.y = y3;
    acc.zz = f29_mul30<P>(zz12, pp);                 // < 2^256
    acc.zzz = f29_mul30<P>(zzz12, ppp);
}

// Sum of nt XYZZ points held in the 8 x 32 form (a bucket's task partials: msm_finalize.hip).  One point is copied, more go through
// the radix-2^29 general addition (6.4 us per dependent addition on a lane where the 8 x 32 group law takes ~20).
template <class P>
LURK_HD Xyzz<P> xyzz_sum_via29(const Xyzz<P>* pts, uint32_t nt) {
    if (nt == 0) return xyzz_identity<P>();
    if (nt == 1) return pts[0];
    Xyzz29<P> acc, q;
    bool acc_id, q_id;
    xyzz29_from_xyzz<P>(pts[0], acc, acc_id);
    for (uint32_t i = 1; i < nt; i++) {
        xyzz29_from_xyzz<P>(pts[i], q, q_id);
        xyzz29_add<P>(acc, acc_id, q, q_id);
    }
    return xyzz29_to_xyzz<P>(acc, acc_id);
}

// The record the MSM's stages hand each other (msm_core.cuh): a point on this layer with the identity as a flag, 160 bytes.  Task sums,
// buckets and the planes of the bucket reduction all travel in this form, so nothing between the accumulation and the last reduction
// level converts a point to the 8 x 32 form and back.
// A STORED record is R-bounded - tight limbs (< 2^29, top limb < 2^27: value < 2^259) - which is what xyzz29_add asks of its inputs:
// the copy of a first base, the outputs of xyzz29_madd / xyzz29_add and of the two doublings all are (see each).  plane_store asserts
// it under LURK_F29_CHECK; the limbs of an identity record are never read.
template <class P>
struct Plane29 {
    Xyzz29<P> p;
    uint32_t id, pad[3];
};
template <class P>
LURK_HD void plane_load(const Plane29<P>* __restrict__ src, Xyzz29<P>& v, bool& id) {
    const Plane29<P> r = *src;
    v = r.p;
    id = r.id != 0;
}
template <class P>
LURK_HD void plane_store(Plane29<P>* __restrict__ dst, const Xyzz29<P>& v, bool id) {
    if (!id) {
        F29_ASSERT_LIMBS(v.x, 29, "record x"); F29_ASSERT_TOP(v.x, 27, "record x");
        F29_ASSERT_LIMBS(v.y, 29, "record y"); F29_ASSERT_TOP(v.y, 27, "record y");
        F29_ASSERT_LIMBS(v.zz, 29, "record zz"); F29_ASSERT_TOP(v.zz, 27, "record zz");
        F29_ASSERT_LIMBS(v.zzz, 29, "record zzz"); F29_ASSERT_TOP(v.zzz, 27, "record zzz");
    }
    Plane29<P> o;
    o.p = v;
    o.id = id;
    o.pad[0] = o.pad[1] = o.pad[2] = 0;
    *dst = o;
}
template <class P>
LURK_HD void plane_store_identity(Plane29<P>* __restrict__ dst) {
    Xyzz29<P> z;
    z.x = z.y = z.zz = z.zzz = f29_zero<P>();
    plane_store<P>(dst, z, true);
}
// Sum of nt >= 1 records (the task sums of one bucket: msm_finalize.hip), a chain of general additions on this layer.
template <class P>
LURK_HD void plane_sum(const Plane29<P>* recs, uint32_t nt, Xyzz29<P>& acc, bool& acc_id) {
    plane_load<P>(recs, acc, acc_id);
    for (uint32_t i = 1; i < nt; i++) {
        Xyzz29<P> q;
        bool q_id;
        plane_load<P>(recs + i, q, q_id);
        xyzz29_add<P>(acc, acc_id, q, q_id);
    }
}

// The finalize stage's work for ONE bucket of the record array `records` (NB buckets in front, task t's sum at NB + t when its bucket is
// two or more tasks): `nt` tasks, the first of them task `first`.  Returns true when the bucket has more than `fin_small` tasks and is
// left to a workgroup (msm_finalize.hip); tests/host_bucket_records replays this on the CPU.
template <class P>
LURK_HD bool plane_finalize_bucket(Plane29<P>* records, uint32_t NB, size_t key, uint32_t nt, uint32_t first, uint32_t fin_small) {
    if (nt == 1) return false;  // the bucket IS its task's sum, stored in place by the accumulation
    if (nt == 0) {
        plane_store_identity<P>(records + key);
        return false;
    }
    if (nt > fin_small) return true;
    Xyzz29<P> acc;
    bool acc_id;
    plane_sum<P>(records + NB + first, nt, acc, acc_id);  // (reads slots behind the buckets, writes one among them)
    plane_store<P>(records + key, acc, acc_id);
    return false;
}

#if defined(__HIPCC__)
// acc <- the sum of the BLOCK accumulators of a workgroup (thread 0 holds it afterwards): a tree through LDS on 160-byte records
// (sh: BLOCK of them).  The hot buckets of msm_finalize.hip and msm_bucket_direct.hip.
template <class P, int BLOCK>
__device__ __forceinline__ void block_tree_sum29(Xyzz29<P>& acc, bool& acc_id, Plane29<P>* sh) {
    const int t = threadIdx.x;
    plane_store<P>(sh + t, acc, acc_id);
    __syncthreads();
    for (int stride = BLOCK / 2; stride >= 1; stride >>= 1) {
        if (t < stride) {
            Xyzz29<P> q;
            bool q_id;
            plane_load<P>(sh + t + stride, q, q_id);
            xyzz29_add<P>(acc, acc_id, q, q_id);
            plane_store<P>(sh + t, acc, acc_id);
        }
        __syncthreads();
    }
}
#endif

// A 64-byte table record in flight: four 16-byte words exactly as the loads return them (one global_load_dwordx4 each).  The
// pipelined task loop holds the NEXT record in this form across a whole mixed addition and turns it into an Affine<P> only when its
// turn comes: held as an Affine<P> the persistent kernel takes 194 registers, in this form it stays inside its budget of 192.
// (a GCC / clang vector type, so that hipcc keeps each word one load and g++ builds the same header for the host harness)
typedef uint32_t Rec16 __attribute__((vector_size(16), may_alias));
struct Rec64 {
    Rec16 q[4];
};
template <class P>
LURK_HD Rec64 rec64_load(const Affine<P>* table, uint32_t e) {
    static_assert(sizeof(Affine<P>) == 64 && alignof(Affine<P>) >= 16, "a table record is four aligned 16-byte words");
    const Rec16* p = reinterpret_cast<const Rec16*>(table + (e & 0x7fffffffu));
    Rec64 r;
#pragma unroll
    for (int i = 0; i < 4; i++) r.q[i] = p[i];
    return r;
}
template <class P>
LURK_HD Affine<P> rec64_affine(const Rec64& r) {
    Affine<P> a;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        a.x.l[i] = r.q[i >> 2][i & 3];
        a.y.l[i] = r.q[2 + (i >> 2)][i & 3];
    }
    return a;
}
// One step of the pipelined loop, taken in front of addition j: hands out record j (loaded one trip ago) with its sign and puts
// record j + 1 and index j + 2 in flight.  Past the end of the task the look-ahead is clamped to what was read before (index j
// again, and on the last trip the record that index names), so nothing is read beyond sorted[last - 1] or beyond the record of a
// real entry of this task; what the clamped loads return is never used.
template <class P>
LURK_HD Affine<P> msm_task_next29(const uint32_t* sorted, const Affine<P>* table, uint32_t j, uint32_t last, bool& neg_next, uint32_t& e_ahead,
                                  Rec64& rec, bool& negate) {
    const Affine<P> q = rec64_affine<P>(rec);
    negate = neg_next;
    neg_next = (e_ahead & 0x80000000u) != 0;
    rec = rec64_load<P>(table, e_ahead);         // entry j + 1 (on the last trip: an earlier entry of the task)
    e_ahead = sorted[j + 2 < last ? j + 2 : j];  // (clamped on the last two trips)
    return q;
}

// One accumulation task on the radix-2^29 layer: the signed table records sorted[first .. last) summed into (acc, acc_id), which
// leave R-bounded (both accumulate kernels and msm_bucket_direct.hip store them as Plane29 records; msm_task_accumulate29 returns them
// as an ordinary XYZZ point for the host harnesses).
// PIPELINED (the persistent kernel only): the same additions with the same arguments in the same order, the gather of record j + 1
// and the load of index j + 2 issued in front of addition j, so that the only exposed gather of a task is its first.
// the mixed addition of the task loops: the signed form on the Pasta fields (-DLURK_ACC_SIGNED=0: the unsigned one everywhere, A/B runs)
template <class P>
LURK_HD constexpr bool msm_acc_signed() {
    return LURK_ACC_SIGNED != 0 && f29_p1_form<P>();
}
template <class P, bool ACC_AFFINE = false>
LURK_HD void xyzz29_madd_task(Xyzz29<P>& acc, bool& acc_id, const Affine<P>& q, bool negate) {
    if constexpr (msm_acc_signed<P>()) xyzz29_madd_s<P, ACC_AFFINE>(acc, acc_id, q, negate);
    else xyzz29_madd<P, ACC_AFFINE>(acc, acc_id, q, negate);
}
template <class P, bool PIPELINED = false>
LURK_HD void msm_task_accumulate29_loop(const uint32_t* sorted, uint32_t first, uint32_t last, const Affine<P>* table, Xyzz29<P>& acc, bool& acc_id) {
    acc.x = acc.y = acc.zz = acc.zzz = f29_zero<P>();
    acc_id = true;
    // Every trip of the plain loop below waits for two dependent loads (sorted[j], then the 64-byte record it names: a random read
    // from a table of up to 3.25 GiB) in front of ~2 100 VALU instructions.  In the plain launch, three waves per SIMD, the other
    // waves cover that wait: gathering the next base ahead was measured THERE with no gain, and so was requesting one dword of it
    // ahead - a one-VGPR "touch" for L2 and the TLB - 3.6 against 3.5 ms (although confining every gather to a 64 MB window of the
    // 3.25 GiB table does make the kernel 8 % faster); at 162 registers the plain kernel has no room for a record in flight either
    // (16 more and it runs two waves per SIMD).  The persistent kernel of commitments in flight runs ONE wave per SIMD, whose wait
    // nothing covers, and has the room: up to 192 registers two of its launches still sit beside a 128-register tail wave
    // (tests/test_cabi_exports.py::test_sort_kernels_fit_beside_a_resident_accumulation).  It takes the PIPELINED loop: one
    // accumulation alone on the device 4.00 -> 3.53 ms at 2^22, 0.85 -> 0.97 of the plain launch's rate.
    if (PIPELINED) {
        if (first >= last) return;
        const uint32_t e_first = sorted[first];
        bool neg_next = (e_first & 0x80000000u) != 0;
        Rec64 rec = rec64_load<P>(table, e_first);
        uint32_t e_ahead = sorted[first + 1 < last ? first + 1 : first];
        uint32_t j = first;
        bool negate;
#if LURK_ACC_AFFINE_FIRST
        {  // first base: a copy (zz = zzz = 1)
            const Affine<P> q = msm_task_next29<P>(sorted, table, j, last, neg_next, e_ahead, rec, negate);
            xyzz29_madd_task<P>(acc, acc_id, q, negate);
            j++;
        }
        if (j < last) {  // second base: affine + affine (unless the first was the identity record)
            const Affine<P> q = msm_task_next29<P>(sorted, table, j, last, neg_next, e_ahead, rec, negate);
            if (!acc_id) xyzz29_madd_task<P, true>(acc, acc_id, q, negate);
            else xyzz29_madd_task<P>(acc, acc_id, q, negate);
            j++;
        }
#endif
        for (; j < last; j++) {
            const Affine<P> q = msm_task_next29<P>(sorted, table, j, last, neg_next, e_ahead, rec, negate);
            xyzz29_madd_task<P>(acc, acc_id, q, negate);
        }
        return;
    }
#if LURK_ACC_AFFINE_FIRST
    uint32_t j = first;
    if (j < last) {  // first base: a copy (zz = zzz = 1)
        const uint32_t e = sorted[j++];
        xyzz29_madd_task<P>(acc, acc_id, table[e & 0x7fffffffu], (e & 0x80000000u) != 0);
    }
    if (j < last) {  // second base: affine + affine (unless the first was the identity record)
        const uint32_t e = sorted[j++];
        const Affine<P> q = table[e & 0x7fffffffu];
#if LURK_ACC_AFFINE_FIRST
        if (!acc_id) xyzz29_madd_task<P, true>(acc, acc_id, q, (e & 0x80000000u) != 0);
        else
#endif
            xyzz29_madd_task<P>(acc, acc_id, q, (e & 0x80000000u) != 0);
    }
    for (; j < last; j++) {
        const uint32_t e = sorted[j];
        const Affine<P> q = table[e & 0x7fffffffu];
        xyzz29_madd_task<P>(acc, acc_id, q, (e & 0x80000000u) != 0);
    }
#else
    for (uint32_t j = first; j < last; j++) {
        const uint32_t e = sorted[j];
#ifdef LURK_ACC_DEBUG_TABLE_MASK  // timing experiment only (wrong results): every gather lands in a small window of the table
        const Affine<P> q = table[e & LURK_ACC_DEBUG_TABLE_MASK];
#else
        const Affine<P> q = table[e & 0x7fffffffu];
#endif
        xyzz29_madd_task<P>(acc, acc_id, q, (e & 0x80000000u) != 0);
    }
#endif
}
// In the signed form the loop leaves an S-bounded sum, normalised ONCE here, after the task's last addition.
template <class P, bool PIPELINED = false>
LURK_HD void msm_task_accumulate29_raw(const uint32_t* sorted, uint32_t first, uint32_t last, const Affine<P>* table, Xyzz29<P>& acc, bool& acc_id) {
    msm_task_accumulate29_loop<P, PIPELINED>(sorted, first, last, table, acc, acc_id);
    if constexpr (msm_acc_signed<P>()) {
        if (!acc_id) xyzz29_norm_s<P>(acc);
    }
}
template <class P, bool PIPELINED = false>
LURK_HD Xyzz<P> msm_task_accumulate29(const uint32_t* sorted, uint32_t first, uint32_t last, const Affine<P>* table) {
    Xyzz29<P> acc;
    bool acc_id;
    msm_task_accumulate29_raw<P, PIPELINED>(sorted, first, last, table, acc, acc_id);
    return xyzz29_to_xyzz<P>(acc, acc_id);
}

}  // namespace lurk
