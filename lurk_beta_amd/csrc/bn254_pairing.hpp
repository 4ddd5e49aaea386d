// bn254_pairing.hpp - the pairing-product check on BN254 and the G2 arithmetic that holds a KZG verifier key.  HOST ONLY, header only:
// it compiles with plain g++ on Fe<Bn254Fq> and the host functions of field.cuh (tests/host_pairing/main.cpp is such a build).
//
// A verification needs ONE decision, e(L, H) e(-R, [tau]H) == 1: a 65-step Miller loop and one final exponentiation over twelve-limb
// towers, a few milliseconds on one core, once per proof.  There is no kernel and there will be none.  Nothing here leaves as a GT
// element: the C ABI (bn254_pairing.hip) exposes the decision only, so any non-degenerate bilinear pairing on G1 x G2 would give the
// same answers; this one is the optimal ate pairing in the form that is easiest to get right:
//   tower     Fq2 = Fq[u]/(u^2 + 1),  Fq6 = Fq2[v]/(v^3 - xi) with xi = 9 + u,  Fq12 = Fq6[w]/(w^2 - v)   (so w^6 = xi)
//   G2        the sextic twist y^2 = x^3 + 3/xi over Fq2, AFFINE throughout (an Fq2 inversion is ~3 us on the host, a scalar multiple
//             1.4 ms); a twist point (x, y) stands for (x w^2, y w^3) on E(Fq12)
//   Miller    the loop over 6x + 2 (65 bits, plain binary), one accumulator shared by all pairs, then the two Frobenius line steps;
//             a line through T with slope lambda is  yP - lambda xP w + (lambda xT - yT) w^3  (vertical lines lie in Fq6 and die in
//             the final exponentiation: they are dropped)
//   final     the easy part by conjugation, one inversion and Frobenius^2; the hard part (p^4 - p^2 + 1)/r by plain
//             square-and-multiply over the 761-bit literal below (tests/test_bn254_pairing_cpu.py recomputes it from x)
// The Frobenius coefficients xi^(i (p-1)/6), 3/xi and the Montgomery forms of the generator are COMPUTED at first use (a function-local
// static: thread-safe), never typed in.  tests/bn254_pairing_ref.py decides the same products another way (Fq12 as Fp[w]/(w^12 - 18 w^6
// + 82), the plain ate loop over 6x^2, one pow by (p^12 - 1)/r).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (field.cuh's function qualifiers, when a .hip translation unit includes this first)
#endif
#include "field.cuh"

namespace lurk {
namespace bn254 {

typedef Fe<Bn254Fq> Fq;

// the BN parameter x: p = 36x^4 + 36x^3 + 24x^2 + 6x + 1, r = 36x^4 + 36x^3 + 18x^2 + 6x + 1
constexpr uint64_t BN_X = 0x44E992B44A6909F1ull;
// 6x + 2 = 2^64 + ATE_LOOP_LOW (65 bits)
constexpr uint64_t ATE_LOOP_LOW = 0x9D797039BE763BA8ull;
static_assert(6 * (unsigned __int128)BN_X + 2 == (((unsigned __int128)1 << 64) | ATE_LOOP_LOW), "6x + 2");
// (p^4 - p^2 + 1) / r, 761 bits
constexpr const char* HARD_EXPONENT_HEX =
    "1baaa710b0759ad331ec15183177faf6c0eb522d5b122784e529a5861876f6b3b1b1355d189227d79581e16f3fd90c66b887d56d5095f23aaa441e3954bcf8ad"
    "cc7b44c87cdbacff1154e7e1da014fd5abf5cc4f49c36d4e81bb482ccdf42b1";
constexpr int HARD_EXPONENT_LIMBS = 24;
// the generator H of the order-r subgroup of the twist (canonical, big-endian hex)
constexpr const char* G2_GEN_X0_HEX = "1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed";
constexpr const char* G2_GEN_X1_HEX = "198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2";
constexpr const char* G2_GEN_Y0_HEX = "12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa";
constexpr const char* G2_GEN_Y1_HEX = "090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b";

// big-endian hex -> little-endian 32-bit limbs (zero-extended; digits beyond nlimbs are dropped)
inline void hex_to_limbs(const char* hex, uint32_t* out, int nlimbs) {
    for (int i = 0; i < nlimbs; i++) out[i] = 0;
    const size_t len = strlen(hex);
    for (size_t k = 0; k < len; k++) {
        const char ch = hex[len - 1 - k];
        const uint32_t d = ch >= '0' && ch <= '9' ? (uint32_t)(ch - '0') : ch >= 'a' && ch <= 'f' ? (uint32_t)(ch - 'a' + 10) : (uint32_t)(ch - 'A' + 10);
        if ((int)(k / 8) < nlimbs) out[k / 8] |= d << (4 * (k % 8));
    }
}
inline Fq fq_from_hex(const char* hex) {
    Fq c;
    hex_to_limbs(hex, c.l, 8);
    return fe_to_mont<Bn254Fq>(c);
}
inline Fq fq_add(const Fq& a, const Fq& b) { return fe_add<Bn254Fq>(a, b); }
inline Fq fq_sub(const Fq& a, const Fq& b) { return fe_sub<Bn254Fq>(a, b); }
inline Fq fq_mul(const Fq& a, const Fq& b) { return fe_mul<Bn254Fq>(a, b); }
inline Fq fq_neg(const Fq& a) { return fe_neg<Bn254Fq>(a); }
inline bool fq_is_reduced(const Fq& a) { return !fe_canonical_ge_mod<Bn254Fq>(a.l); }

// ---- Fq2 = Fq[u]/(u^2 + 1) ----------------------------------------------------------------------------------------------------------------
struct Fq2 {
    Fq c0, c1;
};
inline Fq2 fq2_zero() { return Fq2{fe_zero<Bn254Fq>(), fe_zero<Bn254Fq>()}; }
inline Fq2 fq2_one() { return Fq2{fe_one<Bn254Fq>(), fe_zero<Bn254Fq>()}; }
inline bool fq2_is_zero(const Fq2& a) { return fe_is_zero<Bn254Fq>(a.c0) && fe_is_zero<Bn254Fq>(a.c1); }
inline bool fq2_eq(const Fq2& a, const Fq2& b) { return fe_eq<Bn254Fq>(a.c0, b.c0) && fe_eq<Bn254Fq>(a.c1, b.c1); }
inline Fq2 fq2_add(const Fq2& a, const Fq2& b) { return Fq2{fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)}; }
inline Fq2 fq2_sub(const Fq2& a, const Fq2& b) { return Fq2{fq_sub(a.c0, b.c0), fq_sub(a.c1, b.c1)}; }
inline Fq2 fq2_neg(const Fq2& a) { return Fq2{fq_neg(a.c0), fq_neg(a.c1)}; }
inline Fq2 fq2_dbl(const Fq2& a) { return fq2_add(a, a); }
inline Fq2 fq2_conj(const Fq2& a) { return Fq2{a.c0, fq_neg(a.c1)}; }  // the Frobenius of Fq2: u^p = -u (p = 3 mod 4)
inline Fq2 fq2_frobenius(const Fq2& a) { return fq2_conj(a); }
inline Fq2 fq2_scale(const Fq2& a, const Fq& k) { return Fq2{fq_mul(a.c0, k), fq_mul(a.c1, k)}; }
inline Fq2 fq2_mul(const Fq2& a, const Fq2& b) {  // Karatsuba: three products
    const Fq t0 = fq_mul(a.c0, b.c0), t1 = fq_mul(a.c1, b.c1);
    const Fq t2 = fq_mul(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));
    return Fq2{fq_sub(t0, t1), fq_sub(fq_sub(t2, t0), t1)};
}
inline Fq2 fq2_sqr(const Fq2& a) {  // (a0 + a1)(a0 - a1) + 2 a0 a1 u
    const Fq t = fq_mul(a.c0, a.c1);
    return Fq2{fq_mul(fq_add(a.c0, a.c1), fq_sub(a.c0, a.c1)), fq_add(t, t)};
}
inline Fq2 fq2_inv(const Fq2& a) {  // conj(a) / (a0^2 + a1^2); 0 -> 0
    const Fq n = fe_inv<Bn254Fq>(fq_add(fq_mul(a.c0, a.c0), fq_mul(a.c1, a.c1)));
    return Fq2{fq_mul(a.c0, n), fq_neg(fq_mul(a.c1, n))};
}
inline Fq2 fq2_mul_xi(const Fq2& a) {  // (9 + u)(a0 + a1 u) = (9 a0 - a1) + (9 a1 + a0) u
    const Fq2 a2 = fq2_dbl(a), a4 = fq2_dbl(a2), a9 = fq2_add(fq2_dbl(a4), a);
    return Fq2{fq_sub(a9.c0, a.c1), fq_add(a9.c1, a.c0)};
}
// a^e, e a plain integer of nlimbs 32-bit limbs
inline Fq2 fq2_pow(const Fq2& a, const uint32_t* e, int nlimbs) {
    Fq2 acc = fq2_one();
    for (int i = 32 * nlimbs - 1; i >= 0; i--) {
        acc = fq2_sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1u) acc = fq2_mul(acc, a);
    }
    return acc;
}

struct G2 {  // affine on the twist; inf = the identity (x, y then unspecified)
    Fq2 x, y;
    bool inf;
};

// ---- constants, computed once ---------------------------------------------------------------------------------------------------------
struct Consts {
    Fq2 xi;        // 9 + u
    Fq2 b_twist;   // 3 / xi
    Fq2 gamma[6];  // gamma[i] = xi^(i (p - 1) / 6): w^(i p) = gamma[i] w^i
    G2 gen;        // H
    uint32_t hard[HARD_EXPONENT_LIMBS];
};
inline Consts make_consts() {
    Consts c;
    c.xi = Fq2{fe_from_u64<Bn254Fq>(9), fe_one<Bn254Fq>()};
    c.b_twist = fq2_scale(fq2_inv(c.xi), fe_from_u64<Bn254Fq>(3));
    uint32_t e[8];  // (p - 1) / 6, by long division from the top limb
    for (int i = 0; i < 8; i++) e[i] = Bn254Fq::mod(i);
    e[0] -= 1;  // p is odd
    uint64_t rem = 0;
    for (int i = 7; i >= 0; i--) {
        const uint64_t cur = (rem << 32) | e[i];
        e[i] = (uint32_t)(cur / 6);
        rem = cur % 6;
    }
    c.gamma[0] = fq2_one();
    c.gamma[1] = fq2_pow(c.xi, e, 8);
    for (int i = 2; i < 6; i++) c.gamma[i] = fq2_mul(c.gamma[i - 1], c.gamma[1]);
    c.gen.x = Fq2{fq_from_hex(G2_GEN_X0_HEX), fq_from_hex(G2_GEN_X1_HEX)};
    c.gen.y = Fq2{fq_from_hex(G2_GEN_Y0_HEX), fq_from_hex(G2_GEN_Y1_HEX)};
    c.gen.inf = false;
    hex_to_limbs(HARD_EXPONENT_HEX, c.hard, HARD_EXPONENT_LIMBS);
    return c;
}
inline const Consts& consts() {
    static const Consts c = make_consts();
    return c;
}

// ---- Fq6 = Fq2[v]/(v^3 - xi) ------------------------------------------------------------------------------------------------------------
struct Fq6 {
    Fq2 c0, c1, c2;
};
inline Fq6 fq6_zero() { return Fq6{fq2_zero(), fq2_zero(), fq2_zero()}; }
inline Fq6 fq6_one() { return Fq6{fq2_one(), fq2_zero(), fq2_zero()}; }
inline bool fq6_eq(const Fq6& a, const Fq6& b) { return fq2_eq(a.c0, b.c0) && fq2_eq(a.c1, b.c1) && fq2_eq(a.c2, b.c2); }
inline Fq6 fq6_add(const Fq6& a, const Fq6& b) { return Fq6{fq2_add(a.c0, b.c0), fq2_add(a.c1, b.c1), fq2_add(a.c2, b.c2)}; }
inline Fq6 fq6_sub(const Fq6& a, const Fq6& b) { return Fq6{fq2_sub(a.c0, b.c0), fq2_sub(a.c1, b.c1), fq2_sub(a.c2, b.c2)}; }
inline Fq6 fq6_neg(const Fq6& a) { return Fq6{fq2_neg(a.c0), fq2_neg(a.c1), fq2_neg(a.c2)}; }
inline Fq6 fq6_mul_v(const Fq6& a) { return Fq6{fq2_mul_xi(a.c2), a.c0, a.c1}; }
inline Fq6 fq6_scale(const Fq6& a, const Fq2& k) { return Fq6{fq2_mul(a.c0, k), fq2_mul(a.c1, k), fq2_mul(a.c2, k)}; }
inline Fq6 fq6_mul(const Fq6& a, const Fq6& b) {  // Karatsuba: six products
    const Fq2 t0 = fq2_mul(a.c0, b.c0), t1 = fq2_mul(a.c1, b.c1), t2 = fq2_mul(a.c2, b.c2);
    const Fq2 m12 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c1, a.c2), fq2_add(b.c1, b.c2)), t1), t2);  // a1 b2 + a2 b1
    const Fq2 m01 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(b.c0, b.c1)), t0), t1);  // a0 b1 + a1 b0
    const Fq2 m02 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c2), fq2_add(b.c0, b.c2)), t0), t2);  // a0 b2 + a2 b0
    return Fq6{fq2_add(t0, fq2_mul_xi(m12)), fq2_add(m01, fq2_mul_xi(t2)), fq2_add(m02, t1)};
}
inline Fq6 fq6_sqr(const Fq6& a) { return fq6_mul(a, a); }
// a (b0 + b1 v): the sparse factor of a line
inline Fq6 fq6_mul_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    return Fq6{fq2_add(fq2_mul(a.c0, b0), fq2_mul_xi(fq2_mul(a.c2, b1))), fq2_add(fq2_mul(a.c0, b1), fq2_mul(a.c1, b0)),
               fq2_add(fq2_mul(a.c1, b1), fq2_mul(a.c2, b0))};
}
inline Fq6 fq6_inv(const Fq6& a) {  // (A + B v + C v^2) / (a0 A + xi (a2 B + a1 C)); 0 -> 0
    const Fq2 A = fq2_sub(fq2_sqr(a.c0), fq2_mul_xi(fq2_mul(a.c1, a.c2)));
    const Fq2 B = fq2_sub(fq2_mul_xi(fq2_sqr(a.c2)), fq2_mul(a.c0, a.c1));
    const Fq2 C = fq2_sub(fq2_sqr(a.c1), fq2_mul(a.c0, a.c2));
    const Fq2 F = fq2_add(fq2_mul(a.c0, A), fq2_mul_xi(fq2_add(fq2_mul(a.c2, B), fq2_mul(a.c1, C))));
    return fq6_scale(Fq6{A, B, C}, fq2_inv(F));
}
inline Fq6 fq6_frobenius(const Fq6& a) {  // v = w^2: v^p = gamma[2] v
    const Consts& k = consts();
    return Fq6{fq2_conj(a.c0), fq2_mul(fq2_conj(a.c1), k.gamma[2]), fq2_mul(fq2_conj(a.c2), k.gamma[4])};
}

// ---- Fq12 = Fq6[w]/(w^2 - v) ----------------------------------------------------------------------------------------------------------
// c0 + c1 w = c0.c0 + c1.c0 w + c0.c1 w^2 + c1.c1 w^3 + c0.c2 w^4 + c1.c2 w^5
struct Fq12 {
    Fq6 c0, c1;
};
inline Fq12 fq12_one() { return Fq12{fq6_one(), fq6_zero()}; }
inline bool fq12_eq(const Fq12& a, const Fq12& b) { return fq6_eq(a.c0, b.c0) && fq6_eq(a.c1, b.c1); }
inline bool fq12_is_one(const Fq12& a) { return fq12_eq(a, fq12_one()); }
inline Fq12 fq12_conj(const Fq12& a) { return Fq12{a.c0, fq6_neg(a.c1)}; }  // Frobenius^6
inline Fq12 fq12_mul(const Fq12& a, const Fq12& b) {
    const Fq6 t0 = fq6_mul(a.c0, b.c0), t1 = fq6_mul(a.c1, b.c1);
    const Fq6 m = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1));
    return Fq12{fq6_add(t0, fq6_mul_v(t1)), fq6_sub(fq6_sub(m, t0), t1)};
}
inline Fq12 fq12_sqr(const Fq12& a) {  // (a0 + a1)(a0 + v a1) - t - v t + 2 t w, t = a0 a1
    const Fq6 t = fq6_mul(a.c0, a.c1);
    const Fq6 s = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(a.c0, fq6_mul_v(a.c1)));
    return Fq12{fq6_sub(fq6_sub(s, t), fq6_mul_v(t)), fq6_add(t, t)};
}
inline Fq12 fq12_inv(const Fq12& a) {  // (a0 - a1 w) / (a0^2 - v a1^2); 0 -> 0
    const Fq6 n = fq6_inv(fq6_sub(fq6_sqr(a.c0), fq6_mul_v(fq6_sqr(a.c1))));
    return Fq12{fq6_mul(a.c0, n), fq6_neg(fq6_mul(a.c1, n))};
}
inline Fq12 fq12_frobenius(const Fq12& a) {  // coefficient of w^i -> its conjugate times gamma[i]
    const Consts& k = consts();
    Fq12 r;
    r.c0.c0 = fq2_conj(a.c0.c0);
    r.c1.c0 = fq2_mul(fq2_conj(a.c1.c0), k.gamma[1]);
    r.c0.c1 = fq2_mul(fq2_conj(a.c0.c1), k.gamma[2]);
    r.c1.c1 = fq2_mul(fq2_conj(a.c1.c1), k.gamma[3]);
    r.c0.c2 = fq2_mul(fq2_conj(a.c0.c2), k.gamma[4]);
    r.c1.c2 = fq2_mul(fq2_conj(a.c1.c2), k.gamma[5]);
    return r;
}
// f (l0 + l1 w + l3 w^3), l0 in Fq: the line's three non-zero coefficients
inline Fq12 fq12_mul_line(const Fq12& f, const Fq& l0, const Fq2& l1, const Fq2& l3) {
    const Fq6 a0 = Fq6{fq2_scale(f.c0.c0, l0), fq2_scale(f.c0.c1, l0), fq2_scale(f.c0.c2, l0)};
    const Fq6 a1 = Fq6{fq2_scale(f.c1.c0, l0), fq2_scale(f.c1.c1, l0), fq2_scale(f.c1.c2, l0)};
    return Fq12{fq6_add(a0, fq6_mul_v(fq6_mul_01(f.c1, l1, l3))), fq6_add(a1, fq6_mul_01(f.c0, l1, l3))};
}
inline Fq12 fq12_pow(const Fq12& a, const uint32_t* e, int nlimbs) {
    Fq12 acc = fq12_one();
    bool started = false;
    for (int i = 32 * nlimbs - 1; i >= 0; i--) {
        if (started) acc = fq12_sqr(acc);
        if ((e[i >> 5] >> (i & 31)) & 1u) {
            acc = started ? fq12_mul(acc, a) : a;
            started = true;
        }
    }
    return acc;
}

// ---- G2: the order-r subgroup of the twist y^2 = x^3 + 3/xi ------------------------------------------------------------------------------
inline G2 g2_identity() { return G2{fq2_zero(), fq2_zero(), true}; }
inline const G2& g2_generator() { return consts().gen; }
inline G2 g2_neg(const G2& a) { return G2{a.x, fq2_neg(a.y), a.inf}; }
inline bool g2_eq(const G2& a, const G2& b) { return a.inf || b.inf ? a.inf == b.inf : fq2_eq(a.x, b.x) && fq2_eq(a.y, b.y); }
inline bool g2_on_twist(const G2& a) {
    if (a.inf) return true;
    return fq2_eq(fq2_sqr(a.y), fq2_add(fq2_mul(fq2_sqr(a.x), a.x), consts().b_twist));
}
// the chord-and-tangent step both the group law and the Miller loop take: T <- T + Q (T == Q: the tangent).  Returns false when the
// line is vertical or there is none (an identity on either side, T == -Q, a point of order two): *lambda is then not written.
inline bool g2_step(G2& t, const G2& q, Fq2* lambda) {
    if (q.inf) return false;
    if (t.inf) {
        t = q;
        return false;
    }
    Fq2 lam;
    if (fq2_eq(t.x, q.x)) {
        if (!fq2_eq(t.y, q.y) || fq2_is_zero(t.y)) {
            t = g2_identity();
            return false;
        }
        const Fq2 xx = fq2_sqr(t.x);
        lam = fq2_mul(fq2_add(fq2_dbl(xx), xx), fq2_inv(fq2_dbl(t.y)));
    } else {
        lam = fq2_mul(fq2_sub(q.y, t.y), fq2_inv(fq2_sub(q.x, t.x)));
    }
    const Fq2 x3 = fq2_sub(fq2_sub(fq2_sqr(lam), t.x), q.x);
    const Fq2 y3 = fq2_sub(fq2_mul(lam, fq2_sub(t.x, x3)), t.y);
    t.x = x3;
    t.y = y3;
    *lambda = lam;
    return true;
}
inline G2 g2_add(const G2& a, const G2& b) {
    G2 t = a;
    Fq2 lam;
    (void)g2_step(t, b, &lam);
    return t;
}
inline G2 g2_dbl(const G2& a) { return g2_add(a, a); }
// [k] P, k a plain integer of eight 32-bit limbs (double-and-add, top bit first)
inline G2 g2_mul(const G2& p, const uint32_t* k) {
    G2 acc = g2_identity();
    for (int i = 255; i >= 0; i--) {
        acc = g2_dbl(acc);
        if ((k[i >> 5] >> (i & 31)) & 1u) acc = g2_add(acc, p);
    }
    return acc;
}
// on the twist AND [r] Q = O: the twist's cofactor is 2p - r, so the curve equation alone does not put a point in G2
inline bool g2_in_subgroup(const G2& a) {
    if (!g2_on_twist(a)) return false;
    uint32_t r[8];
    for (int i = 0; i < 8; i++) r[i] = Bn254Fr::mod(i);
    return g2_mul(a, r).inf;
}
// the p-power Frobenius of (x w^2, y w^3), back on the twist
inline G2 g2_frobenius(const G2& a) {
    if (a.inf) return a;
    const Consts& k = consts();
    return G2{fq2_mul(fq2_conj(a.x), k.gamma[2]), fq2_mul(fq2_conj(a.y), k.gamma[3]), false};
}
// the ABI form: 128 bytes {x.c0, x.c1, y.c0, y.c1}, each 4 x u64 little-endian Montgomery (R = 2^256); all-zero = the identity.
// false: a coordinate is not reduced (nothing else is checked here).
inline bool g2_read(const void* p128, G2& out) {
    Fq c[4];
    memcpy((void*)c, p128, 128);
    for (int i = 0; i < 4; i++)
        if (!fq_is_reduced(c[i])) return false;
    out.x = Fq2{c[0], c[1]};
    out.y = Fq2{c[2], c[3]};
    out.inf = fq2_is_zero(out.x) && fq2_is_zero(out.y);
    return true;
}
inline void g2_write(void* p128, const G2& a) {
    Fq c[4] = {a.x.c0, a.x.c1, a.y.c0, a.y.c1};
    if (a.inf) memset((void*)c, 0, sizeof(c));
    memcpy(p128, (const void*)c, 128);
}

// ---- G1: y^2 = x^3 + 3 over Fq, affine -----------------------------------------------------------------------------------------------------
struct G1 {
    Fq x, y;
    bool inf;
};
inline G1 g1_neg(const G1& a) { return G1{a.x, fq_neg(a.y), a.inf}; }
// a 96-byte Jacobian (x, y, z Montgomery; z = 0 is the identity) -> affine.  false: a coordinate is not reduced, or the point is neither
// the identity nor on the curve.
inline bool g1_from_jacobian(const void* p96, G1& out) {
    Fq c[3];
    memcpy((void*)c, p96, 96);
    for (int i = 0; i < 3; i++)
        if (!fq_is_reduced(c[i])) return false;
    out.inf = fe_is_zero<Bn254Fq>(c[2]);
    out.x = out.y = fe_zero<Bn254Fq>();
    if (out.inf) return true;
    const Fq zi = fe_inv<Bn254Fq>(c[2]), zi2 = fq_mul(zi, zi);
    out.x = fq_mul(c[0], zi2);
    out.y = fq_mul(c[1], fq_mul(zi2, zi));
    return fe_eq<Bn254Fq>(fq_mul(out.y, out.y), fq_add(fq_mul(fq_mul(out.x, out.x), out.x), fe_from_u64<Bn254Fq>(3)));
}

// ---- the pairing product ------------------------------------------------------------------------------------------------------------------
// One step of the Miller loop for one pair: T <- T + Q (or 2T when q is T itself) and f <- f * line(P).
inline void miller_step(Fq12& f, G2& t, const G2& q, const G1& p) {
    const G2 t0 = t;
    Fq2 lam;
    if (!g2_step(t, q, &lam)) return;
    f = fq12_mul_line(f, p.y, fq2_neg(fq2_scale(lam, p.x)), fq2_sub(fq2_mul(lam, t0.x), t0.y));
}
// prod_k f_{6x+2, Q_k}(P_k) and the two Frobenius lines of each pair: ONE accumulator, one squaring per step for all pairs.  A pair with
// an identity on either side contributes 1.  Every Q_k must be in G2 (the caller's check): the loop then never meets a vertical line.
inline Fq12 miller_loop(size_t n, const G1* ps, const G2* qs) {
    std::vector<G1> p;
    std::vector<G2> q, t;
    for (size_t k = 0; k < n; k++) {
        if (ps[k].inf || qs[k].inf) continue;
        p.push_back(ps[k]);
        q.push_back(qs[k]);
    }
    t = q;
    Fq12 f = fq12_one();
    for (int i = 63; i >= 0; i--) {  // bit 64 of 6x + 2 is the leading one
        f = fq12_sqr(f);
        for (size_t k = 0; k < q.size(); k++) {
            const G2 same = t[k];
            miller_step(f, t[k], same, p[k]);
        }
        if ((ATE_LOOP_LOW >> i) & 1u)
            for (size_t k = 0; k < q.size(); k++) miller_step(f, t[k], q[k], p[k]);
    }
    for (size_t k = 0; k < q.size(); k++) {
        const G2 q1 = g2_frobenius(q[k]), q2 = g2_neg(g2_frobenius(q1));
        miller_step(f, t[k], q1, p[k]);
        miller_step(f, t[k], q2, p[k]);
    }
    return f;
}
// f^((p^12 - 1) / r) = ((f^(p^6 - 1))^(p^2 + 1))^((p^4 - p^2 + 1) / r)
inline Fq12 final_exponentiation(const Fq12& f) {
    Fq12 g = fq12_mul(fq12_conj(f), fq12_inv(f));
    g = fq12_mul(fq12_frobenius(fq12_frobenius(g)), g);
    return fq12_pow(g, consts().hard, HARD_EXPONENT_LIMBS);
}
// prod_k e(P_k, Q_k) == 1.  n = 0: true.
inline bool pairing_product_is_one(size_t n, const G1* ps, const G2* qs) {
    return fq12_is_one(final_exponentiation(miller_loop(n, ps, qs)));
}

}  // namespace bn254
}  // namespace lurk
