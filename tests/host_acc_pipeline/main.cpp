// The pipelined task loop of the persistent bucket accumulation (curve29.cuh: msm_task_accumulate29_raw<P, true>) against the plain
// loop (<P, false>) on the host, for the four base fields.  A stand-alone program: tests/test_acc_pipeline_host.py builds it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLURK_F29_CHECK=1
// and runs it.  The two loops must leave EXACTLY the same Xyzz29 accumulator (every limb) and identity flag: the pipelined loop only
// moves loads.  The index list of a case is a heap block of exactly `last` words and the table a heap block of exactly the records the
// task references, so a look-ahead that reads past either end is an AddressSanitizer error; the words in front of `first` name a
// record far outside the table, so a loop that read them would fault as well.  The bound assertions of the radix-2^29 layer are on.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../lurk_beta_amd/csrc/curve29.cuh"

using namespace lurk;

#if !F29_CHECKS_ACTIVE
#error "build with -DLURK_F29_CHECK=1"
#endif

static int g_cases = 0;

struct Entry {
    int rec;      // index into the pool of points; -1: the identity record (0, 0)
    bool negate;
};

template <class P>
struct Curve;  // the generator (canonical limbs of x and y) and b of y^2 = x^3 + b
template <>
struct Curve<PallasFp> {  // Pallas: (-1, 2), b = 5
    static constexpr const char* name = "Pallas (PallasFp)";
    static Fe<PallasFp> gx() { return fe_neg<PallasFp>(fe_from_u64<PallasFp>(1)); }
    static Fe<PallasFp> gy() { return fe_from_u64<PallasFp>(2); }
    static Fe<PallasFp> b() { return fe_from_u64<PallasFp>(5); }
};
template <>
struct Curve<PallasFq> {  // Vesta: (-1, 2), b = 5
    static constexpr const char* name = "Vesta (PallasFq)";
    static Fe<PallasFq> gx() { return fe_neg<PallasFq>(fe_from_u64<PallasFq>(1)); }
    static Fe<PallasFq> gy() { return fe_from_u64<PallasFq>(2); }
    static Fe<PallasFq> b() { return fe_from_u64<PallasFq>(5); }
};
template <>
struct Curve<Bn254Fq> {  // BN254 G1: (1, 2), b = 3
    static constexpr const char* name = "BN254 G1 (Bn254Fq)";
    static Fe<Bn254Fq> gx() { return fe_from_u64<Bn254Fq>(1); }
    static Fe<Bn254Fq> gy() { return fe_from_u64<Bn254Fq>(2); }
    static Fe<Bn254Fq> b() { return fe_from_u64<Bn254Fq>(3); }
};
template <>
struct Curve<Bn254Fr> {  // Grumpkin: (1, sqrt(-16)), b = -17
    static constexpr const char* name = "Grumpkin (Bn254Fr)";
    static Fe<Bn254Fr> gx() { return fe_from_u64<Bn254Fr>(1); }
    static Fe<Bn254Fr> gy() {
        Fe<Bn254Fr> y;
        const uint32_t l[8] = {0x823f272cu, 0x833fc48du, 0xf1181294u, 0x2d270d45u, 0x06a45d63u, 0xcf135e75u, 0x2u, 0x0u};
        for (int i = 0; i < 8; i++) y.l[i] = l[i];
        return fe_to_mont<Bn254Fr>(y);
    }
    static Fe<Bn254Fr> b() { return fe_neg<Bn254Fr>(fe_from_u64<Bn254Fr>(17)); }
};

template <class P>
static bool on_curve(const Affine<P>& a) {
    const Fe<P> lhs = fe_sqr<P>(a.y);
    const Fe<P> rhs = fe_add<P>(fe_mul<P>(fe_sqr<P>(a.x), a.x), Curve<P>::b());
    return fe_eq<P>(lhs, rhs);
}

// k G for k = 1 .. n: distinct points, none the negation of another (n is far below the group order)
template <class P>
static std::vector<Affine<P>> make_pool(int n) {
    Affine<P> g;
    g.x = Curve<P>::gx();
    g.y = Curve<P>::gy();
    if (!on_curve<P>(g)) { printf("%s: the generator is not on the curve\n", Curve<P>::name); exit(2); }
    std::vector<Affine<P>> pool;
    Xyzz<P> acc = xyzz_identity<P>();
    for (int k = 0; k < n; k++) {
        xyzz_madd<P>(acc, g, false);
        const Affine<P> a = xyzz_to_affine<P>(acc);
        if (!on_curve<P>(a)) { printf("%s: %d G is not on the curve\n", Curve<P>::name, k + 1); exit(2); }
        pool.push_back(a);
    }
    return pool;
}

template <class P>
static bool same29(const Xyzz29<P>& a, const Xyzz29<P>& b) {
    return memcmp(a.x.l, b.x.l, sizeof a.x.l) == 0 && memcmp(a.y.l, b.y.l, sizeof a.y.l) == 0 && memcmp(a.zz.l, b.zz.l, sizeof a.zz.l) == 0 &&
           memcmp(a.zzz.l, b.zzz.l, sizeof a.zzz.l) == 0;
}

// One task: `prefix` unread words, then the entries.  The table holds exactly the distinct records of the task, in order of first use.
template <class P>
static void run_case(const char* what, const std::vector<Affine<P>>& pool, const std::vector<Entry>& task, uint32_t prefix) {
    g_cases++;
    std::vector<int> slot_of(pool.size() + 1, -1);  // pool index (+1; 0: the identity record) -> table slot
    std::vector<Affine<P>> recs;
    std::vector<uint32_t> words;
    for (const Entry& e : task) {
        int& s = slot_of[e.rec + 1];
        if (s < 0) {
            s = (int)recs.size();
            Affine<P> a;
            if (e.rec < 0) { a.x = fe_zero<P>(); a.y = fe_zero<P>(); }
            else a = pool[e.rec];
            recs.push_back(a);
        }
        words.push_back((uint32_t)s | (e.negate ? 0x80000000u : 0u));
    }
    const uint32_t first = prefix, last = prefix + (uint32_t)task.size();
    // exact-size heap blocks (operator new[]: the sanitizer's red zones start at the first byte after them)
    uint32_t* sorted = new uint32_t[last];
    for (uint32_t i = 0; i < prefix; i++) sorted[i] = 0x7fffffffu;
    for (size_t i = 0; i < words.size(); i++) sorted[prefix + i] = words[i];
    Affine<P>* table = new Affine<P>[recs.size()];
    for (size_t i = 0; i < recs.size(); i++) table[i] = recs[i];

    Xyzz29<P> plain, piped;
    bool plain_id = false, piped_id = false;
    msm_task_accumulate29_raw<P, false>(sorted, first, last, table, plain, plain_id);
    msm_task_accumulate29_raw<P, true>(sorted, first, last, table, piped, piped_id);
    if (plain_id != piped_id || !same29<P>(plain, piped)) {
        printf("%s, %s: the pipelined loop differs from the plain loop (identity flags %d / %d)\n", Curve<P>::name, what, (int)plain_id, (int)piped_id);
        exit(1);
    }
    // and both are the sum: the 8 x 32-bit group law over the same entries, compared as affine points
    Xyzz<P> ref = xyzz_identity<P>();
    for (const Entry& e : task)
        if (e.rec >= 0) xyzz_madd<P>(ref, pool[e.rec], e.negate);
    const Xyzz<P> got = xyzz29_to_xyzz<P>(piped, piped_id);
    if (xyzz_is_identity<P>(ref) != xyzz_is_identity<P>(got)) { printf("%s, %s: identity mismatch against the 8 x 32 group law\n", Curve<P>::name, what); exit(1); }
    if (!xyzz_is_identity<P>(ref)) {
        const Affine<P> ra = xyzz_to_affine<P>(ref), ga = xyzz_to_affine<P>(got);
        if (!fe_eq<P>(ra.x, ga.x) || !fe_eq<P>(ra.y, ga.y)) { printf("%s, %s: the sum differs from the 8 x 32 group law\n", Curve<P>::name, what); exit(1); }
    }
    delete[] table;
    delete[] sorted;
}

template <class P>
static void run_field() {
    const std::vector<Affine<P>> pool = make_pool<P>(70);
    char what[96];
    // distinct records, mixed signs: every length at which the loop takes another path (nothing, the copy, the affine + affine form,
    // the first trip of the steady loop, the clamped look-ahead at each distance from the end) and a full 64-entry task
    const int lengths[] = {0, 1, 2, 3, 4, 5, 64};
    for (int len : lengths)
        for (uint32_t prefix : {0u, 3u}) {
            std::vector<Entry> t;
            for (int i = 0; i < len; i++) t.push_back({i, (i * 5 + len) % 3 == 0});
            snprintf(what, sizeof what, "length %d behind %u words", len, prefix);
            run_case<P>(what, pool, t, prefix);
        }
    // one negated entry at every position of a length-5 task, and all five negated
    for (int pos = 0; pos <= 5; pos++) {
        std::vector<Entry> t;
        for (int i = 0; i < 5; i++) t.push_back({10 + i, pos == 5 || i == pos});
        snprintf(what, sizeof what, "negated entry at %d of 5", pos);
        run_case<P>(what, pool, t, 0);
    }
    // the identity record first, second, in the middle and last (and a task of nothing else)
    for (int pos : {0, 1, 2, 4}) {
        std::vector<Entry> t;
        for (int i = 0; i < 5; i++) t.push_back({i == pos ? -1 : 20 + i, i == 3});
        snprintf(what, sizeof what, "identity record at %d of 5", pos);
        run_case<P>(what, pool, t, 0);
    }
    run_case<P>("identity records only", pool, {{-1, false}, {-1, true}, {-1, false}}, 0);
    // the same record twice in a row (the out-of-line doubling while a prefetch is in flight), and a record followed by its negation
    // (the accumulator returns to the identity and carries on), at positions (0, 1), (1, 2) and (3, 4); both signs of the pair
    for (int pos : {0, 1, 3})
        for (bool cancel : {false, true})
            for (bool neg : {false, true}) {
                std::vector<Entry> t;
                for (int i = 0; i < 5; i++) t.push_back({30 + i, false});
                t[pos + 1].rec = t[pos].rec;
                t[pos].negate = neg;
                t[pos + 1].negate = cancel ? !neg : neg;
                snprintf(what, sizeof what, "%s at (%d, %d), first %s", cancel ? "record and its negation" : "record twice", pos, pos + 1, neg ? "negated" : "plain");
                run_case<P>(what, pool, t, 0);
            }
    // both at once, and ending on them: P P -P -P (back to the identity at the end of the task) and P -P alone
    run_case<P>("P P -P -P", pool, {{40, false}, {40, false}, {40, true}, {40, true}}, 0);
    run_case<P>("P -P", pool, {{41, false}, {41, true}}, 0);
    run_case<P>("P P", pool, {{42, true}, {42, true}}, 2);
}

int main() {
    run_field<PallasFp>();
    run_field<PallasFq>();
    run_field<Bn254Fq>();
    run_field<Bn254Fr>();
    printf("acc pipeline host: %d cases, pipelined == plain\n", g_cases);
    return 0;
}
