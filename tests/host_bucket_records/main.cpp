// Task sums and buckets as radix-2^29 records (curve29.cuh: Plane29) against the 8 x 32 round trip they replace, on the host, for the
// four base fields.  A stand-alone program: tests/test_bucket_records_host.py builds it with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DLURK_F29_CHECK=1
// and runs it.  A case is a list of buckets, each a list of tasks, each a list of signed table entries.  Two paths:
//   records   every task's sum is stored with plane_store at the slot the plan would choose (the bucket's own when the bucket is one
//             task, NB + t otherwise), plane_finalize_bucket runs over every bucket (the hot ones are summed the way the workgroup
//             kernel does: 256 strided lane sums, then the tree), and one first-level merge of the bucket reduction reads the bucket
//             records (plane_load, xyzz29_add);
//   8 x 32    xyzz29_to_xyzz per task, xyzz_sum_via29 per bucket, xyzz29_from_xyzz in front of the same merge - the parent's path.
// Both must give the same affine points (and the same identities) for every merged pair.  The record array is a heap block of exactly
// NB + T records, so a store or a load one record past either end is an AddressSanitizer error; plane_store asserts the R-bound
// (tight limbs, value < 2^259) of every record it stores.
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

static int g_cases = 0, g_buckets = 0;
static const uint32_t FIN_SMALL = 16;  // msm_stages.hpp: MSM_FIN_SMALL

struct Entry {
    int rec;      // index into the pool of points; -1: the identity record (0, 0)
    bool negate;
};
typedef std::vector<Entry> Task;
typedef std::vector<Task> Bucket;

template <class P>
struct Curve;  // the generator (canonical limbs of x and y)
template <>
struct Curve<PallasFp> {
    static constexpr const char* name = "Pallas (PallasFp)";
    static Fe<PallasFp> gx() { return fe_neg<PallasFp>(fe_from_u64<PallasFp>(1)); }
    static Fe<PallasFp> gy() { return fe_from_u64<PallasFp>(2); }
};
template <>
struct Curve<PallasFq> {
    static constexpr const char* name = "Vesta (PallasFq)";
    static Fe<PallasFq> gx() { return fe_neg<PallasFq>(fe_from_u64<PallasFq>(1)); }
    static Fe<PallasFq> gy() { return fe_from_u64<PallasFq>(2); }
};
template <>
struct Curve<Bn254Fq> {
    static constexpr const char* name = "BN254 G1 (Bn254Fq)";
    static Fe<Bn254Fq> gx() { return fe_from_u64<Bn254Fq>(1); }
    static Fe<Bn254Fq> gy() { return fe_from_u64<Bn254Fq>(2); }
};
template <>
struct Curve<Bn254Fr> {
    static constexpr const char* name = "Grumpkin (Bn254Fr)";
    static Fe<Bn254Fr> gx() { return fe_from_u64<Bn254Fr>(1); }
    static Fe<Bn254Fr> gy() {
        Fe<Bn254Fr> y;
        const uint32_t l[8] = {0x823f272cu, 0x833fc48du, 0xf1181294u, 0x2d270d45u, 0x06a45d63u, 0xcf135e75u, 0x2u, 0x0u};
        for (int i = 0; i < 8; i++) y.l[i] = l[i];
        return fe_to_mont<Bn254Fr>(y);
    }
};

// k G for k = 1 .. n
template <class P>
static std::vector<Affine<P>> make_pool(int n) {
    Affine<P> g;
    g.x = Curve<P>::gx();
    g.y = Curve<P>::gy();
    std::vector<Affine<P>> pool;
    Xyzz<P> acc = xyzz_identity<P>();
    for (int k = 0; k < n; k++) {
        xyzz_madd<P>(acc, g, false);
        pool.push_back(xyzz_to_affine<P>(acc));
    }
    return pool;
}

template <class P>
static bool same_point(const Xyzz<P>& a, const Xyzz<P>& b) {
    if (xyzz_is_identity<P>(a) || xyzz_is_identity<P>(b)) return xyzz_is_identity<P>(a) == xyzz_is_identity<P>(b);
    const Affine<P> x = xyzz_to_affine<P>(a), y = xyzz_to_affine<P>(b);
    return fe_eq<P>(x.x, y.x) && fe_eq<P>(x.y, y.y);
}

// the hot-bucket kernel's sum on the host: 256 lanes stride the task records, then the tree of block_tree_sum29
template <class P>
static void workgroup_sum(const Plane29<P>* tasks, uint32_t nt, Xyzz29<P>& out, bool& out_id) {
    const int BLOCK = 256;
    Plane29<P>* sh = new Plane29<P>[BLOCK];
    for (int t = 0; t < BLOCK; t++) {
        Xyzz29<P> acc, q;
        acc.x = acc.y = acc.zz = acc.zzz = f29_zero<P>();
        bool acc_id = true, q_id;
        for (uint32_t j = (uint32_t)t; j < nt; j += BLOCK) {
            plane_load<P>(tasks + j, q, q_id);
            xyzz29_add<P>(acc, acc_id, q, q_id);
        }
        plane_store<P>(sh + t, acc, acc_id);
    }
    for (int stride = BLOCK / 2; stride >= 1; stride >>= 1)
        for (int t = 0; t < stride; t++) {
            Xyzz29<P> acc, q;
            bool acc_id, q_id;
            plane_load<P>(sh + t, acc, acc_id);
            plane_load<P>(sh + t + stride, q, q_id);
            xyzz29_add<P>(acc, acc_id, q, q_id);
            plane_store<P>(sh + t, acc, acc_id);
        }
    plane_load<P>(sh, out, out_id);
    delete[] sh;
}

// One case: NB buckets (NB even).  The table holds exactly the pool; entries index it.
template <class P>
static void run_case(const char* what, const std::vector<Affine<P>>& pool, const std::vector<Bucket>& buckets) {
    g_cases++;
    const uint32_t NB = (uint32_t)buckets.size();
    if (NB % 2) { printf("%s: odd bucket count\n", what); exit(2); }
    // the table: the pool, then the identity record; the sorted list: every task's entries back to back
    std::vector<Affine<P>> table(pool);
    Affine<P> zero;
    zero.x = fe_zero<P>();
    zero.y = fe_zero<P>();
    table.push_back(zero);
    std::vector<uint32_t> sorted, task_first, task_last, first_task(NB), ntasks(NB);
    for (uint32_t k = 0; k < NB; k++) {
        first_task[k] = (uint32_t)task_first.size();
        ntasks[k] = (uint32_t)buckets[k].size();
        for (const Task& t : buckets[k]) {
            task_first.push_back((uint32_t)sorted.size());
            for (const Entry& e : t) sorted.push_back((uint32_t)(e.rec < 0 ? (int)pool.size() : e.rec) | (e.negate ? 0x80000000u : 0u));
            task_last.push_back((uint32_t)sorted.size());
        }
    }
    const uint32_t T = (uint32_t)task_first.size();
    sorted.push_back(0);  // (so that data() is a valid pointer for a case without entries; never read)

    // ---- records: the accumulation's stores, finalize, one first-level merge ----
    Plane29<P>* records = new Plane29<P>[(size_t)NB + T];  // exact size
    std::vector<Xyzz<P>> partials(T);
    for (uint32_t k = 0; k < NB; k++)
        for (uint32_t j = 0; j < ntasks[k]; j++) {
            const uint32_t t = first_task[k] + j;
            Xyzz29<P> acc;
            bool acc_id;
            msm_task_accumulate29_raw<P, false>(sorted.data(), task_first[t], task_last[t], table.data(), acc, acc_id);
            const uint32_t dest = ntasks[k] == 1 ? k : NB + t;  // (msm_tasks_kernel: task_dest)
            plane_store<P>(records + dest, acc, acc_id);
            partials[t] = xyzz29_to_xyzz<P>(acc, acc_id);       // the parent's epilogue
        }
    for (uint32_t k = 0; k < NB; k++) {
        g_buckets++;
        if (plane_finalize_bucket<P>(records, NB, k, ntasks[k], first_task[k], FIN_SMALL)) {
            if (ntasks[k] <= FIN_SMALL) { printf("%s, %s: bucket %u listed with %u tasks\n", Curve<P>::name, what, k, ntasks[k]); exit(1); }
            Xyzz29<P> acc;
            bool acc_id;
            workgroup_sum<P>(records + NB + first_task[k], ntasks[k], acc, acc_id);
            plane_store<P>(records + k, acc, acc_id);
        }
    }
    // ---- 8 x 32: the parent's finalize and its level-0 conversion ----
    std::vector<Xyzz<P>> old_buckets(NB);
    for (uint32_t k = 0; k < NB; k++) old_buckets[k] = xyzz_sum_via29<P>(partials.data() + first_task[k], ntasks[k]);
    // and the sums themselves, by the 8 x 32 group law over the entries
    for (uint32_t k = 0; k < NB; k++) {
        Xyzz<P> ref = xyzz_identity<P>();
        for (const Task& t : buckets[k])
            for (const Entry& e : t)
                if (e.rec >= 0) xyzz_madd<P>(ref, pool[e.rec], e.negate);
        Xyzz29<P> b;
        bool b_id;
        plane_load<P>(records + k, b, b_id);
        if (!same_point<P>(ref, xyzz29_to_xyzz<P>(b, b_id)) || !same_point<P>(ref, old_buckets[k])) {
            printf("%s, %s: bucket %u differs from the 8 x 32 group law (record identity %d)\n", Curve<P>::name, what, k, (int)b_id);
            exit(1);
        }
    }
    for (uint32_t seg = 0; seg < NB / 2; seg++) {
        Xyzz29<P> r, h, ro, ho;
        bool r_id, h_id, ro_id, ho_id;
        plane_load<P>(records + 2 * seg, r, r_id);
        plane_load<P>(records + 2 * seg + 1, h, h_id);
        xyzz29_add<P>(r, r_id, h, h_id);
        xyzz29_from_xyzz<P>(old_buckets[2 * seg], ro, ro_id);
        xyzz29_from_xyzz<P>(old_buckets[2 * seg + 1], ho, ho_id);
        xyzz29_add<P>(ro, ro_id, ho, ho_id);
        if (r_id != ro_id || !same_point<P>(xyzz29_to_xyzz<P>(r, r_id), xyzz29_to_xyzz<P>(ro, ro_id))) {
            printf("%s, %s: merged pair %u differs between the two paths (identity flags %d / %d)\n", Curve<P>::name, what, seg, (int)r_id, (int)ro_id);
            exit(1);
        }
        // (the level's second component, the new plane 0, is the upper bucket itself: compared above)
    }
    delete[] records;
}

static Task task_of(int first_rec, int len, int negate_every = 3) {
    Task t;
    for (int i = 0; i < len; i++) t.push_back({first_rec + i, negate_every > 0 && i % negate_every == 1});
    return t;
}

template <class P>
static void run_field() {
    const std::vector<Affine<P>> pool = make_pool<P>(600);
    // 0 / 1 / 2 / many tasks per bucket, beside each other so that every kind meets every other in a merge
    {
        std::vector<Bucket> b;
        b.push_back({});                                               // empty
        b.push_back({task_of(0, 1)});                                  // one task of one entry: the copy of a first base
        b.push_back({task_of(1, 5)});                                  // one task
        b.push_back({task_of(6, 8), task_of(14, 3)});                  // two tasks
        b.push_back({});
        b.push_back({});                                               // two empty buckets merge to the identity
        Bucket sixteen, seventeen, many;
        for (int j = 0; j < 16; j++) sixteen.push_back(task_of(20 + 2 * j, 2));
        for (int j = 0; j < 17; j++) seventeen.push_back(task_of(60 + 2 * j, 2));
        for (int j = 0; j < 300; j++) many.push_back(task_of(100 + j, 1 + j % 2));   // more tasks than the workgroup has lanes
        b.push_back(sixteen);                                          // the last lane-summed bucket
        b.push_back(seventeen);                                        // the first listed one
        b.push_back(many);
        b.push_back({task_of(500, 4)});
        run_case<P>("0 / 1 / 2 / 16 / 17 / 300 tasks", pool, b);
    }
    // identity task sums: a one-task bucket whose sum is the identity (P - P), a two-task bucket with one identity task, two tasks
    // that cancel each other, identity records only
    {
        std::vector<Bucket> b;
        b.push_back({{{7, false}, {7, true}}});                                        // stored in place as an identity record
        b.push_back({task_of(10, 3)});
        b.push_back({{{8, false}, {8, true}}, task_of(20, 2)});                        // identity + a sum
        b.push_back({task_of(30, 2), {{9, true}, {9, false}}});                        // a sum + identity
        b.push_back({{{40, false}, {41, false}}, {{40, true}, {41, true}}});           // two tasks that cancel: the bucket is the identity
        b.push_back({{{-1, false}, {-1, true}}});                                      // identity records only
        b.push_back({{{50, false}}, {{50, false}}});                                   // two equal task sums: the general doubling
        b.push_back({{{51, false}, {51, false}}});                                     // P + P inside a one-task bucket: the affine doubling
        Bucket hot;                                                                    // a listed bucket whose task sums are all equal or opposite
        for (int j = 0; j < 40; j++) hot.push_back({{60, j % 4 == 3}});
        b.push_back(hot);
        b.push_back({});
        run_case<P>("identity task sums and doublings", pool, b);
    }
    // equal buckets side by side (the merge's doubling) and opposite ones (the merge's identity)
    {
        std::vector<Bucket> b;
        b.push_back({task_of(70, 3, 0)});
        b.push_back({task_of(70, 3, 0)});
        b.push_back({{{80, false}, {81, false}}});
        b.push_back({{{80, true}}, {{81, true}}});
        run_case<P>("equal and opposite neighbours", pool, b);
    }
}

int main() {
    run_field<PallasFp>();
    run_field<PallasFq>();
    run_field<Bn254Fq>();
    run_field<Bn254Fr>();
    printf("bucket records host: %d cases, %d buckets, records == 8 x 32 round trip\n", g_cases, g_buckets);
    return 0;
}
