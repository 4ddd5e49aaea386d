// The plan of a batch of short commitments (lurk_beta_amd/csrc/msm_batch_plan.hpp) and the split of the signed window digits, on the CPU:
// a stand-alone program, built with -fsanitize=address,undefined by tests/test_msm_batch_plan_cpu.py.  Prints "ok <checks>" and exits 0,
// or says what failed and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../lurk_beta_amd/csrc/msm_batch_plan.hpp"
#include "../../lurk_beta_amd/csrc/msm_core.cuh"

using namespace lurk;

static long checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        checks++;                                         \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

// a canonical scalar whose window w (c-bit windows) holds `raw`, everything else zero
static void scalar_with_digit(uint32_t (&s)[8], int c, int w, uint32_t raw) {
    memset(s, 0, sizeof(s));
    const int bit = w * c;
    const unsigned __int128 v = (unsigned __int128)raw << (bit & 31);
    for (int k = 0; k < 3; k++)
        if ((bit >> 5) + k < 8) s[(bit >> 5) + k] |= (uint32_t)(v >> (32 * k));
}

static void check_split() {
    for (int c = 16; c <= 20; c++) {
        const int h = msm_batch_split_bits(c);
        const uint32_t B = 1u << h, count = LURK_MSM_BATCH_MAX_VECTORS, NB = 2 * count * B;
        CHECK(h == (c + 1) / 2 && 2 * h >= c, "c=%d h=%d", c, h);
        CHECK(NB <= 131072u, "c=%d NB=%u", c, NB);
        const uint32_t mags[] = {1u, B - 1u, B, B + 1u, 1u << (c - 1)};
        std::set<uint32_t> keys;
        for (uint32_t mag : mags) {
            uint32_t lo, hi;
            msm_batch_split(mag, h, lo, hi);
            CHECK(lo + (hi << h) == mag, "c=%d mag=%u lo=%u hi=%u", c, mag, lo, hi);
            CHECK(lo <= B - 1 && hi <= B / 2, "c=%d mag=%u lo=%u hi=%u", c, mag, lo, hi);
            // the digit as the recoding produces it, for a scalar built to hold it: every window of the width
            for (int w = 0; w + 1 < msm_num_windows(c); w++) {
                uint32_t s[8], carry = 0, r[8];
                scalar_with_digit(s, c, w, mag);
                memcpy(r, s, sizeof(r));
                for (int v = 0; v < msm_num_windows(c); v++) {
                    const uint32_t d = msm_digit_next(r, c, carry), step_carry_free = d & ~MSM_SIGN;
                    CHECK(step_carry_free == (v == w ? mag : 0u) && !(d & MSM_SIGN), "c=%d w=%d v=%d mag=%u digit=%08x", c, w, v, mag, d);
                }
            }
            for (uint32_t k : {0u, 1u, count - 1}) {
                const uint32_t val[2] = {lo, hi};
                for (uint32_t piece = 0; piece < 2; piece++) {
                    if (!val[piece]) continue;
                    const uint32_t key = msm_batch_key(k, piece, B, val[piece]);
                    CHECK(key < NB, "c=%d key=%u NB=%u", c, key, NB);
                    CHECK(key / B == 2 * k + piece && key % B == val[piece] - 1, "c=%d key=%u", c, key);
                }
            }
        }
        // (vector, piece, value) -> key is one to one over a whole batch
        for (uint32_t k = 0; k < count; k++)
            for (uint32_t piece = 0; piece < 2; piece++)
                for (uint32_t value : {1u, 2u, B / 2, B - 1, B}) {
                    const uint32_t key = msm_batch_key(k, piece, B, value);
                    CHECK(key < NB && keys.insert(key).second, "c=%d k=%u piece=%u value=%u key=%u", c, k, piece, value, key);
                }
        // a raw digit above 2^(c-1) recodes to a negative one of magnitude 2^c - raw <= 2^(c-1) - 1: never outside the halves' ranges
        uint32_t s[8], carry = 0, r[8];
        scalar_with_digit(s, c, 0, (1u << (c - 1)) + 1u);
        memcpy(r, s, sizeof(r));
        const uint32_t d = msm_digit_next(r, c, carry);
        CHECK((d & MSM_SIGN) && (d & ~MSM_SIGN) == (1u << (c - 1)) - 1u && carry == 1, "c=%d digit=%08x", c, d);
    }
}

static void check_segments() {
    const std::vector<std::vector<size_t>> cases = {
        {5}, {0, 3}, {3, 0}, {0, 0, 7, 0, 0, 1, 0}, {1, 0, 0, 0, 1}, {300, 0, 299, 1, 0, 64, 65, 0}, std::vector<size_t>(64, 5), {0, 0, 0},
    };
    for (const auto& lens : cases) {
        std::vector<size_t> offs(lens.size());
        for (size_t k = 0; k < lens.size(); k++) offs[k] = 1000 - 7 * k;  // any order, overlapping
        MsmBatchPlan pl;
        const char* why = msm_batch_plan_make(pl, 20, 1 << 20, offs.data(), lens.data(), lens.size());
        CHECK(why == nullptr, "refused: %s", why ? why : "");
        size_t total = 0;
        for (size_t k = 0; k < lens.size(); k++) {
            CHECK(pl.segs.seg_start[k] == total && pl.segs.off[k] == offs[k] && msm_batch_len(pl, (uint32_t)k) == lens[k], "vector %zu", k);
            if (lens[k]) {
                CHECK(msm_batch_segment(pl.segs.seg_start, pl.segs.count, (uint32_t)total) == k, "first element of vector %zu", k);
                CHECK(msm_batch_segment(pl.segs.seg_start, pl.segs.count, (uint32_t)(total + lens[k] - 1)) == k, "last element of vector %zu", k);
            }
            total += lens[k];
        }
        CHECK(pl.total == total && pl.segs.seg_start[lens.size()] == total && pl.segs.count == lens.size(), "total %zu", total);
        CHECK(pl.G == 2 * lens.size() && pl.B == 1024u && pl.NB == pl.G * pl.B && pl.h == 10 && pl.W == 13 && pl.max_entries == 26 * total, "shape");
        CHECK(pl.NBp % MSM_BATCH_GRP == 0 && pl.NBp >= pl.NB && pl.NBp - pl.NB < MSM_BATCH_GRP && pl.NBp <= 131072u && pl.NG == (int)(pl.NBp / MSM_BATCH_GRP),
              "NBp=%u NB=%u", pl.NBp, pl.NB);
        CHECK(pl.S >= 8 && pl.S <= 64 && pl.nt > pl.NBp + pl.max_entries / pl.S && !pl.planned, "S=%d nt=%zu planned=%d", pl.S, pl.nt, (int)pl.planned);
        for (size_t i = 0; i < total; i++) {  // every element: inside its vector
            const uint32_t k = msm_batch_segment(pl.segs.seg_start, pl.segs.count, (uint32_t)i);
            CHECK(k < lens.size() && pl.segs.seg_start[k] <= i && i < pl.segs.seg_start[k + 1], "element %zu -> vector %u", i, k);
        }
    }
}

// the accumulation form: DIRECT up to an average of 32 (possible) entries per bucket, the planned stages above; or as forced
static void check_forms() {
    MsmBatchPlan pl;
    const size_t offs[2] = {0, 0};
    for (int c = 16; c <= 20; c++) {
        const size_t W = (256 + c - 1) / c, B = (size_t)1 << ((c + 1) / 2);
        // 2 W total > 32 * 4 B  <=>  total > 64 B / W
        const size_t edge = 64 * B / W;
        const size_t at[2] = {edge / 2, edge - edge / 2}, over[2] = {edge / 2, edge - edge / 2 + 1};
        CHECK(msm_batch_plan_make(pl, c, 1 << 20, offs, at, 2) == nullptr && !pl.planned, "c=%d: %zu scalars", c, edge);
        CHECK(msm_batch_plan_make(pl, c, 1 << 20, offs, over, 2) == nullptr && pl.planned, "c=%d: %zu scalars", c, edge + 1);
        CHECK(msm_batch_plan_make(pl, c, 1 << 20, offs, at, 2, 1) == nullptr && pl.planned, "c=%d forced planned", c);
        CHECK(msm_batch_plan_make(pl, c, 1 << 20, offs, over, 2, 0) == nullptr && !pl.planned, "c=%d forced direct", c);
    }
    // the sixteen halving vectors of a 2^20 opening: planned, full tasks
    size_t lens[16], off16[16];
    for (int k = 0; k < 16; k++) lens[k] = (size_t)65536 >> k, off16[k] = 0;
    CHECK(msm_batch_plan_make(pl, 20, 1 << 20, off16, lens, 16) == nullptr && pl.planned && pl.S == 64 && pl.NB == 32768u && pl.NBp == 32768u && pl.NG == 1, "halving: S=%d",
          pl.S);
}

static void check_refusals() {
    MsmBatchPlan pl;
    std::vector<size_t> offs(LURK_MSM_BATCH_MAX_VECTORS + 1, 0), lens(LURK_MSM_BATCH_MAX_VECTORS + 1, 4);
    auto refused = [&](int c, size_t npoints, size_t count, const char* word) {
        const char* why = msm_batch_plan_make(pl, c, npoints, offs.data(), lens.data(), count);
        CHECK(why && strstr(why, word), "count=%zu: %s (wanted '%s')", count, why ? why : "accepted", word);
    };
    const size_t big = (size_t)1 << 22;
    refused(20, big, 0, "count == 0");
    refused(20, big, LURK_MSM_BATCH_MAX_VECTORS + 1, "LURK_MSM_BATCH_MAX_VECTORS");
    CHECK(msm_batch_plan_make(pl, 20, big, offs.data(), lens.data(), LURK_MSM_BATCH_MAX_VECTORS) == nullptr, "64 vectors");
    lens[3] = LURK_MSM_BATCH_MAX_LEN;
    CHECK(msm_batch_plan_make(pl, 20, big, offs.data(), lens.data(), 8) == nullptr, "a vector of exactly the longest length");
    lens[3] = LURK_MSM_BATCH_MAX_LEN + 1;
    refused(20, big, 8, "LURK_MSM_BATCH_MAX_LEN");
    lens[3] = 301;
    refused(20, 300, 8, "more scalars than the key has points");
    for (size_t k = 0; k < 16; k++) lens[k] = LURK_MSM_BATCH_MAX_LEN;  // 2^20 exactly
    CHECK(msm_batch_plan_make(pl, 20, big, offs.data(), lens.data(), 16) == nullptr && pl.total == LURK_MSM_BATCH_MAX_TOTAL, "a total of exactly the most");
    lens[16] = 1;
    refused(20, big, 17, "LURK_MSM_BATCH_MAX_TOTAL");
    lens[16] = 0;
    refused(15, big, 16, "window bits");
    refused(21, big, 16, "window bits");
}

int main() {
    check_split();
    check_segments();
    check_forms();
    check_refusals();
    printf("ok %ld\n", checks);
    return 0;
}
