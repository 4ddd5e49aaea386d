// msm_batch_plan.hpp - the shape of a batch of short commitments under one window-table key (lurk_hip_msm_ctx_submit_batch_dev,
// msm_batch.hip), in the manner of msm_launch_plan.hpp: plain C++ (no HIP), so that tests/host_msm_batch checks it on the CPU.
//
// A key of more than 2^18 points takes 20-bit windows: one key space of 2^19 buckets, which a commitment of 64 scalars sorts, plans
// and reduces like one of 2^20.  The batch splits every signed window digit d of vector k at h = ceil(c / 2) bits instead,
//   |d| = lo + 2^h hi,   both halves with d's sign,
// into two key spaces of B = 2^h buckets per vector: space 2k holds the lo halves, space 2k + 1 the hi halves, and
//   result_k = R_lo + 2^h R_hi,   R = sum_b b * bucket_b of a space.
// With c = 20 that is 2 x 1024 buckets per vector; 64 vectors make NB = 131 072 keys, what the DIRECT accumulation
// (msm_launch_plan.hpp: MSM_DIRECT_MAX_BUCKETS) was sized for.  |d| <= 2^(c-1), so hi <= 2^(c-1-h) <= B / 2: the hi space stays
// (at least) half empty; a half that is zero makes no entry.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lurk_hip.h"

#if defined(__HIPCC__)
#define LURK_BATCH_HD __host__ __device__ inline
#else
#define LURK_BATCH_HD inline
#endif

namespace lurk {

// what the kernels take by value: where each vector starts in the batch's own numbering of its scalars, and in the caller's buffer
struct MsmBatchSegs {
    uint32_t count;
    uint32_t seg_start[LURK_MSM_BATCH_MAX_VECTORS + 1];  // prefix sums of the lengths; [count] = total
    uint64_t off[LURK_MSM_BATCH_MAX_VECTORS];            // first element (32 B) of vector k in the caller's buffer
};

struct MsmBatchPlan {
    int c = 0, h = 0, W = 0;    // the key's window bits, the split, windows per scalar
    uint32_t B = 0, G = 0, NB = 0;  // buckets per key space, key spaces (two per vector), keys
    size_t total = 0;           // scalars of all vectors
    size_t max_entries = 0;     // 2 W total: every half of every digit non-zero
    // the accumulation: DIRECT (msm_bucket_direct.hip: a few lanes per bucket, no task list) for batches whose buckets stay short, the
    // planned stages (msm_plan.hip, msm_acc.hip, msm_finalize.hip: buckets cut into tasks of <= S entries) for the others
    bool planned = false;
    uint32_t NBp = 0;           // NB rounded up to whole scan groups of the plan stage (the keys behind NB stay empty)
    int NG = 0, S = 0;          // scan groups, entries per task
    size_t nt = 0;              // most tasks: one per non-empty bucket and one per S entries
    MsmBatchSegs segs{};
};

constexpr uint32_t MSM_BATCH_GRP = 1u << 15;         // = MSM_GRP (msm_core.cuh): keys per scan group of the plan stage
constexpr size_t MSM_BATCH_TASK_TARGET = 131072;     // = MSM_TASK_TARGET (msm_sort.hpp): tasks that fill the chip's lanes
constexpr size_t MSM_BATCH_DIRECT_PER_BUCKET = 32;   // DIRECT up to this many entries per bucket on average

LURK_BATCH_HD int msm_batch_split_bits(int c) { return (c + 1) / 2; }

// |d| = lo + 2^h hi
LURK_BATCH_HD void msm_batch_split(uint32_t mag, int h, uint32_t& lo, uint32_t& hi) {
    lo = mag & ((1u << h) - 1u);
    hi = mag >> h;
}

// key of a non-zero half: vector k, piece 0 (lo) or 1 (hi), value 1 .. B
LURK_BATCH_HD uint32_t msm_batch_key(uint32_t k, uint32_t piece, uint32_t B, uint32_t value) { return (2u * k + piece) * B + value - 1u; }

// the vector that owns scalar i of the batch (i < seg_start[count]): the largest k with seg_start[k] <= i - which skips the empty vectors
// that start at the same position
LURK_BATCH_HD uint32_t msm_batch_segment(const uint32_t* seg_start, uint32_t count, uint32_t i) {
    uint32_t lo = 0, hi = count;  // invariant: seg_start[lo] <= i < seg_start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_start[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The plan of a batch under a key of `npoints` points with c-bit windows, or the reason it is refused (NULL: accepted).  Nothing is
// allocated or launched before this has accepted the batch.
// form: < 0 by size, 0 DIRECT, 1 the planned stages (LURK_MSM_BATCH_PLANNED: A/B runs and the tests of both forms at small sizes)
inline const char* msm_batch_plan_make(MsmBatchPlan& pl, int c, size_t npoints, const size_t* offsets, const size_t* lens, size_t count, int form = -1) {
    if (count == 0) return "batch: no vectors (count == 0)";
    if (count > LURK_MSM_BATCH_MAX_VECTORS) return "batch: more than LURK_MSM_BATCH_MAX_VECTORS vectors";
    if (c < 16 || c > 20) return "batch: the key's window bits are not in 16..20";
    size_t total = 0;
    for (size_t k = 0; k < count; k++) {
        if (lens[k] > LURK_MSM_BATCH_MAX_LEN) return "batch: a vector is longer than LURK_MSM_BATCH_MAX_LEN";
        if (lens[k] > npoints) return "batch: a vector has more scalars than the key has points";
        total += lens[k];
    }
    if (total > LURK_MSM_BATCH_MAX_TOTAL) return "batch: more than LURK_MSM_BATCH_MAX_TOTAL scalars in all";
    pl.c = c;
    pl.h = msm_batch_split_bits(c);
    pl.W = (256 + c - 1) / c;
    pl.B = 1u << pl.h;
    pl.G = 2u * (uint32_t)count;
    pl.NB = pl.G * pl.B;
    pl.total = total;
    pl.max_entries = (size_t)2 * pl.W * total;
    pl.planned = form < 0 ? pl.max_entries > MSM_BATCH_DIRECT_PER_BUCKET * pl.NB : form != 0;
    pl.NBp = (pl.NB + MSM_BATCH_GRP - 1) / MSM_BATCH_GRP * MSM_BATCH_GRP;
    pl.NG = (int)(pl.NBp / MSM_BATCH_GRP);
    // The planned form is taken where buckets are long (a 2^16-scalar vector puts ~830 entries into each lo bucket and ~1 660 into each hi
    // bucket at c = 20): full 64-entry tasks keep most buckets at <= 16 task sums, which one lane adds up; 16-entry tasks - what filling
    // every lane would ask for - make every bucket of the long vectors a workgroup's job in the finalize stage (measured: 1.51 ms there).
    // Forced at a small size (tests), the rule of msm_make_shape: halve the task length until the tasks fill the lanes
    pl.S = 64;
    if (form >= 0)
        while (pl.S > 8 && pl.max_entries / pl.S < MSM_BATCH_TASK_TARGET) pl.S /= 2;
    pl.nt = (size_t)pl.NBp + pl.max_entries / pl.S + 1;
    pl.segs.count = (uint32_t)count;
    uint32_t at = 0;
    for (size_t k = 0; k < count; k++) {
        pl.segs.seg_start[k] = at;
        pl.segs.off[k] = (uint64_t)offsets[k];
        at += (uint32_t)lens[k];
    }
    pl.segs.seg_start[count] = at;
    return nullptr;
}

inline size_t msm_batch_len(const MsmBatchPlan& pl, uint32_t k) { return pl.segs.seg_start[k + 1] - pl.segs.seg_start[k]; }

}  // namespace lurk
