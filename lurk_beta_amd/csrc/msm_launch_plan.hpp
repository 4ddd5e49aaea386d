// msm_launch_plan.hpp - which form of the bucket accumulation a commitment takes: the scheduling policy of the MSM, stated once.
// Plain C++ (no HIP): MsmCtx::submit_impl / run (msm.hip) ask it once per commitment, tests/host_harness checks its table on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/lurk_hip.h"

namespace lurk {

// How a commitment was handed in: SYNC for run / run_oneshot / reserve, the others are the LURK_MSM_SUBMIT_* values of a submit.
enum class MsmSubmitClass {
    SYNC = -1,
    DEFAULT = LURK_MSM_SUBMIT_DEFAULT,
    FOREGROUND = LURK_MSM_SUBMIT_FOREGROUND,
    BACKGROUND = LURK_MSM_SUBMIT_BACKGROUND,
    FOLLOW = LURK_MSM_SUBMIT_FOLLOW,
};

enum class MsmAccForm {
    DIRECT,                  // plan, accumulate and finalize as one launch, a few lanes per bucket (msm_bucket_direct.hip)
    PLAIN,                   // one launch over every task, on the slot stream (msm_acc.hip)
    PERSISTENT_ACC_STREAM,   // one wave per SIMD on the slot's low-priority accumulate stream (msm_acc_persistent.hip)
    PERSISTENT_SLOT_STREAM,  // wgs_per_cu waves per SIMD on the slot stream, behind the followed commitment's accumulation
};

// Switches of the commitments-in-flight path (read once per process; the defaults are the measured best).
// Everything else that round 2 kept for A/B runs (stream / wave priorities off, more waves per SIMD, a 128-VGPR build,
// background-behind-sort off) lost its measurement and is gone: the winning setting is now the only code path.
struct MsmTuning {
    int persistent = 1, max_acc = 2, placement_log = 0, bucket_direct = 1;
    size_t persistent_min = (size_t)24 << 20;
    int persist_s = 128;  // entries per task of a PERSISTENT_ACC_STREAM commitment whose shape has full tasks (128 = MSM_S_MAX, or 64 = MSM_S)
    static MsmTuning from_env() {
        auto geti = [](const char* k, int d) { const char* v = getenv(k); return v ? atoi(v) : d; };
        MsmTuning t;
        t.persistent = geti("LURK_MSM_ACC_PERSISTENT", 1);  // DEFAULT-class commitments in flight: 0 = plain launch, 1 = persistent from persistent_min entries, 2 = always
        // W n entries (in 2^20) from which a commitment in flight takes the persistent form.  A one-wave-per-SIMD accumulation runs at
        // ~55 % of the plain launch's rate; two of them resident pay that back only when the accumulation is long against the sort and
        // tail around it: 2^21 scalars x 13 windows (27 M entries) break even, 2^20 (13.6 M) is 4 % faster with the plain launch
        // (853-858 against 821-825 Mscalar-mul/s, two in flight; profiles/r05_persistent_threshold.txt).
        t.persistent_min = (size_t)geti("LURK_MSM_PERSISTENT_MIN_MENTRIES", 24) << 20;
        t.max_acc = geti("LURK_MSM_MAX_ACC", 2);              // persistent accumulations resident at once (0 = no limit)
        t.bucket_direct = geti("LURK_MSM_BUCKET_DIRECT", 1);  // 0: short commitments keep the planned-task stages (A/B runs, parity test)
        t.placement_log = geti("LURK_MSM_PLACEMENT_LOG", 0);  // diagnostic: persistent workgroups per CU, on stderr
        // 128-entry tasks make a Poisson(96) bucket - 2^22 uniform scalars over 2^19 buckets - ONE task: its sum is stored in place and
        // finalize has no addition for it, where 64-entry tasks cost a general addition per bucket.  The price is a longer tail per lane,
        // which only the form with another resident accumulation behind it hides: the plain launch and the FOLLOW class keep MSM_S.
        // 64 against 128 alternating on one box: 1 100-1 107 against 1 113 Mscalar-mul/s (LURK_MSM_PERSIST_S=64 for A/B runs)
        t.persist_s = geti("LURK_MSM_PERSIST_S", 128) == 64 ? 64 : 128;
        if (t.max_acc > 2) t.max_acc = 0;
        return t;
    }
};
inline const MsmTuning& msm_tuning() {
    static const MsmTuning t = MsmTuning::from_env();
    return t;
}
// waves per SIMD of a LURK_MSM_SUBMIT_FOLLOW commitment's persistent accumulation; 0: the plain launch (A/B runs)
inline int msm_follow_wgs() {
    static const int wgs = [] { const char* v = getenv("LURK_MSM_FOLLOW_WGS"); const int x = v ? atoi(v) : 2; return x < 0 ? 0 : x > 3 ? 3 : x; }();
    return wgs;
}

// few buckets, few entries (a key of <= 2^16 points under 16-bit windows) take the DIRECT form
constexpr uint32_t MSM_DIRECT_MAX_BUCKETS = 131072;         // two key spaces of 16-bit windows
constexpr size_t MSM_DIRECT_MAX_ENTRIES = (size_t)1 << 21;  // W n: 2^16 points x 16 windows, or a pair over 2^17 composed scalars

struct MsmLaunchPlan {
    MsmAccForm form;
    bool low_prio;         // the sort, the plan and the accumulation at the lowest wave priority (the tail keeps the raised one)
    unsigned wgs_per_cu;   // PERSISTENT_SLOT_STREAM: waves per SIMD; 0 otherwise (PERSISTENT_ACC_STREAM: LURK_MSM_PERSIST_WGS decides)
    bool uses_acc_stream;  // the slot's low-priority accumulate stream exists for this commitment
};

// entries = W n sorted entries, NB = keys of the commitment's shape, follow_wgs = msm_follow_wgs()
inline MsmLaunchPlan msm_launch_plan(MsmSubmitClass cls, size_t entries, uint32_t NB, const MsmTuning& tn, int follow_wgs) {
    const bool bg = cls == MsmSubmitClass::BACKGROUND, follow = cls == MsmSubmitClass::FOLLOW;
    // FOREGROUND and FOLLOW keep everything on the (high-priority) slot stream; a synchronous call runs on the caller's stream
    const bool acc_stream = cls == MsmSubmitClass::DEFAULT || bg;
    MsmLaunchPlan pl{MsmAccForm::PLAIN, follow, 0u, acc_stream};
    // (LURK_MSM_ACC_PERSISTENT=2 - "always the persistent form" - and background submissions keep the planned stages)
    if (tn.bucket_direct && !bg && !(acc_stream && tn.persistent == 2) && NB <= MSM_DIRECT_MAX_BUCKETS && entries <= MSM_DIRECT_MAX_ENTRIES) {
        pl.form = MsmAccForm::DIRECT;
    } else if (follow && follow_wgs > 0) {
        pl.form = MsmAccForm::PERSISTENT_SLOT_STREAM;
        pl.wgs_per_cu = (unsigned)follow_wgs;
    } else if (acc_stream && (bg || (tn.persistent == 1 ? entries >= tn.persistent_min : tn.persistent != 0))) {
        // large commitments in flight take the persistent form on the slot's low-priority accumulate stream; below persistent_min
        // entries the plain launch (see MsmTuning)
        pl.form = MsmAccForm::PERSISTENT_ACC_STREAM;
    }
    return pl;
}

}  // namespace lurk
