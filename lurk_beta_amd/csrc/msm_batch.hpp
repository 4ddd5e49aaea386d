// msm_batch.hpp - what MsmCtx (msm.hip) sees of the batch pass (msm_batch.hip): a slot's batch workspaces, the enqueue and the host tail.
// The shape of a batch is msm_batch_plan.hpp's.
#pragma once
#include "common.hpp"
#include "msm_batch_plan.hpp"
#include "msm_core.cuh"

namespace lurk {

// a slot's batch buffers: allocated by the slot's first batch, grown on demand, kept for the life of the context
struct MsmBatchWork {
    DevBuf cnt, bucket_start, cursor, sorted, records, big_list, big_count, planes_a, planes_b;
    DevBuf task_start, group_tasks, group_task_base, task_info, task_dest, task_order, len_hist;  // the planned form's (msm_plan.hip)
    void* host_pts = nullptr;  // pinned: G x (h + 1) plane sums (XYZZ) for the host tail
    size_t host_pts_bytes = 0;
    MsmBatchPlan plan;         // of the pending batch
    ~MsmBatchWork() {
        if (host_pts) (void)hipHostFree(host_pts);
    }
    void ensure(const MsmBatchPlan& pl, size_t xyzz_bytes);
};

// every kernel of one batch on stream s: the G x (h + 1) plane sums land in bw.host_pts.  table: the key's window table
// T[w * stride + i] = 2^(c w) P_i.  pl.total > 0.
template <class P, class SF>
void msm_batch_enqueue(MsmBatchWork& bw, const MsmBatchPlan& pl, const void* d_scalars, int is_mont, const Affine<P>* table, size_t stride, hipStream_t s);

// vector k's commitment from the plane sums of its two key spaces (the stream is synchronised): R_lo + 2^h R_hi as one Horner walk
template <class P>
Xyzz<P> msm_batch_host_point(const MsmBatchWork& bw, const MsmBatchPlan& pl, uint32_t k);

}  // namespace lurk
