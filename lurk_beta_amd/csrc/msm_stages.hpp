// msm_stages.hpp - the host interfaces of the MSM pipeline's stages (msm_core.cuh), declared once for the unit that defines each and for
// MsmCtx::enqueue (msm.hip), which calls them; the sort's is msm_sort.hpp.  The contracts are stated at the definitions.
#pragma once
#include "common.hpp"
#include "msm_core.cuh"

namespace lurk {

constexpr int MSM_SLOTS = LURK_MSM_SLOTS;  // commitments in flight per context (independent workspaces + streams)
constexpr int MSM_ACC_BLOCK = 256;         // threads per workgroup of both accumulate kernels
constexpr int MSM_FIN_SMALL = 16;          // buckets with <= this many task sums are summed by one lane, fuller ones by a workgroup
constexpr size_t MSM_SMALL_MAX_POINTS = (size_t)1 << 16;  // the small-commitment form: a resident key of at most this many points

// What the stages from the accumulation on hand each other: Plane29<P> (curve29.cuh), a point on the radix-2^29 layer with the identity
// as a flag.  ONE array of them per slot: the NB buckets at [0, NB), the sum of task t of a bucket of two or more tasks at NB + t.  A
// bucket that is one task has that task's sum stored straight into its own slot (task_dest, written by the plan).
template <class P>
struct Plane29;
constexpr size_t MSM_RECORD_BYTES = 160;  // sizeof(Plane29<P>), asserted where the record is defined in full

// ---- 3. task planning (msm_plan.hip): task_start / group_tasks / group_task_base / task_info / task_dest, then the longest-first order ----
void msm_launch_plan_tasks(const uint32_t* cnt, const uint32_t* bucket_start, uint32_t* task_start, uint32_t* group_tasks, uint32_t* group_task_base,
                           int NG, uint32_t NB, uint2* task_info, uint32_t* task_dest, uint32_t* len_hist, uint32_t* order, size_t nt, uint32_t S, int low,
                           hipStream_t s);

// ---- 4. accumulate (msm_acc.hip, msm_acc_persistent.hip): those units are compiled with the multiplier inlined ----
// (task t's sum is stored as a record at records[task_dest[t]])
template <class P>
void msm_launch_accumulate(const uint32_t* sorted, const Affine<P>* table, const uint2* task_info, const uint32_t* order, const uint32_t* task_dest,
                           const uint32_t* group_task_base, int NG, Plane29<P>* records, size_t nt, hipStream_t s);
template <class P>
void msm_launch_accumulate_persistent(const uint32_t* sorted, const Affine<P>* table, const uint2* task_info, const uint32_t* order, const uint32_t* task_dest,
                                      const uint32_t* group_task_base, int NG, Plane29<P>* records, uint32_t* cursor, hipStream_t s, unsigned wgs_per_cu = 0);

// ---- 3-5 in one launch for commitments with few buckets (msm_bucket_direct.hip) ----
int msm_bucket_direct_lanes(size_t NB, size_t entries);
template <class P>
void msm_launch_bucket_direct(const uint32_t* sorted, const Affine<P>* table, const uint32_t* bucket_start, const uint32_t* cnt, uint32_t NB, size_t entries,
                              Plane29<P>* records, uint32_t* big_list, uint32_t* big_count, hipStream_t s);

// ---- 5. finalize (msm_finalize.hip), on the record array: an empty bucket gets its identity record, a bucket of 2 .. MSM_FIN_SMALL tasks is
// summed by one lane, a fuller one goes on the list and is summed by a workgroup (the second launch); a bucket of one task is left alone ----
template <class P>
void msm_launch_finalize(Plane29<P>* records, const uint32_t* cnt, const uint32_t* task_start, const uint32_t* group_task_base, uint32_t NB,
                         uint32_t* big_list, uint32_t* big_count, uint32_t S, hipStream_t s);
template <class P>
void msm_launch_big_buckets(Plane29<P>* records, const uint32_t* cnt, const uint32_t* task_start, const uint32_t* group_task_base, uint32_t NB,
                            const uint32_t* big_list, const uint32_t* big_count, uint32_t S, hipStream_t s);

// ---- 6. the bucket reduction (msm_reduce.hip): one launch per level of the bit-plane merge tree, radix-2^29 points ----
size_t msm_reduce_plane_bytes(size_t nb);
template <class P>
void msm_launch_reduce(const Plane29<P>* buckets, void* planes_a, void* planes_b, int c, int G, uint32_t B, Xyzz<P>* out_host, hipStream_t s);

// ---- the precomputed table T[w*n + i] = 2^(c w) * P_i (msm_precompute.hip) ----
size_t msm_precompute_scratch_bytes(size_t n, int W);
template <class P>
void msm_launch_precompute(const Affine<P>* bases, size_t n, Affine<P>* table, int c, int W, void* scratch, hipStream_t s);

// ---- the small-commitment path (msm_small.hip): a resident key of <= MSM_SMALL_MAX_POINTS points keeps every multiple of every window base ----
int msm_small_window_bits(size_t n);
size_t msm_small_table_entries(size_t n, int c);
unsigned msm_small_groups(size_t n, int c);
unsigned msm_small_out_points(unsigned groups);
size_t msm_small_group_bytes();
size_t msm_small_scratch_bytes();
template <class P>
void msm_small_build_table(const Affine<P>* wbases, size_t n, int c, Affine<P>* table, hipStream_t s);
template <class P, class SF>
void msm_small_launch(const void* d_scalars, size_t n, int is_mont, const Affine<P>* table, int c, void* group_pts, uint32_t* counter, Xyzz<P>* out,
                      hipStream_t s);

}  // namespace lurk
