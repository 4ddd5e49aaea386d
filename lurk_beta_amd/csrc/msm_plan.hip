// msm_plan.hip - stage 3 of the MSM pipeline (msm_core.cuh): the sorted entries of every bucket are cut into tasks of <= S entries and the
// tasks ordered longest first for the accumulation; each task is also told where its sum goes in the slot's record array (task_dest).
// The kernels are short and bound by latency or LDS atomics; none of them touches a field element.
#include "common.hpp"
#include "msm_core.cuh"
#include "msm_sort.hpp"
#include "msm_stages.hpp"

namespace lurk {

// The raised wave priority of every short kernel of a commitment (why: msm_sort.hip, msm_sort_wave_prio).
// `low`: the commitment was submitted with LURK_MSM_SUBMIT_FOLLOW - work staged ahead that must only take what the open step's serial
// chain (cross term, commit(T), folds: wave priority 3) leaves; its sort and plan kernels then run at the lowest wave priority like its
// accumulation (the tail kernels - finalize, bucket reduction - always run at 3: see MsmCtx::submit_impl, msm.hip).
__device__ __forceinline__ void msm_set_wave_prio(int low) {
    if (low) __builtin_amdgcn_s_setprio(0);
    else __builtin_amdgcn_s_setprio(3);
}

// ---- 3. task planning ------------------------------------------------------------------------
// block g (group of MSM_GRP keys), 1024 threads x 32 keys: task starts inside the group + group total
__global__ __launch_bounds__(1024) void msm_taskscan_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ task_start,
                                                              uint32_t* __restrict__ group_tasks, uint32_t S, int low) {
    msm_set_wave_prio(low);
    __shared__ uint32_t sh[1024];
    const int g = blockIdx.x, t = threadIdx.x;
    constexpr int PER = MSM_GRP / 1024;
    const uint4* src = reinterpret_cast<const uint4*>(cnt + (size_t)g * MSM_GRP + (size_t)t * PER);
    uint32_t c[PER];
    uint32_t tot = 0;
#pragma unroll
    for (int j = 0; j < PER / 4; j++) {
        uint4 v = src[j];
        c[4 * j] = (v.x + S - 1) / S;
        c[4 * j + 1] = (v.y + S - 1) / S;
        c[4 * j + 2] = (v.z + S - 1) / S;
        c[4 * j + 3] = (v.w + S - 1) / S;
        tot += c[4 * j] + c[4 * j + 1] + c[4 * j + 2] + c[4 * j + 3];
    }
    sh[t] = tot;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        uint32_t a = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    uint32_t run = sh[t] - tot;
    uint32_t* dst = task_start + (size_t)g * (MSM_GRP + 1) + (size_t)t * PER;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        dst[j] = run;
        run += c[j];
    }
    if (t == 1023) {
        task_start[(size_t)g * (MSM_GRP + 1) + MSM_GRP] = run;
        group_tasks[g] = run;
    }
}
// task table: task t -> [first, last) of the sorted list (<= S entries of one bucket).  Every workgroup first scans the per-group task
// totals itself (NG <= 32 values: group_task_base[0..NG], which workgroup 0 also stores for the kernels that follow) - a launch of its
// own for that scan was one more link in a chain of dependent launches that costs 5-60 us per link beside resident accumulations.
constexpr int MSM_NG_MAX = 64;
__global__ __launch_bounds__(256) void msm_tasks_kernel(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ bucket_start,
                                                          const uint32_t* __restrict__ task_start, const uint32_t* __restrict__ group_tasks,
                                                          uint32_t* __restrict__ group_task_base_out, int NG, uint32_t NB, uint2* __restrict__ task_info,
                                                          uint32_t* __restrict__ task_dest, uint32_t S, int low) {
    msm_set_wave_prio(low);
    __shared__ uint32_t group_task_base[MSM_NG_MAX + 1];
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int g = 0; g < NG; g++) {
            group_task_base[g] = run;
            run += group_tasks[g];
        }
        group_task_base[NG] = run;
        if (blockIdx.x == 0)
            for (int g = 0; g <= NG; g++) group_task_base_out[g] = group_task_base[g];
    }
    __syncthreads();
    uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= group_task_base[NG]) return;
    int g = 0;
    while (g + 1 < NG && group_task_base[g + 1] <= t) g++;
    uint32_t tl = t - group_task_base[g];
    const uint32_t* ts = task_start + (size_t)g * (MSM_GRP + 1);
    uint32_t b = msm_upper_slot(ts, MSM_GRP, tl);
    uint32_t part = tl - ts[b];
    size_t key = (size_t)g * MSM_GRP + b;
    uint32_t first = bucket_start[key] + part * S;
    uint32_t end = bucket_start[key] + cnt[key];
    task_info[t] = make_uint2(first, first + S < end ? first + S : end);
    // where the accumulation stores this task's sum in the slot's record array (msm_stages.hpp): a bucket that is ONE task is its
    // task's sum - straight into the bucket's slot, and the finalize stage has nothing to do for it; otherwise the task's own slot
    // behind the NB buckets
    task_dest[t] = cnt[key] <= S ? (uint32_t)key : NB + t;
}

// Longest-task-first order: tasks are counting-sorted by length (1..S <= MSM_S_MAX) in descending order, so
// the 64 lanes of a wave run tasks of equal length (no lane waits for the longest task of its wave;
// bucket sizes are ragged - Poisson around their mean - and skewed for witness-like scalars) and the
// short tasks fill the tail of the launch.  Full tasks (length S, the bulk at large n) are
// counted per wave with one ballot instead of one LDS atomic each.
__global__ __launch_bounds__(1024) void msm_len_hist_kernel(const uint2* __restrict__ task_info, const uint32_t* __restrict__ group_task_base,
                                                              int NG, uint32_t* __restrict__ len_hist, uint32_t S, int low) {
    msm_set_wave_prio(low);
    __shared__ uint32_t sh[MSM_S_MAX + 1];
    if (threadIdx.x <= MSM_S_MAX) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t ntasks = group_task_base[NG];
    for (uint32_t base = blockIdx.x * 8192u; base < ntasks; base += gridDim.x * 8192u) {
        for (uint32_t k = 0; k < 8; k++) {
            uint32_t t = base + k * 1024u + threadIdx.x;
            uint32_t len = 0;
            if (t < ntasks) {
                uint2 ti = task_info[t];
                len = ti.y - ti.x;
            }
            unsigned long long full = __ballot(len == S);
            if (full && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)full) - 1)) atomicAdd(&sh[S], (uint32_t)__popcll(full));
            if (len != 0 && len != S) atomicAdd(&sh[len], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x <= MSM_S_MAX && sh[threadIdx.x]) atomicAdd(&len_hist[threadIdx.x], sh[threadIdx.x]);
}
// (the start offset of each length class, longest first, is scanned from len_hist by every workgroup of the scatter below: the class
// cursors count from zero - they are cleared with the other small counters by the sort's single-block launch)
__global__ __launch_bounds__(1024) void msm_len_scatter_kernel(const uint2* __restrict__ task_info,
                                                                 const uint32_t* __restrict__ group_task_base, int NG,
                                                                 const uint32_t* __restrict__ len_hist, uint32_t* __restrict__ len_cursor,
                                                                 uint32_t* __restrict__ order, uint32_t S, int low) {
    msm_set_wave_prio(low);
    __shared__ uint32_t sh_cnt[MSM_S_MAX + 1], sh_base[MSM_S_MAX + 1], sh_class[MSM_S_MAX + 1];
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int l = (int)S; l >= 0; l--) {
            sh_class[l] = run;
            run += len_hist[l];
        }
    }
    __syncthreads();
    const uint32_t ntasks = group_task_base[NG];
    for (uint32_t base = blockIdx.x * 1024u; base < ntasks; base += gridDim.x * 1024u) {
        if (threadIdx.x <= MSM_S_MAX) sh_cnt[threadIdx.x] = 0;
        __syncthreads();
        uint32_t t = base + threadIdx.x;
        uint32_t len = 0, rank = 0;
        if (t < ntasks) {
            uint2 ti = task_info[t];
            len = ti.y - ti.x;
        }
        unsigned long long full = __ballot(len == S);
        if (len == S) {
            int lane = threadIdx.x & 63, leader = __ffsll((long long)full) - 1;
            uint32_t wbase = 0;
            if (lane == leader) wbase = atomicAdd(&sh_cnt[S], (uint32_t)__popcll(full));
            wbase = __shfl(wbase, leader);
            rank = wbase + (uint32_t)__popcll(full & ((1ull << lane) - 1ull));
        } else if (len != 0) {
            rank = atomicAdd(&sh_cnt[len], 1u);
        }
        __syncthreads();
        if (threadIdx.x <= MSM_S_MAX && sh_cnt[threadIdx.x]) sh_base[threadIdx.x] = sh_class[threadIdx.x] + atomicAdd(&len_cursor[threadIdx.x], sh_cnt[threadIdx.x]);
        __syncthreads();
        if (len != 0) order[sh_base[len] + rank] = t;
        __syncthreads();
    }
}

// the four launches of the plan; len_hist holds the length histogram and, MSM_S_MAX + 1 words on, the class cursors
void msm_launch_plan_tasks(const uint32_t* cnt, const uint32_t* bucket_start, uint32_t* task_start, uint32_t* group_tasks, uint32_t* group_task_base,
                           int NG, uint32_t NB, uint2* task_info, uint32_t* task_dest, uint32_t* len_hist, uint32_t* order, size_t nt, uint32_t S, int low,
                           hipStream_t s) {
    hipLaunchKernelGGL(msm_taskscan_kernel, dim3(NG), dim3(1024), 0, s, cnt, task_start, group_tasks, S, low);
    hipLaunchKernelGGL(msm_tasks_kernel, dim3(div_up(nt, 256)), dim3(256), 0, s, cnt, bucket_start, task_start, group_tasks, group_task_base, NG, NB, task_info,
                       task_dest, S, low);
    hipLaunchKernelGGL(msm_len_hist_kernel, dim3(256), dim3(1024), 0, s, task_info, group_task_base, NG, len_hist, S, low);
    hipLaunchKernelGGL(msm_len_scatter_kernel, dim3(512), dim3(1024), 0, s, task_info, group_task_base, NG, len_hist, len_hist + MSM_S_MAX + 1, order, S, low);
}

}  // namespace lurk
