// msm_batch.hip - a batch of short commitments under prefixes of one window-table key in one pass: lurk_hip_msm_ctx_submit_batch_dev /
// lurk_hip_msm_ctx_wait_batch.  The caller is the first stage of a HyperKZG opening (hyperkzg.hip), whose folded polynomials
// P_1 .. P_{ell-1} are independent of every challenge (arecibo's hyperkzg EvaluationEngine under the compressing prover of the default
// cycle, /root/reference/src/proof/nova.rs:65-71).
//
// A commitment of 64 scalars under a 2^20-point key sorts, plans and reduces for the key's 2^19 buckets like one of 2^20 scalars; K such
// commitments are K latency chains.  Here every signed window digit is split in two halves (msm_batch_plan.hpp), vector k gets two key
// spaces of 2^ceil(c/2) buckets, and ONE pass serves all of them:
//   1. count     msm_batch_emit_kernel<SF, false>: one lane per scalar - Montgomery -> canonical, the signed digits, both halves - counts the keys
//                (in LDS per workgroup, one global atomic per non-empty bin)
//   2. scan      msm_batch_scan_kernel: one workgroup, bucket_start = exclusive prefix sums of cnt (NB <= 131 072 keys)
//   3. scatter   msm_batch_emit_kernel<SF, true>: the same walk again, every non-zero half placed through its key's cursor
//   4. accumulate the DIRECT form (msm_bucket_direct.hip: a few lanes per bucket, a workgroup for a bucket that holds a whole window) while
//                the buckets stay short; the planned stages (msm_plan.hip, msm_acc.hip, msm_finalize.hip: tasks of <= S entries, balanced
//                over the lanes) when a long vector puts hundreds of entries into each of its buckets (msm_batch_plan.hpp)
//   5. reduce    msm_launch_reduce at c' = h + 1 over G = 2 x count key spaces of B = 2^h buckets (msm_reduce.hip), plane sums to pinned memory
//   6. host      per vector one Horner walk over both spaces' plane sums, R_lo + 2^h R_hi, and the normalisation lurk_hip_msm_ctx_wait does
// The order of a bucket's entries depends on the order the lanes arrive in; the bucket's sum and the normalised result do not.
// No workgroup waits for another inside a launch; the kernels run at the sort kernels' raised wave priority.
#include "msm_batch.hpp"

#include "msm_ctx.hpp"
#include "msm_launch_plan.hpp"
#include "msm_sort.hpp"
#include "msm_stages.hpp"

namespace lurk {

constexpr int BATCH_BLOCK = 1024;
constexpr uint32_t BATCH_BINS_MAX = 2048;  // 2 B at the widest window: c = 20, h = 10
constexpr int BATCH_SCAN_BLOCK = 1024;
static_assert(MSM_BATCH_GRP == (uint32_t)MSM_GRP && MSM_BATCH_TASK_TARGET == MSM_TASK_TARGET, "msm_batch_plan.hpp restates the plan stage's constants");
constexpr uint32_t BATCH_LEN_HIST_WORDS = 2 * (MSM_S_MAX + 1);  // the plan stage's length histogram and class cursors
static_assert(BATCH_LEN_HIST_WORDS <= BATCH_SCAN_BLOCK, "one lane per word");

// every non-zero half of every signed window digit of one canonical scalar (scalar j of vector k): f(bin, entry), bin = the half's key inside
// the vector's two spaces (piece * B + value - 1 < 2 B), entry = (table index | sign) as msm_task_accumulate29_raw reads it
template <class F>
__device__ __forceinline__ void msm_batch_walk(const uint32_t (&s)[8], int c, int h, int W, uint32_t B, uint32_t j, uint32_t stride, F&& f) {
    uint32_t r[8];
#pragma unroll
    for (int t = 0; t < 8; t++) r[t] = s[t];
    uint32_t carry = 0;
    for (int w = 0; w < W; w++) {
        const uint32_t d = msm_digit_next(r, c, carry);
        const uint32_t mag = d & ~MSM_SIGN;
        if (!mag) continue;
        uint32_t lo, hi;
        msm_batch_split(mag, h, lo, hi);
        const uint32_t entry = ((uint32_t)w * stride + j) | (d & MSM_SIGN);
        if (lo) f(lo - 1u, entry);
        if (hi) f(B + hi - 1u, entry);
    }
}

// One lane per scalar of the batch, BATCH_BLOCK consecutive scalars per workgroup.  SCATTER = false: cnt[key] += 1 per non-zero half;
// true: sorted[cursor[key]++] = entry.  Nearly all scalars of a workgroup belong to ONE vector (that of its first scalar): their halves are
// counted in LDS (2 B bins) and reach the global counters as one atomic per non-empty bin - with one global atomic per half, the 2^16 x 13
// halves of a long vector queue on its 1 536 adjacent words (measured: 0.99 ms for the sixteen halving vectors of a 2^20 opening).  The
// scatter counts the same way, takes a run of every non-empty bin from the global cursor, and walks the digits a second time to place each
// entry at its rank inside the run.  A scalar of another vector (a workgroup that spans a boundary) goes to the global counters directly.
template <class SF, bool SCATTER>
__global__ __launch_bounds__(BATCH_BLOCK) void msm_batch_emit_kernel(const uint4* __restrict__ scalars, MsmBatchSegs segs, uint32_t total, int c, int h, int W,
                                                                      uint32_t B, uint32_t stride, int is_mont, uint32_t* __restrict__ counters,
                                                                      uint32_t* __restrict__ sorted, uint32_t cap) {
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint32_t hist[BATCH_BINS_MAX], run[BATCH_BINS_MAX];
    const uint32_t first = blockIdx.x * BATCH_BLOCK, i = first + threadIdx.x, bins = 2 * B;  // (first < total: the grid is div_up(total, BATCH_BLOCK))
    const uint32_t k0 = msm_batch_segment(segs.seg_start, segs.count, first);
    uint32_t* own = counters + (size_t)2 * k0 * B;  // the counters of vector k0's two spaces
    for (uint32_t b = threadIdx.x; b < bins; b += BATCH_BLOCK) hist[b] = 0;
    __syncthreads();
    const bool live = i < total;
    uint32_t k = k0, j = 0, s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        k = msm_batch_segment(segs.seg_start, segs.count, i);
        j = i - segs.seg_start[k];  // the scalar's index in its vector = its base
        const size_t at = (size_t)segs.off[k] + j;
        const uint4 lo4 = scalars[2 * at], hi4 = scalars[2 * at + 1];
        Fe<SF> s;
        s.l[0] = lo4.x; s.l[1] = lo4.y; s.l[2] = lo4.z; s.l[3] = lo4.w;
        s.l[4] = hi4.x; s.l[5] = hi4.y; s.l[6] = hi4.z; s.l[7] = hi4.w;
        if (is_mont) s = fe_from_mont<SF>(s);
#pragma unroll
        for (int t = 0; t < 8; t++) s8[t] = s.l[t];
    }
    const bool local = k == k0;
    uint32_t* mine = counters + (size_t)2 * k * B;
    if (live) {
        msm_batch_walk(s8, c, h, W, B, j, stride, [&](uint32_t bin, uint32_t) {
            if (local) atomicAdd(&hist[bin], 1u);
            else if (!SCATTER) atomicAdd(&mine[bin], 1u);
        });
    }
    __syncthreads();
    if (!SCATTER) {
        for (uint32_t b = threadIdx.x; b < bins; b += BATCH_BLOCK)
            if (hist[b]) atomicAdd(&own[b], hist[b]);
        return;
    }
    for (uint32_t b = threadIdx.x; b < bins; b += BATCH_BLOCK) {
        const uint32_t n = hist[b];
        run[b] = n ? atomicAdd(&own[b], n) : 0u;
        hist[b] = 0;
    }
    __syncthreads();
    if (live) {
        msm_batch_walk(s8, c, h, W, B, j, stride, [&](uint32_t bin, uint32_t entry) {
            const uint32_t pos = local ? run[bin] + atomicAdd(&hist[bin], 1u) : atomicAdd(&mine[bin], 1u);
            if (pos < cap) sorted[pos] = entry;  // (always, unless the caller rewrote the scalars between the two launches)
        });
    }
}

// one workgroup: bucket_start[key] = sum of cnt[0 .. key), a copy as the scatter's cursors; clears the small counters of the stages behind
// it (the big-bucket counter, the plan's length histogram and class cursors), as the sort's single-block launch does for a commitment
__global__ __launch_bounds__(BATCH_SCAN_BLOCK) void msm_batch_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ bucket_start,
                                                                           uint32_t* __restrict__ cursor, uint32_t NB, uint32_t* __restrict__ big_count,
                                                                           uint32_t* __restrict__ len_hist) {
    __builtin_amdgcn_s_setprio(3);
    __shared__ uint32_t part[BATCH_SCAN_BLOCK];
    const uint32_t t = threadIdx.x, per = (NB + BATCH_SCAN_BLOCK - 1) / BATCH_SCAN_BLOCK;
    const uint32_t lo = t * per < NB ? t * per : NB, hi = lo + per < NB ? lo + per : NB;
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; b++) sum += cnt[b];
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < BATCH_SCAN_BLOCK; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t b = lo; b < hi; b++) {
        bucket_start[b] = run;
        cursor[b] = run;
        run += cnt[b];
    }
    if (t == 0) *big_count = 0;
    if (t < BATCH_LEN_HIST_WORDS) len_hist[t] = 0;
}

void MsmBatchWork::ensure(const MsmBatchPlan& pl, size_t xyzz_bytes) {
    const size_t nb = pl.NBp;
    len_hist.ensure(BATCH_LEN_HIST_WORDS * 4);
    if (pl.planned) {
        task_start.ensure((size_t)pl.NG * (MSM_GRP + 1) * 4);
        group_tasks.ensure(64 * 4);
        group_task_base.ensure(64 * 4);
        task_info.ensure(pl.nt * sizeof(uint2));
        task_dest.ensure(pl.nt * 4);
        task_order.ensure(pl.nt * 4);
    }
    cnt.ensure(nb * 4);
    bucket_start.ensure(nb * 4);
    cursor.ensure(nb * 4);
    sorted.ensure(pl.max_entries * 4);
    records.ensure((nb + (pl.planned ? pl.nt : 0)) * MSM_RECORD_BYTES);  // the buckets, behind them the planned form's task sums
    big_list.ensure(nb * 4);
    big_count.ensure(16);
    planes_a.ensure(msm_reduce_plane_bytes(nb));
    planes_b.ensure(msm_reduce_plane_bytes(nb));
    const size_t need = (size_t)pl.G * (pl.h + 1) * xyzz_bytes;
    if (need > host_pts_bytes) {
        if (host_pts) (void)hipHostFree(host_pts);
        host_pts = nullptr;
        host_pts_bytes = 0;
        LURK_HIP_CHECK(hipHostMalloc(&host_pts, need));
        host_pts_bytes = need;
    }
}

template <class P, class SF>
void msm_batch_enqueue(MsmBatchWork& bw, const MsmBatchPlan& pl, const void* d_scalars, int is_mont, const Affine<P>* table, size_t stride, hipStream_t s) {
    LURK_REQUIRE(pl.total > 0 && pl.total <= LURK_MSM_BATCH_MAX_TOTAL && pl.NB <= MSM_DIRECT_MAX_BUCKETS && pl.NBp >= pl.NB && pl.NBp <= MSM_DIRECT_MAX_BUCKETS,
                 "batch: plan out of range");
    LURK_REQUIRE((size_t)pl.W * stride < ((size_t)1 << 31), "batch: table index out of range");
    LURK_REQUIRE(2 * pl.B <= BATCH_BINS_MAX, "batch: more bins per vector than the emit kernel's LDS holds");
    bw.ensure(pl, sizeof(Xyzz<P>));
    uint32_t *cnt = bw.cnt.as<uint32_t>(), *bucket_start = bw.bucket_start.as<uint32_t>(), *cursor = bw.cursor.as<uint32_t>(), *sorted = bw.sorted.as<uint32_t>();
    const dim3 grid(div_up(pl.total, BATCH_BLOCK)), block(BATCH_BLOCK);
    {
        ProfScope ps("msm_batch_sort", s);
        LURK_HIP_CHECK(hipMemsetAsync(cnt, 0, (size_t)pl.NBp * 4, s));
        hipLaunchKernelGGL((msm_batch_emit_kernel<SF, false>), grid, block, 0, s, (const uint4*)d_scalars, pl.segs, (uint32_t)pl.total, pl.c, pl.h, pl.W, pl.B,
                           (uint32_t)stride, is_mont, cnt, sorted, (uint32_t)pl.max_entries);
        hipLaunchKernelGGL(msm_batch_scan_kernel, dim3(1), dim3(BATCH_SCAN_BLOCK), 0, s, (const uint32_t*)cnt, bucket_start, cursor, pl.NBp,
                           bw.big_count.as<uint32_t>(), bw.len_hist.as<uint32_t>());
        hipLaunchKernelGGL((msm_batch_emit_kernel<SF, true>), grid, block, 0, s, (const uint4*)d_scalars, pl.segs, (uint32_t)pl.total, pl.c, pl.h, pl.W, pl.B,
                           (uint32_t)stride, is_mont, cursor, sorted, (uint32_t)pl.max_entries);
        LURK_HIP_CHECK(hipGetLastError());
    }
    Plane29<P>* records = (Plane29<P>*)bw.records.p;
    uint32_t *big_list = bw.big_list.as<uint32_t>(), *big_count = bw.big_count.as<uint32_t>();
    if (!pl.planned) {
        ProfScope ps("msm_batch_accumulate_direct", s);
        msm_launch_bucket_direct<P>(sorted, table, bucket_start, cnt, pl.NB, pl.max_entries, records, big_list, big_count, s);
    } else {
        // the stages of a commitment's PLAIN form (MsmCtx::enqueue, msm.hip) over the NBp keys; the bucket reduction reads the first NB
        uint32_t *task_start = bw.task_start.as<uint32_t>(), *group_task_base = bw.group_task_base.as<uint32_t>(), *task_dest = bw.task_dest.as<uint32_t>(),
                 *order = bw.task_order.as<uint32_t>();
        uint2* task_info = bw.task_info.as<uint2>();
        {
            ProfScope ps("msm_batch_tasks", s);
            msm_launch_plan_tasks(cnt, bucket_start, task_start, bw.group_tasks.as<uint32_t>(), group_task_base, pl.NG, pl.NBp, task_info, task_dest,
                                  bw.len_hist.as<uint32_t>(), order, pl.nt, (uint32_t)pl.S, 0, s);
        }
        {
            ProfScope ps("msm_batch_accumulate", s);
            msm_launch_accumulate<P>(sorted, table, task_info, order, task_dest, group_task_base, pl.NG, records, pl.nt, s);
        }
        {
            ProfScope ps("msm_batch_finalize", s);
            msm_launch_finalize<P>(records, cnt, task_start, group_task_base, pl.NBp, big_list, big_count, (uint32_t)pl.S, s);
            msm_launch_big_buckets<P>(records, cnt, task_start, group_task_base, pl.NBp, big_list, big_count, (uint32_t)pl.S, s);
        }
    }
    {
        ProfScope ps("msm_batch_reduce", s);
        msm_launch_reduce<P>(records, bw.planes_a.p, bw.planes_b.p, pl.h + 1, (int)pl.G, pl.B, (Xyzz<P>*)bw.host_pts, s);
    }
    LURK_HIP_CHECK(hipGetLastError());
}

// space g's plane sums are v[g (h + 1) ..]: [S, P_0 .. P_{h-1}], R_g = S + sum_k 2^k P_k.  R_lo + 2^h R_hi has plane P_lo,j at bit j < h,
// P_hi,j-h (and S_hi at j = h) at bit j >= h: 2 h doublings in all
template <class P>
Xyzz<P> msm_batch_host_point(const MsmBatchWork& bw, const MsmBatchPlan& pl, uint32_t k) {
    const int h = pl.h;
    const Xyzz<P>* v = (const Xyzz<P>*)bw.host_pts;
    const Xyzz<P>*lo = v + (size_t)(2 * k) * (h + 1), *hi = lo + (h + 1);
    Xyzz<P> acc = xyzz_identity<P>();
    for (int j = 2 * h - 1; j >= 0; j--) {
        acc = xyzz_dbl<P>(acc);
        if (j >= h) xyzz_add<P>(acc, hi[1 + (j - h)]);
        else xyzz_add<P>(acc, lo[1 + j]);
        if (j == h) xyzz_add<P>(acc, hi[0]);
    }
    xyzz_add<P>(acc, lo[0]);
    return acc;
}

#define LURK_BATCH_INSTANTIATE(P, SF)                                                                                                        \
    template void msm_batch_enqueue<P, SF>(MsmBatchWork&, const MsmBatchPlan&, const void*, int, const Affine<P>*, size_t, hipStream_t); \
    template Xyzz<P> msm_batch_host_point<P>(const MsmBatchWork&, const MsmBatchPlan&, uint32_t);
LURK_BATCH_INSTANTIATE(PallasFp, PallasFq)
LURK_BATCH_INSTANTIATE(PallasFq, PallasFp)
LURK_BATCH_INSTANTIATE(Bn254Fq, Bn254Fr)
LURK_BATCH_INSTANTIATE(Bn254Fr, Bn254Fq)

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_msm_ctx_submit_batch_dev(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars32, const size_t* offsets, const size_t* lens, size_t count, int is_mont,
                                      void* stream) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "batch: null ctx");
        LURK_REQUIRE(offsets, "batch: null offsets");
        LURK_REQUIRE(lens, "batch: null lens");
        LURK_REQUIRE(count != 0, "batch: no vectors (count == 0)");
        LURK_REQUIRE(count <= LURK_MSM_BATCH_MAX_VECTORS, "batch: more than LURK_MSM_BATCH_MAX_VECTORS vectors");
        bool any = false;
        for (size_t k = 0; k < count; k++) any = any || lens[k] != 0;
        LURK_REQUIRE(!any || d_scalars32, "batch: null scalars");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->submit_batch(slot, d_scalars32, offsets, lens, count, is_mont, (hipStream_t)stream);
    });
}
int lurk_hip_msm_ctx_wait_batch(lurk_hip_msm_ctx* ctx, int slot, void* out_jacobian96) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "batch: null ctx");
        LURK_REQUIRE(out_jacobian96, "batch: null output");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->wait_batch(slot, out_jacobian96);
    });
}

}  // extern "C"
