// msm_multi.hip - one process, several devices: a commitment key cut into slices, each a context (msm.hip) of its own.
#include "common.hpp"
#include "msm_ctx.hpp"
#include "msm_stages.hpp"

using namespace lurk;

// A commitment key cut into contiguous slices, one per device of the list, driven from ONE host process:
// each slice has its own context (resident in that device's HBM) and its own host thread bound to the device, so
// the devices sort / accumulate concurrently; the 96-byte partial commitments come back to the host and are
// summed with the host group law.  No bucket array ever crosses a link.
struct lurk_hip_msm_multi {
    struct Shard {
        size_t lo = 0, hi = 0;
        std::unique_ptr<DeviceWorker> worker;
        std::unique_ptr<MsmCtxBase> ctx;  // created, used and destroyed on the worker thread
        DevBuf staged;                    // device copy of this shard's scalars (host-pointer commits)
        Jacobian<PallasFp> partial;       // every curve shares the 96-byte layout
        // how many of the first n scalars are this shard's (0: it takes no part in a commitment of n scalars)
        size_t count(size_t n) const { return lo < n ? (hi < n ? hi : n) - lo : 0; }
    };
    int curve = 0;
    size_t npoints = 0;
    std::vector<std::unique_ptr<Shard>> shards;
    std::mutex mu;  // one commitment at a time per multi-context
    size_t pending_n[MSM_SLOTS] = {};  // asynchronous form: scalars of the commitment in flight on each slot
    bool pending[MSM_SLOTS] = {};

    // f(shard, index, count) on the worker of every shard that owns some of the first n scalars; waits for all of them
    template <class F>
    void for_shards(size_t n, F&& f) {
        std::vector<Shard*> live;
        for (size_t i = 0; i < shards.size(); i++) {
            Shard* shp = shards[i].get();
            const size_t cnt = shp->count(n);
            if (!cnt) continue;
            shp->worker->post([shp, i, cnt, &f] { f(*shp, i, cnt); });
            live.push_back(shp);
        }
        std::unique_ptr<HipFailure> first;
        for (Shard* shp : live) {
            try {
                shp->worker->wait();
            } catch (const HipFailure& e) {
                if (!first) first.reset(new HipFailure(e));
            }
        }
        if (first) throw *first;
    }
    void require_shard_pointers(const void* const* d_scalars, size_t n) const {
        for (size_t i = 0; i < shards.size(); i++) LURK_REQUIRE(!shards[i]->count(n) || d_scalars[i], "null shard pointer");
    }
    static void sum_parts(int curve, const std::vector<Jacobian<PallasFp>>& parts, void* out) {
        nested_ok(lurk_hip_point_sum(curve, out, parts.data(), parts.size()));
    }
    void sum(size_t n, void* out) {
        std::vector<Jacobian<PallasFp>> parts;
        for (auto& sp : shards)
            if (sp->count(n)) parts.push_back(sp->partial);
        sum_parts(curve, parts, out);
    }
    ~lurk_hip_msm_multi() {
        for (auto& sp : shards) {
            Shard* shp = sp.get();
            if (!shp->worker) continue;
            shp->worker->post([shp] {
                shp->ctx.reset();
                shp->staged.release();
            });
            try { shp->worker->wait(); } catch (...) {}
        }
    }
};

namespace lurk {
int msm_multi_curve(const lurk_hip_msm_multi* key) {
    LURK_REQUIRE(key, "null key");
    return key->curve;
}
}  // namespace lurk

extern "C" {

int lurk_hip_msm_multi_create(lurk_hip_msm_multi** out, int curve, const void* bases, size_t n, const int* devices, int n_dev, int flags) {
    return guarded([&] {
        LURK_REQUIRE(out, "null ctx pointer");
        *out = nullptr;
        LURK_REQUIRE(curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN, "unknown curve id");
        LURK_REQUIRE(n == 0 || bases, "null bases");
        LURK_REQUIRE(devices && n_dev >= 1 && n_dev <= 64, "device list must hold 1..64 entries");
        const int have = lurk_hip_device_count();
        for (int i = 0; i < n_dev; i++) LURK_REQUIRE(devices[i] >= 0 && devices[i] < have, "device id out of range");
        auto m = std::make_unique<lurk_hip_msm_multi>();
        m->curve = curve;
        m->npoints = n;
        if (flags & LURK_MSM_FLAG_AUTO_SLICES) {
            // Every slice is a whole commitment: its own sort, plan and c - 1 reduction levels - ~0.64 ms of latency-bound chain on
            // one MI355X whatever its size - around 0.83 ms of accumulation per 2^20 points.  Below ~2^20 points
            // per slice the chain outweighs what another device takes off the accumulation (and on a list that repeats a device it is
            // pure overhead: +35 % for [0,0] at the rc = 100 step).  Use the first k devices of the list with k = max(1, n >> min_log).
            const char* e = getenv("LURK_MSM_MULTI_MIN_SLICE_LOG");
            int min_log = e ? atoi(e) : 20;
            if (min_log < 0) min_log = 0;
            if (min_log > 40) min_log = 40;
            size_t k = n >> min_log;
            if (k < 1) k = 1;
            if ((size_t)n_dev > k) n_dev = (int)k;
        }
        const size_t base = n / n_dev, extra = n % n_dev;  // the first n % n_dev shards hold one more point
        for (int i = 0; i < n_dev; i++) {
            auto sh = std::make_unique<lurk_hip_msm_multi::Shard>();
            sh->lo = (size_t)i * base + ((size_t)i < extra ? (size_t)i : extra);
            sh->hi = sh->lo + base + ((size_t)i < extra ? 1 : 0);
            sh->worker = std::make_unique<DeviceWorker>(devices[i]);
            m->shards.push_back(std::move(sh));
        }
        const char* hb = (const char*)bases;
        m->for_shards(n, [&](lurk_hip_msm_multi::Shard& sh, size_t, size_t cnt) {
            sh.ctx.reset(new_ctx(curve));
            DevBuf tmp(cnt * 64);
            LURK_HIP_CHECK(hipMemcpy(tmp.p, hb + sh.lo * 64, cnt * 64, hipMemcpyHostToDevice));
            ctx_set_bases(sh.ctx.get(), tmp.p, cnt, /*copy=*/true, flags, nullptr);
        });
        *out = m.release();
    });
}
int lurk_hip_msm_multi_shard(const lurk_hip_msm_multi* m, int index, int* device, size_t* first, size_t* count) {
    return guarded([&] {
        LURK_REQUIRE(m, "null ctx");
        LURK_REQUIRE(index >= 0 && (size_t)index < m->shards.size(), "shard index out of range");
        const auto& sh = *m->shards[index];
        if (device) *device = sh.worker->device();
        if (first) *first = sh.lo;
        if (count) *count = sh.hi - sh.lo;
    });
}
int lurk_hip_msm_multi_num_shards(const lurk_hip_msm_multi* m) { return m ? (int)m->shards.size() : 0; }

int lurk_hip_msm_multi_commit(lurk_hip_msm_multi* m, void* out, const void* scalars, size_t n, int is_mont) {
    return guarded([&] {
        LURK_REQUIRE(m && out, "null argument");
        LURK_REQUIRE(n <= m->npoints, "more scalars than bases in the context");
        LURK_REQUIRE(n == 0 || scalars, "null scalars");
        std::lock_guard<std::mutex> lk(m->mu);
        const char* hs = (const char*)scalars;
        m->for_shards(n, [&](lurk_hip_msm_multi::Shard& sh, size_t, size_t cnt) {
            sh.staged.ensure(cnt * 32);
            LURK_HIP_CHECK(hipMemcpy(sh.staged.p, hs + sh.lo * 32, cnt * 32, hipMemcpyHostToDevice));
            sh.ctx->run(sh.staged.p, cnt, is_mont, nullptr, &sh.partial);
        });
        m->sum(n, out);
    });
}
int lurk_hip_msm_multi_commit_dev(lurk_hip_msm_multi* m, void* out, const void* const* d_scalars, size_t n_slices, size_t n, int is_mont) {
    return guarded([&] {
        LURK_REQUIRE(m && out, "null argument");
        LURK_REQUIRE(n_slices == m->shards.size(), "one device pointer per shard is required (n_slices != number of shards)");
        LURK_REQUIRE(n <= m->npoints, "more scalars than bases in the context");
        LURK_REQUIRE(n == 0 || d_scalars, "null scalars");
        std::lock_guard<std::mutex> lk(m->mu);
        m->require_shard_pointers(d_scalars, n);
        m->for_shards(n, [&](lurk_hip_msm_multi::Shard& sh, size_t idx, size_t cnt) { sh.ctx->run(d_scalars[idx], cnt, is_mont, nullptr, &sh.partial); });
        m->sum(n, out);
    });
}
// Asynchronous form: the slices of one commitment are submitted on slot `slot` of every slice's context from the calling thread
// (each under its own device guard: a submit only enqueues) and run concurrently on their devices; wait collects the partial
// commitments in slice order and sums them with the host group law.  after_streams[i] (may be NULL) is the stream ON SLICE i's
// DEVICE that produced slice i's scalars, e.g. the stream a peer copy into that device was enqueued on.
int lurk_hip_msm_multi_submit_dev(lurk_hip_msm_multi* m, int slot, const void* const* d_scalars, void* const* after_streams, size_t n_slices, size_t n,
                                  int is_mont, int mode) {
    return guarded([&] {
        LURK_REQUIRE(m, "null ctx");
        LURK_REQUIRE(slot >= 0 && slot < MSM_SLOTS, "slot out of range");
        LURK_REQUIRE(n_slices == m->shards.size(), "one device pointer per shard is required (n_slices != number of shards)");
        LURK_REQUIRE(n <= m->npoints, "more scalars than bases in the context");
        LURK_REQUIRE(n == 0 || d_scalars, "null scalars");
        LURK_REQUIRE(mode >= LURK_MSM_SUBMIT_DEFAULT && mode <= LURK_MSM_SUBMIT_FOLLOW, "unknown submit mode");
        std::lock_guard<std::mutex> lk(m->mu);
        LURK_REQUIRE(!m->pending[slot], "slot is busy: wait for it first");
        m->require_shard_pointers(d_scalars, n);
        size_t done = 0;
        try {
            for (; done < m->shards.size(); done++) {
                auto& sh = *m->shards[done];
                const size_t cnt = sh.count(n);
                if (!cnt) continue;
                DeviceGuard dg(sh.worker->device());
                sh.ctx->submit(slot, d_scalars[done], cnt, is_mont, after_streams ? (hipStream_t)after_streams[done] : nullptr, mode);
            }
        } catch (...) {  // what was submitted is drained: the key stays usable
            for (size_t i = 0; i < done; i++) {
                auto& sh = *m->shards[i];
                if (!sh.count(n)) continue;
                try {
                    DeviceGuard dg(sh.worker->device());
                    sh.ctx->wait(slot, &sh.partial);
                } catch (...) {
                }
            }
            throw;
        }
        m->pending[slot] = true;
        m->pending_n[slot] = n;
    });
}
int lurk_hip_msm_multi_wait(lurk_hip_msm_multi* m, int slot, void* out) {
    return guarded([&] {
        LURK_REQUIRE(m && out, "null argument");
        LURK_REQUIRE(slot >= 0 && slot < MSM_SLOTS, "slot out of range");
        std::lock_guard<std::mutex> lk(m->mu);
        LURK_REQUIRE(m->pending[slot], "nothing was submitted on this slot");
        m->pending[slot] = false;
        const size_t n = m->pending_n[slot];
        std::unique_ptr<HipFailure> first;
        std::vector<Jacobian<PallasFp>> parts;
        for (auto& sp : m->shards) {
            auto& sh = *sp;
            if (!sh.count(n)) continue;
            Jacobian<PallasFp> part;
            try {  // every slice is waited for even if one fails: nothing stays in flight
                DeviceGuard dg(sh.worker->device());
                sh.ctx->wait(slot, &part);
                parts.push_back(part);
            } catch (const HipFailure& e) {
                if (!first) first.reset(new HipFailure(e));
            }
        }
        if (first) throw *first;
        lurk_hip_msm_multi::sum_parts(m->curve, parts, out);
    });
}
int lurk_hip_msm_multi_destroy(lurk_hip_msm_multi* m) {
    if (!m) return 0;
    return guarded([&] { delete m; });
}

}  // extern "C"
