// msm_oneshot.hip - pasta-msm's / grumpkin-msm's calling convention over the resident-bases context (msm.hip): bases and scalars in host
// memory at every call, nothing resident for the caller.  The twelve symbols an unmodified arecibo links: lurk_hip_msm_<curve>,
// mult_pippenger_<curve>, cuda_pippenger_<curve>.
#include <atomic>

#include "common.hpp"
#include "msm_ctx.hpp"

namespace lurk {

static int oneshot_key_cache_env() {
    const char* v = getenv("LURK_MSM_ONESHOT_KEY_CACHE");
    return v && atoi(v) != 0;
}
static std::atomic<int> g_oneshot_key_cache{oneshot_key_cache_env()};
bool oneshot_key_cache_enabled() { return g_oneshot_key_cache.load() != 0; }

static int msm_oneshot(int curve, void* out, const void* bases, size_t n, const void* scalars, int is_mont) {
    return guarded([&] {
        LURK_REQUIRE(out, "null output");
        LURK_REQUIRE(n == 0 || (bases && scalars), "null buffer");
        // one cached context per (device, curve): its device buffers and workspaces survive between calls, so an unmodified caller
        // of the pasta-msm symbols pays PCIe (96 B per point) but no allocation.  Calls on one (device, curve) serialise.
        static std::mutex mu;
        static std::map<std::pair<int, int>, std::unique_ptr<MsmCtxBase>> cache;
        MsmCtxBase* c;
        {
            std::lock_guard<std::mutex> lk(mu);
            auto key = std::make_pair(current_device(), curve);
            auto it = cache.find(key);
            if (it == cache.end()) it = cache.emplace(key, std::unique_ptr<MsmCtxBase>(new_ctx(curve))).first;
            c = it->second.get();
        }
        c->run_oneshot(bases, scalars, n, is_mont, out);
    });
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_msm_pallas(void* out, const void* bases, size_t n, const void* scalars, int is_mont) {
    return msm_oneshot(LURK_CURVE_PALLAS, out, bases, n, scalars, is_mont);
}
int lurk_hip_msm_vesta(void* out, const void* bases, size_t n, const void* scalars, int is_mont) {
    return msm_oneshot(LURK_CURVE_VESTA, out, bases, n, scalars, is_mont);
}
int lurk_hip_msm_bn254(void* out, const void* bases, size_t n, const void* scalars, int is_mont) {
    return msm_oneshot(LURK_CURVE_BN254, out, bases, n, scalars, is_mont);
}
int lurk_hip_msm_grumpkin(void* out, const void* bases, size_t n, const void* scalars, int is_mont) {
    return msm_oneshot(LURK_CURVE_GRUMPKIN, out, bases, n, scalars, is_mont);
}

// pasta-msm's own C symbols: they return nothing (its CPU Pippenger cannot fail), so a failure here ends the process with the
// library's message - never a silent wrong commitment, never a CPU fallback
static void pasta_msm_symbol(int curve, void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    if (msm_oneshot(curve, out, points, npoints, scalars, is_mont ? 1 : 0) != 0) {
        static const char* const names[] = {"pallas", "vesta", "bn254", "grumpkin"};
        fprintf(stderr, "liblurk_hip: mult_pippenger_%s failed: %s\n", names[curve], lurk_hip_last_error());
        abort();
    }
}
void mult_pippenger_pallas(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    pasta_msm_symbol(LURK_CURVE_PALLAS, out, points, npoints, scalars, is_mont);
}
void mult_pippenger_vesta(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    pasta_msm_symbol(LURK_CURVE_VESTA, out, points, npoints, scalars, is_mont);
}

// pasta-msm's GPU entry points (its `cuda` feature, sppark's calling convention): the same arguments, a RustError {code, message} returned
// BY VALUE - message is a malloc'd C string the Rust side frees (sppark's `impl Drop for Error`), NULL on success.  What arecibo's GPU
// path binds instead of mult_pippenger_* (SURVEY.md section 8b).
static lurk_hip_rust_error rust_error_from(int rc) {
    lurk_hip_rust_error e;
    e.code = rc;
    e.message = rc == 0 ? nullptr : strdup(lurk_hip_last_error());
    return e;
}
lurk_hip_rust_error cuda_pippenger_pallas(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    return rust_error_from(msm_oneshot(LURK_CURVE_PALLAS, out, points, npoints, scalars, is_mont ? 1 : 0));
}
lurk_hip_rust_error cuda_pippenger_vesta(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    return rust_error_from(msm_oneshot(LURK_CURVE_VESTA, out, points, npoints, scalars, is_mont ? 1 : 0));
}
// grumpkin-msm's names (the BN254 / Grumpkin cycle), the same behaviour
void mult_pippenger_bn254(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    pasta_msm_symbol(LURK_CURVE_BN254, out, points, npoints, scalars, is_mont);
}
void mult_pippenger_grumpkin(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    pasta_msm_symbol(LURK_CURVE_GRUMPKIN, out, points, npoints, scalars, is_mont);
}
lurk_hip_rust_error cuda_pippenger_bn254(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    return rust_error_from(msm_oneshot(LURK_CURVE_BN254, out, points, npoints, scalars, is_mont ? 1 : 0));
}
lurk_hip_rust_error cuda_pippenger_grumpkin(void* out, const void* points, size_t npoints, const void* scalars, bool is_mont) {
    return rust_error_from(msm_oneshot(LURK_CURVE_GRUMPKIN, out, points, npoints, scalars, is_mont ? 1 : 0));
}

int lurk_hip_msm_oneshot_key_cache(int enable) {
    return guarded([&] { g_oneshot_key_cache.store(enable ? 1 : 0); });
}

}  // extern "C"
