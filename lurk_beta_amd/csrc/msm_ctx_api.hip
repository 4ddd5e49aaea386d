// msm_ctx_api.hip - the lurk_hip_msm_ctx_* entry points of the C ABI over a commitment-key context (msm_ctx.hpp; MsmCtx<P, SF>: msm.hip), and
// what the library's other units read of a context (common.hpp).
#include "common.hpp"
#include "dispatch.hpp"
#include "msm_ctx.hpp"

namespace lurk {

void keygen_from_label_device(int curve, const void* label, size_t label_len, size_t n, void* d_out, hipStream_t s);  // keygen.hip

void msm_ctx_wait_pair_xyzz(lurk_hip_msm_ctx* ctx, int slot, void* out_lo_xyzz128, void* out_hi_xyzz128) {
    LURK_REQUIRE(ctx && out_lo_xyzz128 && out_hi_xyzz128, "null argument");
    DeviceGuard dg(ctx->impl->device);
    ctx->impl->wait_pair(slot, out_lo_xyzz128, out_hi_xyzz128, /*xyzz=*/true);
}
MsmTableView msm_ctx_table_view(const lurk_hip_msm_ctx* ctx) {
    LURK_REQUIRE(ctx, "null ctx");
    const MsmCtxBase& c = *ctx->impl;
    MsmTableView v;
    v.table = c.device_table();
    v.npoints = c.npoints;
    v.curve = c.curve;
    v.window_bits = c.c;
    v.form = c.small ? LURK_MSM_FORM_SMALL : c.precomputed ? LURK_MSM_FORM_TABLE : LURK_MSM_FORM_PLAIN;
    v.windows = v.form == LURK_MSM_FORM_TABLE ? msm_num_windows(c.c) : 1;
    v.device = c.device;
    return v;
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_msm_ctx_create(lurk_hip_msm_ctx** ctx, int curve, const void* bases, size_t n, int flags) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "null ctx pointer");
        LURK_REQUIRE(n == 0 || bases, "null bases");
        std::unique_ptr<MsmCtxBase> c(new_ctx(curve));
        DevBuf tmp(n * 64);
        if (n) LURK_HIP_CHECK(hipMemcpy(tmp.p, bases, n * 64, hipMemcpyHostToDevice));
        ctx_set_bases(c.get(), tmp.p, n, /*copy=*/true, flags, nullptr);
        *ctx = new lurk_hip_msm_ctx{std::move(c)};
    });
}
int lurk_hip_msm_ctx_create_dev(lurk_hip_msm_ctx** ctx, int curve, const void* d_bases, size_t n, int flags, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "null ctx pointer");
        LURK_REQUIRE(n == 0 || d_bases, "null bases");
        std::unique_ptr<MsmCtxBase> c(new_ctx(curve));
        ctx_set_bases(c.get(), d_bases, n, /*copy=*/false, flags, (hipStream_t)stream);
        *ctx = new lurk_hip_msm_ctx{std::move(c)};
    });
}
int lurk_hip_msm_ctx_run(lurk_hip_msm_ctx* ctx, void* out, const void* scalars, size_t n, int is_mont) {
    return guarded([&] {
        LURK_REQUIRE(ctx && out, "null argument");
        LURK_REQUIRE(n == 0 || scalars, "null scalars");
        DeviceGuard dg(ctx->impl->device);
        DevBuf ds(n * 32);
        if (n) LURK_HIP_CHECK(hipMemcpy(ds.p, scalars, n * 32, hipMemcpyHostToDevice));
        ctx->impl->run(ds.p, n, is_mont, nullptr, out);
    });
}
int lurk_hip_msm_ctx_run_dev(lurk_hip_msm_ctx* ctx, void* out, const void* d_scalars, size_t n, int is_mont, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(ctx && out, "null argument");
        LURK_REQUIRE(n == 0 || d_scalars, "null scalars");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->run(d_scalars, n, is_mont, (hipStream_t)stream, out);
    });
}
int lurk_hip_msm_ctx_submit_dev(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars, size_t n, int is_mont, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "null ctx");
        LURK_REQUIRE(n == 0 || d_scalars, "null scalars");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->submit(slot, d_scalars, n, is_mont, (hipStream_t)stream, LURK_MSM_SUBMIT_DEFAULT);
    });
}
int lurk_hip_msm_ctx_submit_dev_mode(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars, size_t n, int is_mont, void* stream, int mode) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "null ctx");
        LURK_REQUIRE(n == 0 || d_scalars, "null scalars");
        LURK_REQUIRE(mode >= LURK_MSM_SUBMIT_DEFAULT && mode <= LURK_MSM_SUBMIT_FOLLOW, "unknown submit mode");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->submit(slot, d_scalars, n, is_mont, (hipStream_t)stream, mode);
    });
}
int lurk_hip_msm_ctx_submit_pair_dev(lurk_hip_msm_ctx* ctx, int slot, const void* d_scalars, size_t n, int is_mont, void* stream, int sel_bit) {
    return guarded([&] {
        LURK_REQUIRE(ctx && d_scalars, "null argument");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->submit_pair(slot, d_scalars, n, is_mont, (hipStream_t)stream, sel_bit);
    });
}
int lurk_hip_msm_ctx_wait_pair(lurk_hip_msm_ctx* ctx, int slot, void* out_lo, void* out_hi) {
    return guarded([&] {
        LURK_REQUIRE(ctx && out_lo && out_hi, "null argument");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->wait_pair(slot, out_lo, out_hi, /*xyzz=*/false);
    });
}
int lurk_hip_msm_ctx_wait(lurk_hip_msm_ctx* ctx, int slot, void* out) {
    return guarded([&] {
        LURK_REQUIRE(ctx && out, "null argument");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->wait(slot, out);
    });
}
int lurk_hip_msm_ctx_destroy(lurk_hip_msm_ctx* ctx) {
    if (!ctx) return 0;
    return guarded([&] {
        DeviceGuard dg(ctx->impl->device);
        lurk::msm_ctx_drop_folded_child(ctx);
        delete ctx;
    });
}

int lurk_hip_msm_ctx_rebind_dev(lurk_hip_msm_ctx* ctx, const void* d_bases, size_t npoints) {
    return guarded([&] {
        LURK_REQUIRE(ctx && (npoints == 0 || d_bases), "null argument");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->rebind(d_bases, npoints);
    });
}
int lurk_hip_msm_ctx_reserve(lurk_hip_msm_ctx* ctx, size_t nscalars, int slots) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "null ctx");
        DeviceGuard dg(ctx->impl->device);
        ctx->impl->reserve(nscalars, slots);
    });
}
int lurk_hip_msm_ctx_from_label(lurk_hip_msm_ctx** ctx, int curve, const void* label, size_t label_len, size_t npoints, int flags) {
    return guarded([&] {
        LURK_REQUIRE(ctx && (label || label_len == 0), "null argument");
        *ctx = nullptr;
        require_pasta_curve(curve, "lurk_hip_msm_ctx_from_label (hash-to-curve)");
        std::unique_ptr<MsmCtxBase> c(new_ctx(curve));
        DevBuf bases(npoints * 64);
        keygen_from_label_device(curve, label, label_len, npoints, bases.p, nullptr);
        if (flags & LURK_MSM_FLAG_PRECOMPUTE) ctx_set_bases(c.get(), bases.p, npoints, false, flags, nullptr);  // the table owns its copy
        else c->adopt_table(std::move(bases), npoints, false, MSM_C_PLAIN);
        *ctx = new lurk_hip_msm_ctx{std::move(c)};
    });
}
int lurk_hip_msm_ctx_device(const lurk_hip_msm_ctx* ctx, int* device) {
    return guarded([&] {
        LURK_REQUIRE(ctx && device, "null argument");
        *device = ctx->impl->device;
    });
}
int lurk_hip_msm_ctx_info(const lurk_hip_msm_ctx* ctx, int* curve, size_t* npoints, int* window_bits, int* precomputed) {
    return guarded([&] {
        LURK_REQUIRE(ctx, "null ctx");
        if (curve) *curve = ctx->impl->curve;
        if (npoints) *npoints = ctx->impl->npoints;
        if (window_bits) *window_bits = ctx->impl->c;
        if (precomputed) *precomputed = (ctx->impl->small || ctx->impl->precomputed) ? 1 : 0;  // a boolean, as before the small form existed
    });
}
int lurk_hip_msm_ctx_form(const lurk_hip_msm_ctx* ctx, int* form) {
    return guarded([&] {
        LURK_REQUIRE(ctx && form, "null argument");
        *form = ctx->impl->small ? LURK_MSM_FORM_SMALL : ctx->impl->precomputed ? LURK_MSM_FORM_TABLE : LURK_MSM_FORM_PLAIN;
    });
}

}  // extern "C"
