// msm_keyfile.hip - a commitment key (msm.hip) saved to and loaded from a file.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "common.hpp"
#include "dispatch.hpp"
#include "msm_ctx.hpp"

using namespace lurk;

extern "C" {

// ---- key files ----------------------------------------------------------------------------------
// The reference keeps its public parameters - the commitment key is their bulk - in a disk cache and maps them back
// (/root/reference/src/public_parameters/mod.rs:33-56 "this clone is VERY expensive", disk_cache.rs:69-77).  A key file is the
// resident context's image: a 64-byte header, then the 64-byte affine records exactly as they sit in HBM (the bases; with
// with_table also the per-window multiples), so loading is open + mmap + copies straight into device memory, no parsing.
struct KeyFileHeader {
    char magic[8];  // "LURKHIPK"
    uint32_t version, curve, window_bits, windows;  // windows = 1: bases only
    uint64_t npoints, reserved[4];
};
static_assert(sizeof(KeyFileHeader) == 64, "key file header is 64 bytes");

int lurk_hip_msm_ctx_save(const lurk_hip_msm_ctx* ctx, const char* path, int with_table) {
    return guarded([&] {
        LURK_REQUIRE(ctx && path, "null argument");
        const MsmCtxBase& c = *ctx->impl;
        DeviceGuard dg(c.device);
        KeyFileHeader h{};
        memcpy(h.magic, "LURKHIPK", 8);
        h.version = 1;
        h.curve = (uint32_t)c.curve;
        h.window_bits = (uint32_t)c.c;
        h.windows = (with_table && c.precomputed && !c.small) ? (uint32_t)msm_num_windows(c.c) : 1u;  // the small form's table is rebuilt on load
        h.npoints = c.npoints;
        FILE* f = fopen(path, "wb");
        LURK_REQUIRE(f, std::string("cannot create ") + path);
        bool good = fwrite(&h, sizeof(h), 1, f) == 1;
        const size_t total = (size_t)h.windows * c.npoints * 64, chunk = (size_t)64 << 20;
        std::vector<char> buf(total < chunk ? total : chunk);
        for (size_t off = 0; good && off < total; off += chunk) {
            const size_t len = total - off < chunk ? total - off : chunk;
            if (hipMemcpy(buf.data(), (const char*)c.device_table() + off, len, hipMemcpyDeviceToHost) != hipSuccess) good = false;
            else good = fwrite(buf.data(), 1, len, f) == len;
        }
        good = (fclose(f) == 0) && good;
        LURK_REQUIRE(good, std::string("write failed: ") + path);
    });
}

// expect_curve >= 0: the file must hold a key of that curve (checked on the header, before anything is mapped or uploaded)
static void msm_ctx_load_impl(lurk_hip_msm_ctx** ctx, const char* path, int flags, int expect_curve);
int lurk_hip_msm_ctx_load(lurk_hip_msm_ctx** ctx, const char* path, int flags) {
    return guarded([&] { msm_ctx_load_impl(ctx, path, flags, -1); });
}
int lurk_hip_msm_ctx_load_curve(lurk_hip_msm_ctx** ctx, int curve, const char* path, int flags) {
    return guarded([&] {
        LURK_REQUIRE(curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN, "unknown curve id");
        msm_ctx_load_impl(ctx, path, flags, curve);
    });
}
static void msm_ctx_load_impl(lurk_hip_msm_ctx** ctx, const char* path, int flags, int expect_curve) {
    {
        LURK_REQUIRE(ctx && path, "null argument");
        *ctx = nullptr;
        const int fd = open(path, O_RDONLY);
        LURK_REQUIRE(fd >= 0, std::string("cannot open ") + path);
        struct stat st;
        KeyFileHeader h{};
        bool good = fstat(fd, &st) == 0 && (size_t)st.st_size >= sizeof(h) && pread(fd, &h, sizeof(h), 0) == (ssize_t)sizeof(h);
        good = good && memcmp(h.magic, "LURKHIPK", 8) == 0 && h.version == 1 && h.curve <= (uint32_t)LURK_CURVE_GRUMPKIN && h.windows >= 1 && h.windows <= MSM_MAX_W &&
               (h.windows == 1 || (h.window_bits >= 16 && h.window_bits <= 20 && h.windows == (uint32_t)msm_num_windows((int)h.window_bits))) &&
               h.npoints < ((uint64_t)1 << 31) && (uint64_t)st.st_size == sizeof(h) + (uint64_t)h.windows * h.npoints * 64;
        if (!good) {
            close(fd);
            LURK_REQUIRE(false, std::string("not a lurk-hip key file (or truncated): ") + path);
        }
        if (expect_curve >= 0 && (int)h.curve != expect_curve) {
            close(fd);
            LURK_REQUIRE(false, std::string("key file ") + path + " holds a " + curve_name((int)h.curve) + " key, not a " + curve_name(expect_curve) + " one");
        }
        const size_t n = h.npoints, total = (size_t)h.windows * n * 64;
        void* map = total ? mmap(nullptr, sizeof(h) + total, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
        close(fd);
        LURK_REQUIRE(!total || map != MAP_FAILED, std::string("mmap failed: ") + path);
        std::unique_ptr<MsmCtxBase> c(new_ctx((int)h.curve));
        try {
            const bool want_table = (flags & LURK_MSM_FLAG_PRECOMPUTE) != 0;
            DevBuf buf(total);
            if (total) LURK_HIP_CHECK(hipMemcpy(buf.p, (const char*)map + sizeof(h), total, hipMemcpyHostToDevice));
            if (h.windows > 1 && want_table) {
                c->adopt_table(std::move(buf), n, true, (int)h.window_bits);  // the file's table as it is
            } else if (want_table) {
                ctx_set_bases(c.get(), buf.p, n, false, flags, nullptr);      // bases from the file, table rebuilt on the device
            } else {
                DevBuf bases(n * 64);  // bases only (drop a table the caller did not ask for)
                if (n) LURK_HIP_CHECK(hipMemcpy(bases.p, buf.p, n * 64, hipMemcpyDeviceToDevice));
                c->adopt_table(std::move(bases), n, false, MSM_C_PLAIN);
            }
        } catch (...) {
            if (map) munmap(map, sizeof(h) + total);
            throw;
        }
        if (map) munmap(map, sizeof(h) + total);
        *ctx = new lurk_hip_msm_ctx{std::move(c)};
    }
}

}  // extern "C"
