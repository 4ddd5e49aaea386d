// msm_ctx.hpp - what the MSM's translation units share of a commitment-key context: the interface MsmCtx<P, SF> (msm.hip) implements
// and the handle behind the C ABI.  The one-shot symbols (msm_oneshot.hip), key files (msm_keyfile.hip), the multi-device key
// (msm_multi.hip) and the folded-child registry (msm_folded.hip) see a context through this header alone.
#pragma once
#include <memory>

#include "common.hpp"
#include "msm_core.cuh"

namespace lurk {

struct MsmCtxBase {
    int curve = 0;
    int device = 0;  // the device the context lives on: every entry point runs under a DeviceGuard for it
    size_t npoints = 0;
    bool precomputed = false;
    bool small = false;  // precomputed in the small-commitment form (msm_small.hip): `c` is its window width, no bucket pipeline
    int c = MSM_C_PLAIN;
    bool keep_buffers = false;  // a context whose points are replaced again and again (the inner-product argument's folded key): the table
                                // buffer and the precomputation's scratch stay allocated between set_bases_device calls
    virtual ~MsmCtxBase() {}
    // synchronous: enqueue on `s` with slot 0's workspace, wait, host tail
    virtual void run(const void* d_scalars, size_t n, int is_mont, hipStream_t s, void* out_jac96_host) = 0;
    // asynchronous: enqueue on the slot's own stream (after `after`, the stream that produced the scalars)
    virtual void submit(int slot, const void* d_scalars, size_t n, int is_mont, hipStream_t after, int mode) = 0;
    virtual void wait(int slot, void* out_jac96_host) = 0;
    // two commitments with disjoint supports in one pass: scalars whose index has bit sel_bit clear -> out_lo, set -> out_hi
    virtual void submit_pair(int slot, const void* d_scalars, size_t n, int is_mont, hipStream_t after, int sel_bit) = 0;
    // xyzz: the two results as XYZZ points (128 B each), not normalised: no field inversion; otherwise 96-byte Jacobian points with Z = 1
    virtual void wait_pair(int slot, void* out_lo_host, void* out_hi_host, bool xyzz) = 0;
    // a batch of short commitments under prefixes of the key in one pass (msm_batch.hip); offsets / lens: host arrays, elements of 32 B
    virtual void submit_batch(int slot, const void* d_scalars, const size_t* offsets, const size_t* lens, size_t count, int is_mont, hipStream_t after) = 0;
    virtual void wait_batch(int slot, void* out_jac96_host /* count x 96 B */) = 0;
    // pasta-msm's calling convention: everything in host memory, nothing resident (buffers and workspaces are kept for the next call)
    virtual void run_oneshot(const void* bases, const void* scalars, size_t n, int is_mont, void* out_jac96_host) = 0;
    virtual void rebind(const void* d_bases, size_t n) = 0;  // plain key over other (borrowed) device bases, workspaces kept
    virtual void reserve(size_t n, int slots) = 0;  // allocate the workspaces of slots 0..slots-1 for n scalars now
    virtual const void* device_table() const = 0;  // npoints (x windows when precomputed) 64-byte records
    // adopt a table that is already complete in device memory (loaded from a key file)
    virtual void adopt_table(DevBuf&& buf, size_t n, bool precomputed_, int c_) = 0;
};

MsmCtxBase* new_ctx(int curve);  // an empty context of the curve on the current device
// flags: LURK_MSM_FLAG_* of the C ABI; copy = false borrows d_bases (a table form always owns its copy)
void ctx_set_bases(MsmCtxBase* c, const void* d_bases, size_t n, bool copy, int flags, hipStream_t s);

bool oneshot_key_cache_enabled();  // the switch of lurk_hip_msm_oneshot_key_cache (msm_oneshot.hip)

}  // namespace lurk

struct lurk_hip_msm_ctx {
    std::unique_ptr<lurk::MsmCtxBase> impl;
};
