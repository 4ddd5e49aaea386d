// msm_folded.hip - the registry of folded-key contexts (msm_ctx.hpp), one per parent key.
#include "common.hpp"
#include "dispatch.hpp"
#include "msm_ctx.hpp"

namespace lurk {
// The folded key of the inner-product argument (ipa.hip) as a context that belongs to its parent key: created at the first proof, its
// points replaced (table rebuilt in place, workspaces kept) at every later one - creating and destroying a 65 536-point table key per
// proof cost 3-4 ms of hipMalloc / hipFree on the host.  One argument at a time holds it; a second one under the same key at the same
// moment gets a private context (owned = true).
struct FoldedChild {
    std::unique_ptr<lurk_hip_msm_ctx> ctx;
    std::mutex mu;
};
static std::mutex g_children_mu;
// (never destroyed: a key its owner forgot to destroy must not have its child's streams and buffers released by a static destructor
// after the HIP runtime has shut down)
static auto& g_children = *new std::map<const lurk_hip_msm_ctx*, std::unique_ptr<FoldedChild>>();

FoldedKeyLease::~FoldedKeyLease() {
    if (owned && ctx) (void)lurk_hip_msm_ctx_destroy(ctx);
}
FoldedKeyLease msm_ctx_folded_child(lurk_hip_msm_ctx* parent, const void* d_points, size_t m, hipStream_t s) {
    LURK_REQUIRE(parent && d_points && m, "null argument");
    const int curve = parent->impl->curve;
    require_pasta_curve(curve, "the inner-product argument's folded key");
    const int flags = LURK_MSM_FLAG_PRECOMPUTE | LURK_MSM_FLAG_WINDOW_BITS(16);
    FoldedChild* fc = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_children_mu);
        auto& slot = g_children[parent];
        if (!slot) slot.reset(new FoldedChild);
        fc = slot.get();
    }
    FoldedKeyLease lease;
    lease.lk = std::unique_lock<std::mutex>(fc->mu, std::try_to_lock);
    if (!lease.lk.owns_lock()) {  // somebody else's argument holds the parent's child: a private one
        if (lurk_hip_msm_ctx_create_dev(&lease.ctx, curve, d_points, m, flags, (void*)s) != 0) throw HipFailure{LURK_HIP_ERR_HIP, lurk_hip_last_error()};
        lease.owned = true;
        return lease;
    }
    if (!fc->ctx) {
        std::unique_ptr<MsmCtxBase> c(new_ctx(curve));
        c->keep_buffers = true;
        ctx_set_bases(c.get(), d_points, m, /*copy=*/false, flags, s);
        fc->ctx.reset(new lurk_hip_msm_ctx{std::move(c)});
    } else {
        ctx_set_bases(fc->ctx->impl.get(), d_points, m, /*copy=*/false, flags, s);
    }
    lease.ctx = fc->ctx.get();
    return lease;
}
void msm_ctx_drop_folded_child(const lurk_hip_msm_ctx* parent) {
    std::unique_ptr<FoldedChild> dead;
    {
        std::lock_guard<std::mutex> lk(g_children_mu);
        auto it = g_children.find(parent);
        if (it == g_children.end()) return;
        dead = std::move(it->second);
        g_children.erase(it);
    }
    if (dead->ctx) {
        msm_ctx_drop_folded_child(dead->ctx.get());  // (a folded key long enough to have been folded again)
        dead->ctx.reset();
    }
}

}  // namespace lurk
