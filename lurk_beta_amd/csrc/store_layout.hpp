// store_layout.hpp - what the one-shot hydration (store.hip) and the resident store (store_resident.hip) share: the shape of the
// StoreHasher preimages (/root/reference/src/lem/store.rs:29-78) per node kind and the width below which a group goes to the host.
#pragma once
#include "common.hpp"

namespace lurk {

// groups of at most this many nodes are hashed on the host: device level time / host hash time = 0.138 ms / ~20 us
constexpr uint32_t STORE_HOST_MAX = 6;

inline int kind_arity(uint32_t kind) {
    switch (kind) {
        case LURK_NODE_TUPLE2: return 4;
        case LURK_NODE_TUPLE3: return 6;
        case LURK_NODE_TUPLE4: return 8;
        case LURK_NODE_COMPACT: return 4;
        case LURK_NODE_COMM: return 3;
        default: return 0;
    }
}
inline int kind_children(uint32_t kind) {
    switch (kind) {
        case LURK_NODE_TUPLE2: return 2;
        case LURK_NODE_TUPLE3: return 3;
        case LURK_NODE_TUPLE4: return 4;
        case LURK_NODE_COMPACT: return 3;
        case LURK_NODE_COMM: return 1;
        default: return 0;
    }
}

}  // namespace lurk
