// r1cs_shape.cuh - the resident relaxed-R1CS shape as the translation units that run on it see it (fold.hip: multiply_vec, the cross
// terms; r1cs_sat.hip: the satisfiability check): the CSR matrices with their coefficient dictionary, the lazy row accumulator and the
// XCD-aware row-block mapping.  fold.hip creates and destroys shapes; layout and bounds are argued there.
#pragma once
#include <memory>
#include <mutex>

#include "common.hpp"
#include "poseidon29.cuh"

namespace lurk {

constexpr int FOLD_BLOCK = 256;

// Row classes of the satisfiability check, by the longest of a row's three linear combinations: one lane per row, a sub-wave group per
// mid-length row, 16 lanes per long row.  rows = [wide | mid | lane] row ids, ascending inside each class.
struct SatPlan {
    DevBuf rows;
    size_t n_wide = 0, n_mid = 0, n_lane = 0;
    uint32_t lane_max = 0, mid_max = 0;  // the class bounds the lists were built for
    DevBuf rec;                          // {failing rows, lowest failing row}: 2 x u64
    uint64_t* host = nullptr;            // pinned: [0, 1] the record's initial value, [2, 3] the record read back
    ~SatPlan() {
        if (host) (void)hipHostFree(host);
    }
};

// Row classes of the sparse multilinear evaluation (verify.hip), as above but over the rows that have an entry at all: a row
// without one contributes nothing and is not visited.  Built on the first call, immutable afterwards.
struct MlePlan {
    DevBuf rows;  // [wide | mid | lane] row ids
    size_t n_wide = 0, n_mid = 0, n_lane = 0;
    uint64_t max_col = 0;  // the largest column index of the three matrices (0 for an empty shape)
};

struct CsrDev {
    DevBuf rowptr;  // u32 x (rows + 1)
    DevBuf ent;     // uint2 {col, coefficient id} x nnz
    size_t nnz = 0;
};

struct R1csShape {
    int field_id = 0;
    size_t num_cons = 0, num_vars = 0, num_io = 0;
    CsrDev m[3];
    DevBuf dict;  // distinct coefficients, P29_STRIDE words each (canonical Montgomery-2^261 limbs)
    size_t dict_size = 0;
    DevBuf long_rows;  // u32 row ids with more than FOLD_LONG entries in A, B or C
    size_t n_long = 0;
    int device = 0;
    // lurk_hip_r1cs_is_sat_dev's row classes (r1cs_sat.hip): built on the first call, so that a shape that is never checked pays nothing
    mutable std::mutex sat_mu;
    mutable std::unique_ptr<SatPlan> sat;
    // lurk_hip_r1cs_sparse_mle_dev's row classes (verify.hip): built on the first call under mle_mu, read-only afterwards
    mutable std::mutex mle_mu;
    mutable std::unique_ptr<MlePlan> mle;
};

// ---- rows --------------------------------------------------------------------------------------------------
// Lazy accumulator of one row value: terms a*b (both tight) are added as unreduced 17-column products.
// 45 products per column fit 64 bits: the columns are normalised every fourth term.  Every term adds < 2^253
// to the value: every 64 terms the reduced partial sum re-enters as one term (times the Montgomery one) so that
// rows of any length stay below 2^261.
template <class P>
struct RowAcc {
    Dot29<P> acc;
    uint32_t since, terms;
};
template <class P>
__device__ __forceinline__ void row_init(RowAcc<P>& r) {
    dot29_init<P>(r.acc);
    r.since = 0;
    r.terms = 0;
}
template <class P>
__device__ __forceinline__ void row_mac(RowAcc<P>& r, const F29<P>& a, const F29<P>& b, const uint32_t* one29) {
    if (r.terms == 64) {
        F29<P> part = dot29_finish<P>(r.acc);
        dot29_init<P>(r.acc);
        dot29_mac<P>(r.acc, part, ld_const29<P>(one29));
        r.terms = 1;
        r.since = 1;
    }
    if (r.since == 4) {
        dot29_carry<P>(r.acc);
        r.since = 0;
    }
    dot29_mac<P>(r.acc, a, b);
    r.since++;
    r.terms++;
}

struct CsrView {
    const uint32_t* rowptr;
    const uint2* ent;
};

struct R1csDev {
    CsrView a, b, c;
    const uint32_t* dict;
    size_t dict_size;
    size_t rows;
    const uint32_t* long_rows;  // rows with > FOLD_LONG entries in A, B or C
    uint32_t n_long;
};

// Workgroup -> row block, XCD-aware.  Consecutive workgroup ids go round the 8 XCDs (each with its own 4 MiB L2), and the rows of the
// step circuit are frame-structured: a frame's rows gather almost only that frame's ~9 000 columns of z (multiframe.rs:699-702).  With
// the identity mapping every XCD's L2 sees every frame's columns (each 32-byte element of z is fetched into up to 8 L2s); here XCD x
// walks ONE contiguous eighth of the rows, so a frame's columns of z1 / z2 are fetched by one L2 and hit there for the rest of the
// frame's rows.
constexpr unsigned FOLD_XCDS = 8;
__device__ __forceinline__ size_t fold_row_block(unsigned b, unsigned nblocks) {
    const unsigned per = (nblocks + FOLD_XCDS - 1) / FOLD_XCDS;
    return (size_t)(b % FOLD_XCDS) * per + b / FOLD_XCDS;
}

static R1csDev dev_view(const R1csShape& sh) {
    R1csDev d;
    d.a = CsrView{sh.m[0].rowptr.as<uint32_t>(), sh.m[0].ent.as<uint2>()};
    d.b = CsrView{sh.m[1].rowptr.as<uint32_t>(), sh.m[1].ent.as<uint2>()};
    d.c = CsrView{sh.m[2].rowptr.as<uint32_t>(), sh.m[2].ent.as<uint2>()};
    d.dict = sh.dict.as<uint32_t>();
    d.dict_size = sh.dict_size;
    d.rows = sh.num_cons;
    d.long_rows = sh.long_rows.as<uint32_t>();
    d.n_long = (uint32_t)sh.n_long;
    return d;
}

}  // namespace lurk

struct lurk_hip_r1cs {
    lurk::R1csShape sh;  // immutable after creation (but for the lazily built sat plan, under its own lock): calls on one shape from any thread / stream are independent
};

