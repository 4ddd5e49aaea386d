// r1cs_shape.cuh - the resident relaxed-R1CS shape and what every kernel that walks its matrices shares (fold.hip: multiply_vec, the
// cross terms; r1cs_sat.hip: the satisfiability check; verify.hip: the sparse multilinear evaluation; r1cs_transpose.hip):
//   the shape      the CSR matrices with their coefficient dictionary (R1csShape / R1csDev); fold.hip creates and destroys shapes and
//                  argues the layout
//   the row        r1cs_row: the lazy inner product of one CSR row with a dense vector, by one lane or a group of lanes, with the
//                  bounds of its accumulation (RowAcc) - the one definition of the row loop
//   the classes    RowClasses / RowClassDev: rows sorted into lane, mid and wide rows by length, built on the host once per plan
//                  (build_row_classes) and walked as virtual blocks of one launch (row_class_vblock); FOLD_LONG, fold.hip's own bound
//   the lanes      fold_row_block (XCD-aware workgroup -> row block), class_blocks, and row_slot: which row a lane works on, with the
//                  rule for a group of lanes that has no row
#pragma once
#include <algorithm>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "poseidon29.cuh"

namespace lurk {

constexpr int FOLD_BLOCK = 256;
constexpr uint32_t FOLD_LONG = 32;  // fold.hip: rows with more entries (in any of A, B, C) leave the lane-per-row kernels for FOLD_GROUP lanes per row
constexpr int FOLD_GROUP = 16;
// Entries whose loads one lane issues together.  Measured in isolation at rc = 100 (bench_tools/fold_bench.py, round 6): a batch of 4
// entries keeps 180-200 registers live (two waves per SIMD), a batch of 2 keeps 144 (three waves): 0.227 -> 0.200 ms for the
// cached-products kernel, 0.323 -> 0.312 for the six-gather one - the kernels are bound by gather latency that only more resident waves
// hide (1.6 waves per SIMD on average in round 4's counters).
#ifndef LURK_FOLD_BATCH
#define LURK_FOLD_BATCH 2
#endif
constexpr int FOLD_BATCH = LURK_FOLD_BATCH;

// Row classes, by the longest of a row's three linear combinations (the satisfiability check and the sparse multilinear evaluation;
// fold.hip keeps its own two-way split at FOLD_LONG):
//     lane   <= SAT_LANE_MAX entries        one lane per row
//     mid    <= SAT_MID_MAX                 SAT_GROUP lanes per row (at most 256 entries: the group adds its partial sums limb-wise)
//     wide   the rest (bit decompositions)  SAT_WIDE_GROUP lanes per row, any length
constexpr uint32_t SAT_LANE_MAX = 8;  // defaults of the class bounds (is_sat: LURK_SAT_LANE_MAX / LURK_SAT_MID_MAX override them for measurements)
constexpr uint32_t SAT_MID_MAX = 96;
constexpr uint32_t SAT_GROUP = 4;  // lanes per mid-length row: 4 / 8 / 16 measured 0.242 / 0.285 / 0.384 ms at rc = 100
constexpr int SAT_WIDE_GROUP = 16;

// rows = [wide | mid | lane] row ids, ascending inside each class
struct RowClasses {
    DevBuf rows;
    size_t n_wide = 0, n_mid = 0, n_lane = 0;
    uint32_t lane_max = 0, mid_max = 0;  // the class bounds the lists were built for
};

// lurk_hip_r1cs_is_sat_dev's plan (r1cs_sat.hip): every row, empty ones included
struct SatPlan {
    RowClasses cls;
    DevBuf rec;                // {failing rows, lowest failing row}: 2 x u64
    uint64_t* host = nullptr;  // pinned: [0, 1] the record's initial value, [2, 3] the record read back
    ~SatPlan() {
        if (host) (void)hipHostFree(host);
    }
};

// lurk_hip_r1cs_sparse_mle_dev's plan (verify.hip): the rows that have an entry at all - a row without one contributes nothing and is
// not visited.  Built on the first call, immutable afterwards.
struct MlePlan {
    RowClasses cls;
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
// Every kernel that walks the matrices forms the inner product of one CSR row with a dense vector through r1cs_row below.  Its bounds,
// argued here once (radix-2^29 limbs, Montgomery-2^261 values; "tight": limbs < 2^29, value < 2^258.1):
//   a term      coefficient (canonical, from the dictionary) x vector element (f29_from_mont256: tight) is added to RowAcc as an
//               unreduced 17-column product.  45 products per column fit 64 bits: the columns are normalised every fourth term.
//   a row       every term adds < 2^253 to the value.  Every 64 terms the reduced partial sum re-enters as ONE term (times the
//               Montgomery one), so that a row of any length stays below 2^261 and dot29_finish returns a tight value.
//   a group     G lanes share a row: lane g accumulates entries g, g + G, ... and reduces its own partial sum.  The partial sums are
//               then added across the group limb-wise, two butterfly steps between carry passes (4 x 2^29 < 2^32), while the row is
//               short enough for their sum to stay below 2^261: <= 256 entries (< 256 * 2^252 + 16 p).  Beyond 256 entries they enter
//               the group leader's RowAcc one by one (times the Montgomery one), under the row bound above.
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

// LDS = true: the dictionary (and the Montgomery one that closes it) was copied into LDS, plain reads
template <class P, bool LDS>
__device__ __forceinline__ F29<P> r1cs_coeff(const uint32_t* dict, uint32_t id) {
    const uint32_t* p = dict + (size_t)id * P29_STRIDE;
    if (!LDS) return ld_const29<P>(p);
    F29<P> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
    return r;
}

// G lanes, one row of one matrix times z: lane gl of the group accumulates entries lo + gl, lo + gl + G, ..., FOLD_BATCH of them at a
// time so that the dependent loads of a batch (record -> coefficient, element of z) are in flight together; for G > 1 the reduced
// partial sums are added across the group (valid on the group's first lane; every lane of the group must arrive).  ANY_LEN = false: the
// caller guarantees at most 256 entries.  one29: the Montgomery one, the dictionary's closing record.
template <class P, int G, bool ANY_LEN, bool LDS>
__device__ __forceinline__ F29<P> r1cs_row(const CsrView& m, const uint32_t* dict, const uint32_t* one29, uint32_t lo, uint32_t hi, uint32_t gl,
                                          const Fe<P>* __restrict__ z) {
    RowAcc<P> acc;
    row_init<P>(acc);
    for (uint32_t k = lo + gl; k < hi; k += G * FOLD_BATCH) {
        uint2 e[FOLD_BATCH];
#pragma unroll
        for (int u = 0; u < FOLD_BATCH; u++) e[u] = k + u * G < hi ? m.ent[k + u * G] : make_uint2(0u, 0u);
        F29<P> c[FOLD_BATCH];
        Fe<P> zz[FOLD_BATCH];
#pragma unroll
        for (int u = 0; u < FOLD_BATCH; u++) {
            c[u] = r1cs_coeff<P, LDS>(dict, e[u].y);
            zz[u] = z[e[u].x];
        }
#pragma unroll
        for (int u = 0; u < FOLD_BATCH; u++)
            if (k + u * G < hi) row_mac<P>(acc, c[u], f29_from_mont256<P>(zz[u]), one29);
    }
    F29<P> part = dot29_finish<P>(acc.acc);  // tight
    if (G == 1) return part;
    if (!ANY_LEN || hi - lo <= 256) {
        int steps = 0;
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
#pragma unroll
            for (int i = 0; i < 9; i++) part.l[i] += __shfl_down(part.l[i], off);
            if (++steps == 2 || off == 1) {  // 4 x 2^29 < 2^32
                part = f29_carry<P>(part);
                steps = 0;
            }
        }
        return part;
    }
    RowAcc<P> tot;
    row_init<P>(tot);
    const int leader = (threadIdx.x & 63) & ~(G - 1);
#pragma unroll 1
    for (int g = 0; g < G; g++) {
        F29<P> v;
#pragma unroll
        for (int i = 0; i < 9; i++) v.l[i] = __shfl(part.l[i], leader + g);
        row_mac<P>(tot, v, r1cs_coeff<P, LDS>(one29, 0), one29);
    }
    return dot29_finish<P>(tot.acc);
}

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
// 256-lane blocks for n rows of `group` lanes each, rounded to the XCD count so that fold_row_block is a bijection (0 for no row)
static unsigned class_blocks(size_t n, int group) {
    if (!n) return 0;
    const unsigned nb = div_up(n * group, FOLD_BLOCK);
    return (nb + FOLD_XCDS - 1) / FOLD_XCDS * FOLD_XCDS;
}

// the bounds of row's three combinations; true: the row is a long one of fold.hip
__device__ __forceinline__ bool fold_is_long(const R1csDev& s, size_t row, uint32_t* lo, uint32_t* hi) {
    lo[0] = s.a.rowptr[row]; hi[0] = s.a.rowptr[row + 1];
    lo[1] = s.b.rowptr[row]; hi[1] = s.b.rowptr[row + 1];
    lo[2] = s.c.rowptr[row]; hi[2] = s.c.rowptr[row + 1];
    return hi[0] - lo[0] > FOLD_LONG || hi[1] - lo[1] > FOLD_LONG || hi[2] - lo[2] > FOLD_LONG;
}

// Lane tid of 256-lane block `block` of a list of n >= 1 rows walked G lanes per row: the row, this lane's place gl in its group, and
// whether the group has a row of its own.  A group without a row shadows the last one (the shuffles of r1cs_row need every lane) and
// keeps nothing; with G = 1 such a lane has nothing to do and its row is not read.
struct RowSlot {
    uint32_t row, gl;
    bool live;
};
template <int G>
__device__ __forceinline__ RowSlot row_slot(const uint32_t* list, uint32_t n, size_t block, uint32_t tid) {
    const size_t slot = (block * FOLD_BLOCK + tid) / G;
    RowSlot t;
    t.live = slot < n;
    t.gl = tid & (G - 1);
    t.row = G > 1 || t.live ? list[t.live ? slot : n - 1] : 0;
    return t;
}

// The classes as one launch sees them: virtual 256-lane blocks [wide | mid | lane], each range a multiple of FOLD_XCDS (0 for an empty
// class) so that fold_row_block keeps a frame's rows on one L2.
struct RowClassDev {
    const uint32_t* rows;
    uint32_t n_wide, n_mid, n_lane;
    unsigned wide_blocks, mid_blocks, lane_blocks;
};
// Virtual block j of the concatenated classes: body(G, ANY_LEN, list, n, vb, nb) - lanes per row and whether a row may exceed 256
// entries (as std::integral_constant), the class list and its length, the block's index among the nb of its class.
template <int GM, class Body>
__device__ __forceinline__ void row_class_vblock(const RowClassDev& c, unsigned j, Body&& body) {
    using std::integral_constant;
    if (j < c.wide_blocks) body(integral_constant<int, SAT_WIDE_GROUP>(), integral_constant<bool, true>(), c.rows, c.n_wide, j, c.wide_blocks);
    else if (j < c.wide_blocks + c.mid_blocks) body(integral_constant<int, GM>(), integral_constant<bool, false>(), c.rows + c.n_wide, c.n_mid, j - c.wide_blocks, c.mid_blocks);
    else body(integral_constant<int, 1>(), integral_constant<bool, false>(), c.rows + c.n_wide + c.n_mid, c.n_lane, j - c.wide_blocks - c.mid_blocks, c.lane_blocks);
}

static RowClassDev class_view(const RowClasses& c, int mid_group) {
    RowClassDev d;
    d.rows = c.rows.as<uint32_t>();
    d.n_wide = (uint32_t)c.n_wide;
    d.n_mid = (uint32_t)c.n_mid;
    d.n_lane = (uint32_t)c.n_lane;
    d.wide_blocks = class_blocks(c.n_wide, SAT_WIDE_GROUP);
    d.mid_blocks = class_blocks(c.n_mid, mid_group);
    d.lane_blocks = class_blocks(c.n_lane, 1);
    return d;
}

// classes the rows of a resident shape (reads the three rowptr back; the caller holds the lock of the plan that owns `out`)
static void build_row_classes(RowClasses& out, const R1csShape& sh, uint32_t lane_max, uint32_t mid_max, bool skip_empty_rows) {
    const size_t rows = sh.num_cons;
    std::vector<uint32_t> rp[3];
    for (int w = 0; w < 3; w++) {
        rp[w].resize(rows + 1);
        LURK_HIP_CHECK(hipMemcpy(rp[w].data(), sh.m[w].rowptr.p, (rows + 1) * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint32_t> cls[3];  // wide, mid, lane
    for (size_t i = 0; i < rows; i++) {
        uint32_t len = 0;
        for (int w = 0; w < 3; w++) len = std::max(len, rp[w][i + 1] - rp[w][i]);
        if (!len && skip_empty_rows) continue;
        cls[len <= lane_max ? 2 : len <= mid_max ? 1 : 0].push_back((uint32_t)i);
    }
    out.n_wide = cls[0].size();
    out.n_mid = cls[1].size();
    out.n_lane = cls[2].size();
    out.lane_max = lane_max;
    out.mid_max = mid_max;
    cls[0].insert(cls[0].end(), cls[1].begin(), cls[1].end());
    cls[0].insert(cls[0].end(), cls[2].begin(), cls[2].end());
    out.rows.alloc(cls[0].size() * 4);
    if (!cls[0].empty()) LURK_HIP_CHECK(hipMemcpy(out.rows.p, cls[0].data(), cls[0].size() * 4, hipMemcpyHostToDevice));
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

