// hyperkzg.hip - the HyperKZG opening argument over BN254 G1 with the vectors resident in HBM, and the three polynomial primitives it
// is made of (adjacent-pair fold, univariate evaluation at a few points, division by linear factors) over fields 0, 1 and 2.
//
// Reference: lurk-beta's default engine is Bn256EngineKZG (/root/reference/src/proof/nova.rs:65-71), whose EE1 is
// nova::provider::hyperkzg::EvaluationEngine (arecibo, un-vendored: /root/reference/Cargo.toml:128).  The protocol below is this
// repository's own statement of the published scheme, recalled [MEM] - NOT byte-compatible with arecibo - restated in Python integers in
// tests/hyperkzg_ref.py.  With ck[i] = [tau^i]G resident (lurk_hip_msm_ctx_*), n = 2^ell evaluations P_0 of a multilinear polynomial and
// the point x (x_0 <-> the most significant index bit, as lurk_hip_eq_evals_dev):
//     P_{i+1}[j] = P_i[2j] + x_{ell-1-i} (P_i[2j+1] - P_i[2j])            i = 0 .. ell-2        hk_fold_pairs_kernel
//     com_i = commit(P_i), i = 1 .. ell-1;  y = the same fold of P_{ell-1} with x_0            the key's async slots
//     r = challenge(0, com);  u = (r, -r, r^2);  v[t][i] = P_i(u_t)                            hk_eval_kernel (two launches)
//     q = challenge(1, v);  B = sum_i q^i P_i (zero-padded)                                    hk_batch_kernel
//     h_t = (B - B(u_t)) / (X - u_t);  W_t = commit(h_t)                                       hk_div_* (three passes), three slots
// Every kernel streams through HBM once or twice; the commitments dominate (an opening commits ~ n + 3 n scalars).
// The verifier up to the pairing (lurk_hip_hyperkzg_pairing_inputs) is host code: the pairing itself stays with the caller.
#include <memory>
#include <vector>

#include "common.hpp"
#include "curve.cuh"
#include "dispatch.hpp"

namespace lurk {

constexpr int HK_BLOCK = 256;
constexpr int HK_MAX_POINTS = 4;
constexpr int HK_MAX_ROOTS = 3;
constexpr int HK_MAX_POLYS = 32;
constexpr int HK_EVAL_SEG = 4096;    // least coefficients per workgroup of the evaluation (16 per lane: the lane's power of u is paid once)
constexpr int HK_EVAL_MAX_SEGS = 256;  // most workgroups per polynomial (the last workgroup adds their partial sums lane by lane)
constexpr int HK_DIV_E = 4;          // coefficients per lane of the division's local pass
constexpr int HK_DIV_TILE = HK_BLOCK * HK_DIV_E;  // ... and per workgroup
constexpr int HK_BATCH_DEFAULT = 1;  // LURK_HYPERKZG_BATCH when the environment does not say: measured, DESIGN.md section 3.7.2

// a^e by square-and-multiply from the top set bit (e = 0 -> 1)
template <class F>
LURK_HD Fe<F> hk_pow(const Fe<F>& a, uint64_t e) {
    Fe<F> r = fe_one<F>();
    int top = 63;
    while (top >= 0 && !((e >> top) & 1u)) top--;
    for (int b = top; b >= 0; b--) {
        r = fe_mul<F>(r, r);
        if ((e >> b) & 1u) r = fe_mul<F>(r, a);
    }
    return r;
}

// ---- adjacent-pair fold: out[j] = in[2j] + x (in[2j+1] - in[2j]), j < ceil(len / 2); an element past the end reads as zero ----------
// (NOT fold_halves, which pairs i with len/2 + i.)  A lane reads 64 contiguous bytes and writes 32; out may not alias in.
template <class F>
__global__ __launch_bounds__(HK_BLOCK) void hk_fold_pairs_kernel(const Fe<F>* __restrict__ in, size_t len, Fe<F> x, Fe<F>* __restrict__ out) {
    const size_t half = (len + 1) / 2;
    for (size_t j = (size_t)blockIdx.x * HK_BLOCK + threadIdx.x; j < half; j += (size_t)gridDim.x * HK_BLOCK) {
        const Fe<F> lo = in[2 * j];
        const Fe<F> hi = 2 * j + 1 < len ? in[2 * j + 1] : fe_zero<F>();
        out[j] = fe_add<F>(lo, fe_mul<F>(x, fe_sub<F>(hi, lo)));
    }
}

// ---- univariate evaluation of several polynomials of one buffer at NP <= 4 points, one pass --------------------------------------------
// Polynomial p occupies buf[off[p] .. off[p] + len[p]) (coefficients low to high) and is cut into workgroup segments of seg[p]
// coefficients (a multiple of HK_BLOCK); workgroups blk0[p] .. blk0[p+1] - 1 take its segments.  Lane t of a segment that starts at s0
// runs Horner in u^256 over the coefficients s0 + t + 256 k (consecutive lanes read consecutive elements), scales by u^(s0 + t), and
// the workgroup adds its 256 lanes through LDS.  The last workgroup to take a ticket (the pattern of sumcheck.hip: release before,
// acquire after) adds the workgroups' partial sums of every polynomial: out[p * NP + j] = P_p(u_j).
struct HkEvalPlan {
    uint64_t off[HK_MAX_POLYS], len[HK_MAX_POLYS];
    uint32_t blk0[HK_MAX_POLYS + 1], seg[HK_MAX_POLYS];
    int npolys;
};
template <class F>
struct HkPoints {
    Fe<F> u[HK_MAX_POINTS], u256[HK_MAX_POINTS];
};

template <class F, int NP>
__global__ __launch_bounds__(HK_BLOCK) void hk_eval_kernel(const Fe<F>* __restrict__ buf, HkEvalPlan pl, HkPoints<F> pts, Fe<F>* partial, uint32_t* counter,
                                                            Fe<F>* out) {
    __shared__ uint4 raw[HK_BLOCK * NP * 2];
    __shared__ uint32_t sh_ticket;
    Fe<F>* sh = reinterpret_cast<Fe<F>*>(raw);
    const int t = threadIdx.x;
    int p = 0;
    while (p + 1 < pl.npolys && blockIdx.x >= pl.blk0[p + 1]) p++;
    const size_t s0 = (size_t)(blockIdx.x - pl.blk0[p]) * pl.seg[p];
    const size_t s1 = s0 + pl.seg[p] < pl.len[p] ? s0 + pl.seg[p] : pl.len[p];
    const Fe<F>* c = buf + pl.off[p];
    Fe<F> acc[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) acc[j] = fe_zero<F>();
    if (s0 + t < s1) {
        const size_t first = s0 + t;
        for (size_t k = (s1 - first - 1) / HK_BLOCK + 1; k-- > 0;) {
            const Fe<F> cv = c[first + k * HK_BLOCK];
#pragma unroll
            for (int j = 0; j < NP; j++) acc[j] = fe_add<F>(fe_mul<F>(acc[j], pts.u256[j]), cv);
        }
#pragma unroll
        for (int j = 0; j < NP; j++) acc[j] = fe_mul<F>(acc[j], hk_pow<F>(pts.u[j], first));
    }
#pragma unroll
    for (int j = 0; j < NP; j++) sh[j * HK_BLOCK + t] = acc[j];
    __syncthreads();
    for (int s = HK_BLOCK / 2; s >= 1; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int j = 0; j < NP; j++) sh[j * HK_BLOCK + t] = fe_add<F>(sh[j * HK_BLOCK + t], sh[j * HK_BLOCK + t + s]);
        }
        __syncthreads();
    }
    if (t == 0) {
#pragma unroll
        for (int j = 0; j < NP; j++) partial[(size_t)blockIdx.x * NP + j] = sh[j * HK_BLOCK];
        __threadfence();  // the partial sums are visible device-wide before the ticket is taken
        sh_ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (sh_ticket != gridDim.x - 1) return;
    __threadfence();
    if (t < pl.npolys * NP) {  // <= 32 x 4 lanes, one (polynomial, point) each
        const int pp = t / NP, j = t % NP;
        Fe<F> sum = fe_zero<F>();
        for (uint32_t b = pl.blk0[pp]; b < pl.blk0[pp + 1]; b++) sum = fe_add<F>(sum, partial[(size_t)b * NP + j]);
        out[t] = sum;
    }
    if (t == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
}

// ---- the batch polynomial: B[j] = sum_{i : j < n >> i} q^i P_i[j], one pass ------------------------------------------------------------
// P_0 is the caller's buffer, P_i (i >= 1) sits at rest[n - 2 (n >> i)] with n >> i elements; Horner in q from the shortest polynomial
// that still covers j down to P_0 (about two terms per element on average: 2 n elements are read in all).
template <class F>
__global__ __launch_bounds__(HK_BLOCK) void hk_batch_kernel(const Fe<F>* __restrict__ p0, const Fe<F>* __restrict__ rest, size_t n, int ell, Fe<F> q,
                                                             Fe<F>* __restrict__ out) {
    for (size_t j = (size_t)blockIdx.x * HK_BLOCK + threadIdx.x; j < n; j += (size_t)gridDim.x * HK_BLOCK) {
        int i = 0;
        while (i + 1 < ell && (n >> (i + 1)) > j) i++;
        Fe<F> acc = i == 0 ? p0[j] : rest[n - 2 * (n >> i) + j];
        for (i--; i >= 0; i--) acc = fe_add<F>(fe_mul<F>(acc, q), i == 0 ? p0[j] : rest[n - 2 * (n >> i) + j]);
        out[j] = acc;
    }
}

// ---- division by (X - u) for NR <= 3 roots in one pass over the coefficients -----------------------------------------------------------
// b(X) = h(X) (X - u) + b(u) with h_{j-1} = b_j + u h_j, h_{len-1} = 0: a suffix Horner recurrence, h_j = sum_{k > j} b_k u^(k-j-1).
// Blocked scan, no workgroup waits for another one inside a launch:
//   pass 1 (hk_div_local_kernel, one workgroup per tile of HK_DIV_TILE coefficients): the recurrence inside the tile with zero carry-in
//          (a lane's HK_DIV_E coefficients, a suffix scan of the lanes' values by powers of u^E through LDS, the lane's pass again with
//          its carry) -> the local quotient, and the tile's value V_c = sum_k b_{s+k} u^k;
//   pass 2 (hk_div_carry_kernel, one workgroup per root): the same scan over the tile values by powers of u^TILE -> the carry into
//          every tile H_c = h_{e-1} (e = the tile's end), and the remainder b(u) = the inclusive total;
//   pass 3 (hk_div_fix_kernel): h_j += u^(e-1-j) H_c, consecutive lanes on consecutive elements.
template <class F>
struct HkRoots {
    Fe<F> u[HK_MAX_ROOTS], u_e[HK_MAX_ROOTS], u256[HK_MAX_ROOTS], u_tile[HK_MAX_ROOTS], u_tile_g[HK_MAX_ROOTS];
};
template <class F>
struct HkQuot {
    Fe<F>* q[HK_MAX_ROOTS];
};

// inclusive suffix scan over the workgroup's lanes: returns X_t = sum_{t' >= t} a_{t'} w^(t' - t); sh: HK_BLOCK elements of LDS
template <class F>
__device__ __forceinline__ Fe<F> hk_suffix_scan(Fe<F>* sh, Fe<F> a, Fe<F> w) {
    const int t = threadIdx.x;
    sh[t] = a;
    __syncthreads();
    Fe<F> pw = w;
    for (int s = 1; s < HK_BLOCK; s <<= 1) {
        Fe<F> v = sh[t];
        if (t + s < HK_BLOCK) v = fe_add<F>(v, fe_mul<F>(pw, sh[t + s]));
        __syncthreads();
        sh[t] = v;
        __syncthreads();
        pw = fe_mul<F>(pw, pw);
    }
    return sh[t];
}

template <class F, int NR>
__global__ __launch_bounds__(HK_BLOCK) void hk_div_local_kernel(const Fe<F>* __restrict__ b, size_t len, HkRoots<F> ro, HkQuot<F> quo, Fe<F>* __restrict__ tile_val) {
    __shared__ uint4 raw[HK_BLOCK * 2];
    Fe<F>* sh = reinterpret_cast<Fe<F>*>(raw);
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * HK_DIV_TILE + (size_t)t * HK_DIV_E;
    Fe<F> c[HK_DIV_E];
#pragma unroll
    for (int k = 0; k < HK_DIV_E; k++) c[k] = base + k < len ? b[base + k] : fe_zero<F>();
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const Fe<F> u = ro.u[r];
        Fe<F> acc = fe_zero<F>();
#pragma unroll
        for (int k = HK_DIV_E - 1; k >= 0; k--) acc = fe_add<F>(c[k], fe_mul<F>(u, acc));
        hk_suffix_scan<F>(sh, acc, ro.u_e[r]);
        acc = t + 1 < HK_BLOCK ? sh[t + 1] : fe_zero<F>();  // the carry into this lane's chunk
        if (t == 0) tile_val[(size_t)r * gridDim.x + blockIdx.x] = sh[0];
        __syncthreads();  // (the next root's scan writes sh)
        Fe<F>* out = quo.q[r];
#pragma unroll
        for (int k = HK_DIV_E - 1; k >= 0; k--) {
            if (base + k + 1 < len) out[base + k] = acc;  // the quotient has len - 1 coefficients
            acc = fe_add<F>(c[k], fe_mul<F>(u, acc));
        }
    }
}

// one workgroup per root; nt tile values in, nt carries and the remainder out.  A lane takes g = ceil(nt / HK_BLOCK) consecutive tiles.
template <class F>
__global__ __launch_bounds__(HK_BLOCK) void hk_div_carry_kernel(const Fe<F>* __restrict__ tile_val, uint32_t nt, uint32_t g, HkRoots<F> ro, Fe<F>* __restrict__ carry,
                                                                 Fe<F>* __restrict__ rem) {
    __shared__ uint4 raw[HK_BLOCK * 2];
    Fe<F>* sh = reinterpret_cast<Fe<F>*>(raw);
    const int t = threadIdx.x, r = blockIdx.x;
    const Fe<F>* v = tile_val + (size_t)r * nt;
    const Fe<F> w = ro.u_tile[r];
    Fe<F> acc = fe_zero<F>();
    for (uint32_t k = g; k-- > 0;) {
        const uint32_t c = (uint32_t)t * g + k;
        if (c < nt) acc = fe_add<F>(v[c], fe_mul<F>(w, acc));
    }
    hk_suffix_scan<F>(sh, acc, ro.u_tile_g[r]);
    acc = t + 1 < HK_BLOCK ? sh[t + 1] : fe_zero<F>();
    if (t == 0) rem[r] = sh[0];
    for (uint32_t k = g; k-- > 0;) {
        const uint32_t c = (uint32_t)t * g + k;
        if (c < nt) {
            carry[(size_t)r * nt + c] = acc;
            acc = fe_add<F>(v[c], fe_mul<F>(w, acc));
        }
    }
}

template <class F, int NR>
__global__ __launch_bounds__(HK_BLOCK) void hk_div_fix_kernel(size_t len, HkRoots<F> ro, const Fe<F>* __restrict__ carry, HkQuot<F> quo) {
    const int t = threadIdx.x;
    const size_t s = (size_t)blockIdx.x * HK_DIV_TILE;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const Fe<F> h = carry[(size_t)r * gridDim.x + blockIdx.x];
        if (fe_is_zero<F>(h)) continue;  // (uniform over the workgroup; always so for the last tile)
        Fe<F> gk = fe_mul<F>(h, hk_pow<F>(ro.u[r], (uint64_t)(HK_BLOCK - 1 - t)));  // u^(TILE - 1 - j) H for j = t + 256 (E - 1)
        Fe<F>* out = quo.q[r];
#pragma unroll
        for (int k = HK_DIV_E - 1; k >= 0; k--) {
            const size_t j = s + (size_t)k * HK_BLOCK + t;
            if (j + 1 < len) out[j] = fe_add<F>(out[j], gk);
            gk = fe_mul<F>(gk, ro.u256[r]);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static unsigned hk_grid(size_t work) {
    unsigned blocks = work ? div_up(work, HK_BLOCK) : 1, cap = grid_cap(16);
    return blocks > cap ? cap : blocks;
}

template <class F>
static void hk_fold_pairs(const void* d_in, size_t len, const Fe<F>& x, void* d_out, hipStream_t s) {
    ProfScope ps("hkzg_fold", s);
    hipLaunchKernelGGL((hk_fold_pairs_kernel<F>), dim3(hk_grid((len + 1) / 2)), dim3(HK_BLOCK), 0, s, (const Fe<F>*)d_in, len, x, (Fe<F>*)d_out);
    LURK_HIP_CHECK(hipGetLastError());
}

// npolys polynomials of one device buffer (element offsets / lengths) at np points; d_out: npolys x np Montgomery values on the device
// (polynomial-major).  Stream-ordered, no synchronisation; scratch from the stream's arena is held by the caller (d_partial, d_counter).
struct HkEvalScratch {
    ArenaBuf buf;
    Fe<Bn254Fr>* partial;  // (reinterpreted per field: 32-byte elements)
    uint32_t* counter;
    explicit HkEvalScratch(hipStream_t s) : buf((size_t)HK_MAX_POLYS * HK_EVAL_MAX_SEGS * HK_MAX_POINTS * 32 + 256, s) {
        counter = (uint32_t*)buf.p;  // the polled word leads its block (16-byte block, zeroed per launch)
        partial = (Fe<Bn254Fr>*)((char*)buf.p + 256);
    }
};
template <class F>
static void hk_eval(const void* d_buf, int npolys, const size_t* off, const size_t* len, const Fe<F>* points, int np, void* d_out, HkEvalScratch& sc, hipStream_t s) {
    LURK_REQUIRE(npolys >= 1 && npolys <= HK_MAX_POLYS && np >= 1 && np <= HK_MAX_POINTS, "evaluation: polynomial or point count out of range");
    HkEvalPlan pl;
    memset(&pl, 0, sizeof(pl));
    pl.npolys = npolys;
    uint32_t blocks = 0;
    for (int p = 0; p < npolys; p++) {
        size_t seg = HK_EVAL_SEG;
        const size_t per = (len[p] + HK_EVAL_MAX_SEGS - 1) / HK_EVAL_MAX_SEGS;
        if (per > seg) seg = (per + HK_BLOCK - 1) / HK_BLOCK * HK_BLOCK;
        LURK_REQUIRE(seg < ((size_t)1 << 32), "evaluation: polynomial too long");
        pl.off[p] = off[p];
        pl.len[p] = len[p];
        pl.seg[p] = (uint32_t)seg;
        pl.blk0[p] = blocks;
        blocks += len[p] ? (uint32_t)((len[p] + seg - 1) / seg) : 1;  // (an empty polynomial keeps one workgroup: its sum is zero)
    }
    pl.blk0[npolys] = blocks;
    HkPoints<F> pts;
    for (int j = 0; j < HK_MAX_POINTS; j++) {
        pts.u[j] = j < np ? points[j] : fe_zero<F>();
        pts.u256[j] = hk_pow<F>(pts.u[j], HK_BLOCK);
    }
    LURK_HIP_CHECK(hipMemsetAsync(sc.counter, 0, 16, s));
    Fe<F>* partial = (Fe<F>*)sc.partial;
    ProfScope ps("hkzg_eval", s);
    const Fe<F>* b = (const Fe<F>*)d_buf;
    Fe<F>* o = (Fe<F>*)d_out;
    if (np == 1) hipLaunchKernelGGL((hk_eval_kernel<F, 1>), dim3(blocks), dim3(HK_BLOCK), 0, s, b, pl, pts, partial, sc.counter, o);
    else if (np == 2) hipLaunchKernelGGL((hk_eval_kernel<F, 2>), dim3(blocks), dim3(HK_BLOCK), 0, s, b, pl, pts, partial, sc.counter, o);
    else if (np == 3) hipLaunchKernelGGL((hk_eval_kernel<F, 3>), dim3(blocks), dim3(HK_BLOCK), 0, s, b, pl, pts, partial, sc.counter, o);
    else hipLaunchKernelGGL((hk_eval_kernel<F, 4>), dim3(blocks), dim3(HK_BLOCK), 0, s, b, pl, pts, partial, sc.counter, o);
    LURK_HIP_CHECK(hipGetLastError());
}

// d_quot[r]: len - 1 elements each (may be NULL when len == 1); d_rem: nr Montgomery remainders on the device.  Stream-ordered.
template <class F>
static void hk_div_linear(const void* d_b, size_t len, const Fe<F>* roots, int nr, void* const* d_quot, void* d_rem, hipStream_t s) {
    LURK_REQUIRE(nr >= 1 && nr <= HK_MAX_ROOTS && len >= 1, "division: 1 to 3 roots and at least one coefficient");
    const size_t nt = (len + HK_DIV_TILE - 1) / HK_DIV_TILE;
    LURK_REQUIRE(nt < ((size_t)1 << 31), "division: polynomial too long");
    const uint32_t g = (uint32_t)((nt + HK_BLOCK - 1) / HK_BLOCK);
    HkRoots<F> ro;
    HkQuot<F> quo;
    for (int r = 0; r < HK_MAX_ROOTS; r++) {
        ro.u[r] = r < nr ? roots[r] : fe_zero<F>();
        ro.u_e[r] = hk_pow<F>(ro.u[r], HK_DIV_E);
        ro.u256[r] = hk_pow<F>(ro.u[r], HK_BLOCK);
        ro.u_tile[r] = hk_pow<F>(ro.u[r], HK_DIV_TILE);
        ro.u_tile_g[r] = hk_pow<F>(ro.u_tile[r], g);
        quo.q[r] = r < nr ? (Fe<F>*)d_quot[r] : nullptr;
    }
    ArenaBuf vals((size_t)nr * nt * 32, s), carry((size_t)nr * nt * 32, s);
    ProfScope ps("hkzg_div", s);
    const Fe<F>* b = (const Fe<F>*)d_b;
    Fe<F>*tv = (Fe<F>*)vals.p, *cy = (Fe<F>*)carry.p;
    const dim3 grid((unsigned)nt), block(HK_BLOCK);
    if (nr == 1) hipLaunchKernelGGL((hk_div_local_kernel<F, 1>), grid, block, 0, s, b, len, ro, quo, tv);
    else if (nr == 2) hipLaunchKernelGGL((hk_div_local_kernel<F, 2>), grid, block, 0, s, b, len, ro, quo, tv);
    else hipLaunchKernelGGL((hk_div_local_kernel<F, 3>), grid, block, 0, s, b, len, ro, quo, tv);
    hipLaunchKernelGGL((hk_div_carry_kernel<F>), dim3(nr), block, 0, s, (const Fe<F>*)tv, (uint32_t)nt, g, ro, cy, (Fe<F>*)d_rem);
    if (nt > 1) {
        if (nr == 1) hipLaunchKernelGGL((hk_div_fix_kernel<F, 1>), grid, block, 0, s, len, ro, (const Fe<F>*)cy, quo);
        else if (nr == 2) hipLaunchKernelGGL((hk_div_fix_kernel<F, 2>), grid, block, 0, s, len, ro, (const Fe<F>*)cy, quo);
        else hipLaunchKernelGGL((hk_div_fix_kernel<F, 3>), grid, block, 0, s, len, ro, (const Fe<F>*)cy, quo);
    }
    LURK_HIP_CHECK(hipGetLastError());
}

// LURK_HYPERKZG_BATCH (1 / 0): the short commitments of stage 0 as one batch, or every one a submit of its own.  Read at EACH call, so
// that one process can prove both ways.  The default is what the measurement of DESIGN.md section 3.7.2 decided.
static bool hk_batch_enabled() {
    const char* v = getenv("LURK_HYPERKZG_BATCH");
    return v ? atoi(v) != 0 : HK_BATCH_DEFAULT != 0;
}
// LURK_HYPERKZG_BATCH_MAX_LEN: the longest polynomial that goes with the batch, at most (and by default) LURK_MSM_BATCH_MAX_LEN.  An
// internal knob, read at each call: with it a 2^10 opening has some commitments of their own and some batched, as a 2^20 one does.
static size_t hk_batch_max_len() {
    const char* v = getenv("LURK_HYPERKZG_BATCH_MAX_LEN");
    const long long x = v ? atoll(v) : 0;
    return x > 0 && (size_t)x < LURK_MSM_BATCH_MAX_LEN ? (size_t)x : LURK_MSM_BATCH_MAX_LEN;
}

// ---- the prover ------------------------------------------------------------------------------------------------------------------------
// Commitments stay in flight through the key's async slots: com_{i+1} is submitted behind fold i and accumulates while fold i + 1 (and
// the ones after it) run on the caller's stream; a slot is waited for only when the loop comes round to it again.  The three W_t take
// slots 0..2.  Whatever fails, every slot that was submitted is drained before the call returns: the key stays usable.
template <class F>
static void hyperkzg_prove(lurk_hip_msm_ctx* key, const void* d_poly, size_t n, int ell, const void* x32_mont, lurk_hip_hyperkzg_challenge_fn challenge, void* user,
                           uint64_t* out_com, uint64_t* out_v, uint64_t* out_w, void* out_y, hipStream_t s) {
    std::vector<Fe<F>> x(ell);
    memcpy((void*)x.data(), x32_mont, (size_t)ell * 32);
    stream_pool_retain();
    ArenaBuf rest(n * 32, s), bpoly(n * 32, s), quot((size_t)3 * n * 32, s), small((size_t)(HK_MAX_POLYS * 3 + 8) * 32, s);
    HkEvalScratch esc(s);
    Fe<F>* d_rest = (Fe<F>*)rest.p;
    struct Drain {
        lurk_hip_msm_ctx* key;
        long pending[LURK_MSM_SLOTS];
        int batch_slot;  // >= 0: a batch is pending on this slot
        ~Drain() {
            uint64_t sink[12];
            for (int k = 0; k < LURK_MSM_SLOTS; k++)
                if (pending[k] >= 0) (void)lurk_hip_msm_ctx_wait(key, k, sink);
            if (batch_slot >= 0) {
                std::vector<uint64_t> many((size_t)12 * LURK_MSM_BATCH_MAX_VECTORS);
                (void)lurk_hip_msm_ctx_wait_batch(key, batch_slot, many.data());
            }
        }
    } drain{key, {}, -1};
    for (int k = 0; k < LURK_MSM_SLOTS; k++) drain.pending[k] = -1;
    // The short polynomials P_{first_short} .. P_{ell-1} (at most hk_batch_max_len() scalars each) leave as ONE batch behind the last fold
    // (lurk_hip_msm_ctx_submit_batch_dev: msm_batch.hip) on the last slot; the longer ones keep their per-slot submits on the others.  Off
    // (LURK_HYPERKZG_BATCH=0), under a key that is not in the window-table form, or with fewer than two short polynomials: every
    // commitment a submit of its own, over all slots.  The proof's bytes are the same either way.
    int first_short = ell;  // P_i, i >= first_short, are batched
    if (hk_batch_enabled() && msm_ctx_table_view(key).form == LURK_MSM_FORM_TABLE) {
        const size_t cap = hk_batch_max_len();
        int i = 1;
        while (i < ell && (n >> i) > cap) i++;
        if (ell - i >= 2 && ell - i <= LURK_MSM_BATCH_MAX_VECTORS) first_short = i;
    }
    const bool batched = first_short < ell;
    const int nslots = batched ? LURK_MSM_SLOTS - 1 : LURK_MSM_SLOTS, batch_slot = LURK_MSM_SLOTS - 1;
    // folds and commitments
    const Fe<F>* cur = (const Fe<F>*)d_poly;
    size_t len = n;
    for (int i = 0; i + 1 < ell; i++) {
        Fe<F>* nxt = d_rest + (n - 2 * (n >> (i + 1)));
        hk_fold_pairs<F>(cur, len, x[ell - 1 - i], nxt, s);
        len /= 2;
        cur = nxt;
        if (i + 1 >= first_short) continue;  // P_{i+1} goes with the batch
        const int slot = i % nslots;
        if (drain.pending[slot] >= 0) {
            const long which = drain.pending[slot];
            drain.pending[slot] = -1;
            nested_ok(lurk_hip_msm_ctx_wait(key, slot, out_com + 12 * which));
        }
        nested_ok(lurk_hip_msm_ctx_submit_dev(key, slot, nxt, len, 1, (void*)s));
        drain.pending[slot] = i;
    }
    if (batched) {
        size_t off[LURK_MSM_BATCH_MAX_VECTORS], ln[LURK_MSM_BATCH_MAX_VECTORS];
        for (int i = first_short; i < ell; i++) {
            off[i - first_short] = n - 2 * (n >> i);
            ln[i - first_short] = n >> i;
        }
        nested_ok(lurk_hip_msm_ctx_submit_batch_dev(key, batch_slot, d_rest, off, ln, (size_t)(ell - first_short), 1, (void*)s));
        drain.batch_slot = batch_slot;
    }
    Fe<F> tail[2];
    LURK_HIP_CHECK(hipMemcpyAsync(tail, cur, 64, hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    const Fe<F> y = fe_add<F>(tail[0], fe_mul<F>(x[0], fe_sub<F>(tail[1], tail[0])));
    fe_write_canonical<F>(out_y, y);
    for (int k = 0; k < LURK_MSM_SLOTS; k++) {
        if (drain.pending[k] < 0) continue;
        const long which = drain.pending[k];
        drain.pending[k] = -1;
        nested_ok(lurk_hip_msm_ctx_wait(key, k, out_com + 12 * which));
    }
    if (drain.batch_slot >= 0) {
        drain.batch_slot = -1;
        nested_ok(lurk_hip_msm_ctx_wait_batch(key, batch_slot, out_com + 12 * (size_t)(first_short - 1)));
    }
    // stage 0: r from the commitments
    uint64_t ch[4] = {0, 0, 0, 0};
    LURK_REQUIRE(challenge(user, 0, out_com, (size_t)(ell - 1), ch) == 0, "the transcript callback failed");
    const Fe<F> r = fe_read_canonical<F>(ch, "the challenge");
    LURK_REQUIRE(!fe_is_zero<F>(r), "zero challenge");
    const Fe<F> u[3] = {r, fe_neg<F>(r), fe_mul<F>(r, r)};
    // evaluations: P_0 alone, then P_1 .. P_{ell-1} out of the one buffer
    Fe<F>* d_v = (Fe<F>*)small.p;  // [polynomial][point]
    {
        const size_t off0 = 0, len0 = n;
        hk_eval<F>(d_poly, 1, &off0, &len0, u, 3, d_v, esc, s);
        if (ell > 1) {
            size_t off[HK_MAX_POLYS], ln[HK_MAX_POLYS];
            for (int i = 1; i < ell; i++) {
                off[i - 1] = n - 2 * (n >> i);
                ln[i - 1] = n >> i;
            }
            hk_eval<F>(d_rest, ell - 1, off, ln, u, 3, d_v + 3, esc, s);
        }
    }
    std::vector<Fe<F>> v((size_t)3 * ell);
    LURK_HIP_CHECK(hipMemcpyAsync((void*)v.data(), d_v, (size_t)3 * ell * 32, hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    for (int t = 0; t < 3; t++)
        for (int i = 0; i < ell; i++) fe_write_canonical<F>(out_v + 4 * ((size_t)t * ell + i), v[(size_t)i * 3 + t]);
    // stage 1: q from the evaluations
    ch[0] = ch[1] = ch[2] = ch[3] = 0;
    LURK_REQUIRE(challenge(user, 1, out_v, (size_t)3 * ell, ch) == 0, "the transcript callback failed");
    const Fe<F> q = fe_read_canonical<F>(ch, "the challenge");
    {
        ProfScope ps("hkzg_batch", s);
        hipLaunchKernelGGL((hk_batch_kernel<F>), dim3(hk_grid(n)), dim3(HK_BLOCK), 0, s, (const Fe<F>*)d_poly, (const Fe<F>*)d_rest, n, ell, q, (Fe<F>*)bpoly.p);
        LURK_HIP_CHECK(hipGetLastError());
    }
    void* d_q[3] = {quot.p, (char*)quot.p + n * 32, (char*)quot.p + 2 * n * 32};
    Fe<F>* d_rem = d_v + (size_t)3 * HK_MAX_POLYS;
    hk_div_linear<F>(bpoly.p, n, u, 3, d_q, d_rem, s);
    for (int t = 0; t < 3; t++) {
        nested_ok(lurk_hip_msm_ctx_submit_dev(key, t, d_q[t], n - 1, 1, (void*)s));
        drain.pending[t] = t;
    }
    Fe<F> rem[3];
    LURK_HIP_CHECK(hipMemcpyAsync(rem, d_rem, 96, hipMemcpyDeviceToHost, s));
    LURK_HIP_CHECK(hipStreamSynchronize(s));
    for (int t = 0; t < 3; t++) {  // B(u_t) must be sum_i q^i v[t][i]: anything else is a fault of the kernels above, never of the input
        Fe<F> want = fe_zero<F>();
        for (int i = ell - 1; i >= 0; i--) want = fe_add<F>(fe_mul<F>(want, q), v[(size_t)i * 3 + t]);
        if (!fe_eq<F>(want, rem[t])) throw HipFailure{LURK_HIP_ERR_HIP, "hyperkzg: the remainder of the batch polynomial differs from the combined evaluations"};
    }
    for (int t = 0; t < 3; t++) {
        drain.pending[t] = -1;
        nested_ok(lurk_hip_msm_ctx_wait(key, t, out_w + 12 * t));
    }
}

// ---- the verifier up to the pairing (host only) ------------------------------------------------------------------------------------------
// a 96-byte Jacobian of BN254 G1 (Montgomery): reduced coordinates, and the identity (z = 0) or y^2 = x^3 + 3 z^6
static bool hk_point_ok(const void* p96) {
    using P = Bn254Fq;
    Jacobian<P> j;
    memcpy(&j, p96, 96);
    if (fe_canonical_ge_mod<P>(j.x.l) || fe_canonical_ge_mod<P>(j.y.l) || fe_canonical_ge_mod<P>(j.z.l)) return false;
    if (fe_is_zero<P>(j.z)) return true;
    const Fe<P> z2 = fe_sqr<P>(j.z), z6 = fe_mul<P>(fe_sqr<P>(z2), z2);
    const Fe<P> rhs = fe_add<P>(fe_mul<P>(fe_sqr<P>(j.x), j.x), fe_mul<P>(fe_from_u64<P>(3), z6));
    return fe_eq<P>(fe_sqr<P>(j.y), rhs);
}

static void hyperkzg_pairing_inputs(int ell, const void* c96, const void* x32, const void* y32, const uint64_t* com, const uint64_t* v32, const uint64_t* w, const void* r32,
                                    const void* q32, const void* d32, void* out_l, void* out_r, int* accepted, int* failed) {
    using F = Bn254Fr;
    const int curve = LURK_CURVE_BN254;
    auto reject = [&](int code) {
        memset(out_l, 0, 96);
        memset(out_r, 0, 96);
        *accepted = 0;
        if (failed) *failed = code;
    };
    auto reduced = [](const void* p) {
        uint32_t l[8];
        memcpy(l, p, 32);
        return !fe_canonical_ge_mod<F>(l);
    };
    // malformed input is rejected before any arithmetic
    bool wf = reduced(y32) && reduced(r32) && reduced(q32) && reduced(d32) && hk_point_ok(c96);
    for (int i = 0; wf && i < ell; i++) wf = reduced((const char*)x32 + 32 * i);
    for (int i = 0; wf && i < 3 * ell; i++) wf = reduced(v32 + 4 * i);
    for (int i = 0; wf && i + 1 < ell; i++) wf = hk_point_ok(com + 12 * i);
    for (int t = 0; wf && t < 3; t++) wf = hk_point_ok(w + 12 * t);
    if (!wf) return reject(LURK_HYPERKZG_MALFORMED);
    const Fe<F> r = fe_read_canonical<F>(r32, "r"), q = fe_read_canonical<F>(q32, "q"), d = fe_read_canonical<F>(d32, "d"), y = fe_read_canonical<F>(y32, "y");
    if (fe_is_zero<F>(r)) return reject(LURK_HYPERKZG_MALFORMED);
    std::vector<Fe<F>> x(ell), v((size_t)3 * ell);
    for (int i = 0; i < ell; i++) x[i] = fe_read_canonical<F>((const char*)x32 + 32 * i, "x");
    for (int i = 0; i < 3 * ell; i++) v[i] = fe_read_canonical<F>(v32 + 4 * i, "v");
    const Fe<F> one = fe_one<F>(), two_r = fe_dbl<F>(r);
    // 2 r Y_{i+1} = r (1 - x_{ell-1-i}) (v[0][i] + v[1][i]) + x_{ell-1-i} (v[0][i] - v[1][i]),  Y_i = v[2][i], Y_ell = y
    for (int i = 0; i < ell; i++) {
        const Fe<F> xi = x[ell - 1 - i], v0 = v[i], v1 = v[(size_t)ell + i], ynext = i + 1 < ell ? v[(size_t)2 * ell + i + 1] : y;
        const Fe<F> lhs = fe_mul<F>(two_r, ynext);
        const Fe<F> rhs = fe_add<F>(fe_mul<F>(fe_mul<F>(r, fe_sub<F>(one, xi)), fe_add<F>(v0, v1)), fe_mul<F>(xi, fe_sub<F>(v0, v1)));
        if (!fe_eq<F>(lhs, rhs)) return reject(LURK_HYPERKZG_FOLD);
    }
    const Fe<F> u[3] = {r, fe_neg<F>(r), fe_mul<F>(r, r)};
    const Fe<F> dp[3] = {one, d, fe_mul<F>(d, d)};
    // Bcom = sum_i q^i com_i (com_0 = C); L = [1 + d + d^2] Bcom - [sum_t d^t b_t] G + sum_t [d^t u_t] W_t; R = sum_t [d^t] W_t
    std::vector<uint64_t> pts((size_t)12 * (ell > 5 ? ell : 5));
    Fe<F> qp = one;
    for (int i = 0; i < ell; i++) {
        uint64_t sc[4];
        fe_write_canonical<F>(sc, qp);
        nested_ok(lurk_hip_point_mul(curve, pts.data() + 12 * i, i == 0 ? c96 : (const void*)(com + 12 * (i - 1)), sc, 0));
        qp = fe_mul<F>(qp, q);
    }
    uint64_t bcom[12];
    nested_ok(lurk_hip_point_sum(curve, bcom, pts.data(), ell));
    Fe<F> bsum = fe_zero<F>();
    for (int t = 0; t < 3; t++) {
        Fe<F> bt = fe_zero<F>();
        for (int i = ell - 1; i >= 0; i--) bt = fe_add<F>(fe_mul<F>(bt, q), v[(size_t)t * ell + i]);
        bsum = fe_add<F>(bsum, fe_mul<F>(dp[t], bt));
    }
    Jacobian<Bn254Fq> g;
    g.x = fe_one<Bn254Fq>();
    g.y = fe_dbl<Bn254Fq>(fe_one<Bn254Fq>());
    g.z = fe_one<Bn254Fq>();
    uint64_t sc[4];
    fe_write_canonical<F>(sc, fe_add<F>(fe_add<F>(dp[0], dp[1]), dp[2]));
    nested_ok(lurk_hip_point_mul(curve, pts.data(), bcom, sc, 0));
    fe_write_canonical<F>(sc, fe_neg<F>(bsum));
    nested_ok(lurk_hip_point_mul(curve, pts.data() + 12, &g, sc, 0));
    for (int t = 0; t < 3; t++) {
        fe_write_canonical<F>(sc, fe_mul<F>(dp[t], u[t]));
        nested_ok(lurk_hip_point_mul(curve, pts.data() + 12 * (2 + t), w + 12 * t, sc, 0));
    }
    nested_ok(lurk_hip_point_sum(curve, out_l, pts.data(), 5));
    for (int t = 0; t < 3; t++) {
        fe_write_canonical<F>(sc, dp[t]);
        nested_ok(lurk_hip_point_mul(curve, pts.data() + 12 * t, w + 12 * t, sc, 0));
    }
    nested_ok(lurk_hip_point_sum(curve, out_r, pts.data(), 3));
    *accepted = 1;
    if (failed) *failed = LURK_HYPERKZG_ACCEPTED;
}

}  // namespace lurk

using namespace lurk;

extern "C" {

int lurk_hip_mle_fold_pairs_dev(int field_id, const void* d_in, size_t len, const void* x32_mont, void* d_out, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        LURK_REQUIRE(len >= 1, "length must be at least 1");
        LURK_REQUIRE(d_in && d_out && x32_mont, "null argument");
        const size_t half = (len + 1) / 2;
        LURK_REQUIRE((const char*)d_out + half * 32 <= (const char*)d_in || (const char*)d_in + len * 32 <= (const char*)d_out, "the output may not alias the input");
        with_field(field_id, [&](auto tag) {
            using F = decltype(tag);
            Fe<F> x;
            memcpy(x.l, x32_mont, 32);
            hk_fold_pairs<F>(d_in, len, x, d_out, (hipStream_t)stream);
        });
    });
}

int lurk_hip_poly_eval_dev(int field_id, const void* d_coeffs, size_t len, const void* points32_mont, int n_points, void* out32_mont, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        LURK_REQUIRE(n_points >= 1 && n_points <= HK_MAX_POINTS, "1 to 4 evaluation points");
        LURK_REQUIRE(points32_mont && out32_mont && (len == 0 || d_coeffs), "null argument");
        hipStream_t s = (hipStream_t)stream;
        with_field(field_id, [&](auto tag) {
            using F = decltype(tag);
            Fe<F> pts[HK_MAX_POINTS];
            memcpy((void*)pts, points32_mont, (size_t)n_points * 32);
            ArenaBuf d_out(HK_MAX_POINTS * 32, s);
            HkEvalScratch sc(s);
            const size_t off = 0;
            hk_eval<F>(d_coeffs, 1, &off, &len, pts, n_points, d_out.p, sc, s);
            LURK_HIP_CHECK(hipMemcpyAsync(out32_mont, d_out.p, (size_t)n_points * 32, hipMemcpyDeviceToHost, s));
            LURK_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int lurk_hip_poly_div_linear_dev(int field_id, const void* d_coeffs, size_t len, const void* roots32_mont, int n_roots, void* const* d_quotients,
                                 void* remainders32_mont, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(field_id >= 0 && field_id <= 2, "unknown field id");
        LURK_REQUIRE(n_roots >= 1 && n_roots <= HK_MAX_ROOTS, "1 to 3 roots");
        LURK_REQUIRE(len >= 1, "at least one coefficient");
        LURK_REQUIRE(d_coeffs && roots32_mont && remainders32_mont && (len == 1 || d_quotients), "null argument");
        for (int r = 0; len > 1 && r < n_roots; r++) {
            const char *q = (const char*)d_quotients[r], *b = (const char*)d_coeffs;
            LURK_REQUIRE(q, "null quotient buffer");
            LURK_REQUIRE(q + (len - 1) * 32 <= b || b + len * 32 <= q, "a quotient may not alias the input");
        }
        hipStream_t s = (hipStream_t)stream;
        with_field(field_id, [&](auto tag) {
            using F = decltype(tag);
            Fe<F> roots[HK_MAX_ROOTS];
            memcpy((void*)roots, roots32_mont, (size_t)n_roots * 32);
            void* none[HK_MAX_ROOTS] = {nullptr, nullptr, nullptr};
            ArenaBuf d_rem(HK_MAX_ROOTS * 32, s);
            hk_div_linear<F>(d_coeffs, len, roots, n_roots, len > 1 ? d_quotients : none, d_rem.p, s);
            LURK_HIP_CHECK(hipMemcpyAsync(remainders32_mont, d_rem.p, (size_t)n_roots * 32, hipMemcpyDeviceToHost, s));
            LURK_HIP_CHECK(hipStreamSynchronize(s));
        });
    });
}

int lurk_hip_hyperkzg_prove_dev(lurk_hip_msm_ctx* key, const void* d_poly32_mont, size_t n, const void* x32_mont, lurk_hip_hyperkzg_challenge_fn challenge, void* user,
                                void* out_com_jacobian96, void* out_v32, void* out_w_jacobian96, void* out_y32, void* stream) {
    return guarded([&] {
        LURK_REQUIRE(key && d_poly32_mont && x32_mont && challenge && out_v32 && out_w_jacobian96 && out_y32, "null argument");
        int curve = 0, bits = 0, device = 0;
        size_t points = 0;
        if (lurk_hip_msm_ctx_info(key, &curve, &points, &bits, nullptr) != 0 || lurk_hip_msm_ctx_device(key, &device) != 0)
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, lurk_hip_last_error()};
        if (curve != LURK_CURVE_BN254)
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string("lurk_hip_hyperkzg_prove_dev needs a key on BN254 G1: this key is on ") + curve_name(curve)};
        LURK_REQUIRE(n >= 2 && (n & (n - 1)) == 0, "the number of evaluations must be a power of two >= 2");
        LURK_REQUIRE(n <= points, "the key has fewer points than the polynomial has evaluations");
        int ell = 0;
        while (((size_t)1 << ell) < n) ell++;
        LURK_REQUIRE(ell <= 30, "the polynomial is too long");
        LURK_REQUIRE(ell == 1 || out_com_jacobian96, "null argument");
        DeviceGuard dg(device);
        hyperkzg_prove<Bn254Fr>(key, d_poly32_mont, n, ell, x32_mont, challenge, user, (uint64_t*)out_com_jacobian96, (uint64_t*)out_v32, (uint64_t*)out_w_jacobian96,
                                out_y32, (hipStream_t)stream);
    });
}

int lurk_hip_hyperkzg_pairing_inputs(int curve, int ell, const void* c_jacobian96, const void* x32_canonical, const void* y32_canonical, const void* com_jacobian96,
                                     const void* v32_canonical, const void* w_jacobian96, const void* r32_canonical, const void* q32_canonical,
                                     const void* d32_canonical, void* out_l_jacobian96, void* out_r_jacobian96, int* accepted, int* failed_check) {
    return host_guarded([&] {
        if (curve != LURK_CURVE_BN254) {
            if (curve >= LURK_CURVE_PALLAS && curve <= LURK_CURVE_GRUMPKIN)
                throw HipFailure{LURK_HIP_ERR_INVALID_ARG, std::string("lurk_hip_hyperkzg_pairing_inputs is offered on BN254 G1 only, not on ") + curve_name(curve)};
            throw HipFailure{LURK_HIP_ERR_INVALID_ARG, "unknown curve id"};
        }
        LURK_REQUIRE(ell >= 1 && ell <= 30, "ell out of range");
        LURK_REQUIRE(c_jacobian96 && x32_canonical && y32_canonical && v32_canonical && w_jacobian96 && r32_canonical && q32_canonical && d32_canonical &&
                         out_l_jacobian96 && out_r_jacobian96 && accepted && (ell == 1 || com_jacobian96),
                     "null argument");
        hyperkzg_pairing_inputs(ell, c_jacobian96, x32_canonical, y32_canonical, (const uint64_t*)com_jacobian96, (const uint64_t*)v32_canonical,
                                (const uint64_t*)w_jacobian96, r32_canonical, q32_canonical, d32_canonical, out_l_jacobian96, out_r_jacobian96, accepted, failed_check);
    });
}
}
