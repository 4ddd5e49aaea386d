// f29_p1_probe.hip - TEST ONLY: the narrow-contract products of field29.cuh (f29_mul30, f29_sqr30, a two-term row through
// dot29_finish2), one lane per row in ONE launch per field, for tests/test_gpu_field29_p1.py.  Built twice: as it is (the Pasta
// fields run the blocks of field29_mul_asm_p1.cuh) and with -DLURK_F29_P1=0 (the plain blocks).
//
//   f29_p1_probe <in> <out>
//
// <in>:  u32 n, then per field (PallasFp, PallasFq) A[n * 9], B[n * 9]: nine radix-2^29 limbs per row, A tight, B with limbs < 2^30
// <out>: per field, n rows of 27 u32:  f29_mul30(a, b) | f29_sqr30(a) | a * b' + a' * b  with a' the next row's a (cyclic) and b',
//        the row's b with its limbs masked to 29 bits (the row's operands are tight)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lurk_beta_amd/csrc/field29.cuh"

using namespace lurk;

template <class P>
__device__ F29<P> ld(const uint32_t* src, int row, uint32_t mask) {
    F29<P> x;
#pragma unroll
    for (int k = 0; k < 9; k++) x.l[k] = src[(size_t)row * 9 + k] & mask;
    return x;
}

template <class P>
__global__ void probe_kernel(int n, const uint32_t* __restrict__ A, const uint32_t* __restrict__ B, uint32_t* __restrict__ O) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = i + 1 < n ? i + 1 : 0;
    const F29<P> a = ld<P>(A, i, 0xffffffffu), b = ld<P>(B, i, 0xffffffffu);
    const F29<P> m = f29_mul30<P>(a, b);
    const F29<P> s = f29_sqr30<P>(a);
    Dot29<P> row;
    dot29_init<P>(row);
    dot29_mac<P>(row, a, ld<P>(B, i, F29_MASK));
    dot29_mac<P>(row, ld<P>(A, j, 0xffffffffu), ld<P>(B, j, F29_MASK));
    const F29<P> d = dot29_finish2<P>(row);
    uint32_t* o = O + (size_t)i * 27;
    for (int k = 0; k < 9; k++) { o[k] = m.l[k]; o[9 + k] = s.l[k]; o[18 + k] = d.l[k]; }
}

#define CHECK(x)                                                                          \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));                \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    uint32_t n = 0;
    if (!in || !out || fread(&n, 4, 1, in) != 1 || n == 0 || n > (1u << 20)) {
        fprintf(stderr, "bad input\n");
        return 3;
    }
    const size_t words = (size_t)n * 9;
    std::vector<uint32_t> a(words), b(words), o((size_t)n * 27);
    uint32_t *dA, *dB, *dO;
    CHECK(hipMalloc(&dA, words * 4));
    CHECK(hipMalloc(&dB, words * 4));
    CHECK(hipMalloc(&dO, o.size() * 4));
    for (int field = 0; field < 2; field++) {
        if (fread(a.data(), 4, words, in) != words || fread(b.data(), 4, words, in) != words) {
            fprintf(stderr, "input truncated\n");
            return 3;
        }
        CHECK(hipMemcpy(dA, a.data(), words * 4, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(dB, b.data(), words * 4, hipMemcpyHostToDevice));
        CHECK(hipMemset(dO, 0xA5, o.size() * 4));
        const int bs = 256, grid = (int)((n + bs - 1) / bs);
        if (field == 0) probe_kernel<PallasFp><<<grid, bs>>>((int)n, dA, dB, dO);
        else probe_kernel<PallasFq><<<grid, bs>>>((int)n, dA, dB, dO);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(o.data(), dO, o.size() * 4, hipMemcpyDeviceToHost));
        if (fwrite(o.data(), 4, o.size(), out) != o.size()) return 4;
    }
    CHECK(hipFree(dA));
    CHECK(hipFree(dB));
    CHECK(hipFree(dO));
    fclose(in);
    return fclose(out) != 0 ? 4 : 0;
}
