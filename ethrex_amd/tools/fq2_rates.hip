// Microbenchmark: the fused Fq2 multiply (fq2_mul_f: 4 products, 2
// Montgomery reductions) against Karatsuba (fq2_mul_k: 3 products, 3
// reductions, 3 subtractions) on gfx950, as one dependent chain per thread
// and as four independent chains per thread.  Prints ns per multiply per
// thread-chain and the aggregate multiplies/s, median of REPS timed launches
// after one warm-up, with the min..max spread.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I ../csrc fq2_rates.hip \
//         -o fq2_rates
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include "gpu_g2_bn254.h"
using namespace em;

#define ITER 2048
#define REPS 7
constexpr int BLOCKS = 2048, THREADS = 256;

__device__ __forceinline__ fq2 seed_fq2(u64 seed, u32 salt) {
    // any norm2p-shaped value works: limbs < 2^29, top limb small
    fq2 r;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        r.c0.v[i] = (u32)(seed * (2 * i + 3) + salt + threadIdx.x) & 0x0fffffffu;
        r.c1.v[i] = (u32)(seed * (2 * i + 5) ^ (salt + blockIdx.x)) & 0x0fffffffu;
    }
    r.c0.v[8] &= 0xfffff;
    r.c1.v[8] &= 0xfffff;
    return r;
}
__device__ __forceinline__ u64 fold(const fq2 &a) {
    u64 s = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) s += (u64)a.c0.v[i] * 3 + a.c1.v[i];
    return s;
}

template <bool FUSED>
__device__ __forceinline__ fq2 mulv(const fq2 &a, const fq2 &b) {
    if constexpr (FUSED) return fq2_mul_f(a, b);
    else return fq2_mul_k(a, b);
}

// one dependent chain: x = x * y
template <bool FUSED>
__global__ void __launch_bounds__(256) k_dep(u64 *out, u64 seed) {
    fq2 x = seed_fq2(seed, 1), y = seed_fq2(seed, 2);
    for (int i = 0; i < ITER; i++) x = mulv<FUSED>(x, y);
    out[blockIdx.x * blockDim.x + threadIdx.x] = fold(x);
}
// four independent chains
template <bool FUSED>
__global__ void __launch_bounds__(256) k_ilp(u64 *out, u64 seed) {
    fq2 a = seed_fq2(seed, 1), b = seed_fq2(seed, 2), c = seed_fq2(seed, 3),
        d = seed_fq2(seed, 4), y = seed_fq2(seed, 5);
    for (int i = 0; i < ITER / 4; i++) {
        a = mulv<FUSED>(a, y);
        b = mulv<FUSED>(b, y);
        c = mulv<FUSED>(c, y);
        d = mulv<FUSED>(d, y);
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = fold(a) + fold(b) + fold(c) + fold(d);
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int run(void (*k)(u64 *, u64), const char *name, u64 *d) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k, dim3(BLOCKS), dim3(THREADS), 0, 0, d, 12345ull);
    CK(hipDeviceSynchronize());
    float ms[REPS];
    for (int r = 0; r < REPS; r++) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k, dim3(BLOCKS), dim3(THREADS), 0, 0, d, 777ull + r);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms[r], e0, e1));
    }
    std::sort(ms, ms + REPS);
    double muls = (double)BLOCKS * THREADS * ITER;
    std::printf("%-22s median %8.3f ms (min %8.3f max %8.3f)  %7.2f G fq2-mul/s\n",
                name, ms[REPS / 2], ms[0], ms[REPS - 1],
                muls / (ms[REPS / 2] * 1e-3) / 1e9);
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    return 0;
}

int main() {
    u64 *d;
    CK(hipMalloc(&d, (size_t)BLOCKS * THREADS * 8));
    int rc = 0;
    rc |= run(k_dep<true>, "fused     dependent", d);
    rc |= run(k_dep<false>, "karatsuba dependent", d);
    rc |= run(k_ilp<true>, "fused     4 chains", d);
    rc |= run(k_ilp<false>, "karatsuba 4 chains", d);
    CK(hipFree(d));
    return rc;
}
