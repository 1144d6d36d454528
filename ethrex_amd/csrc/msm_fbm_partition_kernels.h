// ============================================================================
// Bucket partition of the merged fixed-base MSM — gfx950 kernels.
//
// Replaces k_fbm_digits + the 21-bit rocPRIM pair sort + k_offsets of the
// merged mode's stage 1 (geometry and index arithmetic: msm_fbm_partition.h).
// Output: values grouped by bucket id (any order inside a bucket) and the
// bucket offsets.  Every kernel is a template, so only the BN254 G1 TU
// instantiates them.
//
// Blocks coordinate only through kernel boundaries and atomic range
// reservations.  Each pass is count -> exclusive scan -> scatter:
//   count    LDS histogram of the unit's bins, flushed with one global
//            atomicAdd per non-empty bin into cnt[region * 256 + bin]
//   scan     off = exclusive_scan(cnt)   (rocPRIM)
//   scatter  the same histogram again, then ONE reservation per non-empty
//            bin: the unit takes the range that ends at off[bin] + cnt[bin]
//            and counts cnt[bin] down by its share, so the counters are
//            back at zero when the pass is over.  Entries are ranked into
//            LDS in bin order and leave in runs of consecutive addresses.
// The count and scatter kernels of a pass derive the bins the same way from
// the same input, so a reservation can never leave its bin's range.
// ============================================================================
#pragma once
#include <hip/hip_runtime.h>

#include "msm_fbm_partition.h"
#include "msm_kernels.h"   // fe4, SGN_SKIP

namespace em {

constexpr int FBP_BLOCK = 256;
constexpr int FBP_A_SPT = 4;   // scalars per thread of the pass-A count

template <typename CFG>
static __global__ void k_fbp_zero(uint32_t *__restrict__ p, uint32_t n) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

// exclusive prefix of v over the block's 256 threads (all must call)
__device__ __forceinline__ uint32_t fbp_block_scan(uint32_t v, uint32_t *wsum) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t y = __shfl_up(x, d);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t add = 0;
    for (uint32_t k = 0; k < wave; k++) add += wsum[k];
    return add + x - v;
}

// keys and values of scalar i, the k_fbm_digits rule: key = |d| - 1,
// value = table index w*n + i with the sign bit; zero digits and points at
// infinity park at key 0 with SGN_SKIP
template <typename CFG>
__device__ __forceinline__ void fbp_entries(const fe4 &k, bool skip, size_t n,
                                            size_t i, uint32_t *key,
                                            uint32_t *val) {
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < CFG::NWIN_REAL; w++) {
        uint32_t neg;
        uint32_t mag =
            fbm_recode_step<CFG::C>(fbm_digit<CFG::C>(k.v, w), carry, neg);
        bool sk = skip || mag == 0;
        size_t e = (size_t)w * n + i;
        key[w] = sk ? 0u : mag - 1;
        val[w] = (uint32_t)e | (neg << 31) | (sk ? SGN_SKIP : 0u);
    }
}

// ---- pass A, fused with the digit recode ----
template <typename CFG>
__global__ void __launch_bounds__(FBP_BLOCK)
k_fbp_count_a(const fe4 *__restrict__ scalars, const uint8_t *__restrict__ inf,
              size_t n, uint32_t *__restrict__ cnt) {
    using G = fbp_geom<CFG::IB>;
    constexpr int NW = CFG::NWIN_REAL;
    __shared__ uint32_t lh[G::NBIN_A];
    const uint32_t t = threadIdx.x;
    if (t < G::NBIN_A) lh[t] = 0;
    __syncthreads();
    size_t base = (size_t)blockIdx.x * (FBP_BLOCK * FBP_A_SPT);
    for (int s = 0; s < FBP_A_SPT; s++) {
        size_t i = base + (size_t)s * FBP_BLOCK + t;
        if (i >= n) break;
        uint32_t key[NW], val[NW];
        fbp_entries<CFG>(scalars[i], inf[i] != 0, n, i, key, val);
#pragma unroll
        for (int w = 0; w < NW; w++) atomicAdd(&lh[fbp_bin<FBP_SHIFT_A>(key[w])], 1u);
    }
    __syncthreads();
    if (t < G::NBIN_A && lh[t]) atomicAdd(&cnt[t], lh[t]);
}

// one scalar per thread; the block's NW * 256 entries of all windows are
// ranked together, so a bin's run is hundreds of bytes long
template <typename CFG>
__global__ void __launch_bounds__(FBP_BLOCK)
k_fbp_scatter_a(const fe4 *__restrict__ scalars,
                const uint8_t *__restrict__ inf, size_t n,
                uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                uint16_t *__restrict__ kout, uint32_t *__restrict__ vout) {
    using G = fbp_geom<CFG::IB>;
    constexpr int NW = CFG::NWIN_REAL;
    constexpr int E = FBP_BLOCK * NW;
    __shared__ uint32_t lv[E];
    __shared__ uint16_t lk[E];
    __shared__ uint8_t lb[E];
    __shared__ uint32_t lh[G::NBIN_A], lcur[G::NBIN_A], ldelta[G::NBIN_A];
    __shared__ uint32_t wsum[FBP_BLOCK / 64];
    const uint32_t t = threadIdx.x;
    if (t < G::NBIN_A) lh[t] = 0;
    __syncthreads();
    const size_t first = (size_t)blockIdx.x * FBP_BLOCK;
    const size_t i = first + t;
    const bool valid = i < n;
    uint32_t key[NW], val[NW];
    if (valid) {
        fbp_entries<CFG>(scalars[i], inf[i] != 0, n, i, key, val);
#pragma unroll
        for (int w = 0; w < NW; w++) atomicAdd(&lh[fbp_bin<FBP_SHIFT_A>(key[w])], 1u);
    }
    __syncthreads();
    const uint32_t mine = t < G::NBIN_A ? lh[t] : 0u;
    const uint32_t ex = fbp_block_scan(mine, wsum);
    if (t < G::NBIN_A) {
        lcur[t] = ex;
        // dst of LDS slot j of this bin = (reserved start) + (j - ex)
        if (mine) ldelta[t] = off[t] + (atomicSub(&cnt[t], mine) - mine) - ex;
    }
    __syncthreads();
    if (valid) {
#pragma unroll
        for (int w = 0; w < NW; w++) {
            uint32_t b = fbp_bin<FBP_SHIFT_A>(key[w]);
            uint32_t pos = atomicAdd(&lcur[b], 1u);
            lv[pos] = val[w];
            lk[pos] = (uint16_t)fbp_low<FBP_SHIFT_A>(key[w]);
            lb[pos] = (uint8_t)b;
        }
    }
    __syncthreads();
    const size_t left = n - first;   // first < n: the grid covers n exactly
    const uint32_t cntv =
        (uint32_t)(left < (size_t)FBP_BLOCK ? left : (size_t)FBP_BLOCK) * NW;
    for (uint32_t j = t; j < cntv; j += FBP_BLOCK) {
        uint32_t dst = ldelta[lb[j]] + j;
        vout[dst] = lv[j];
        kout[dst] = lk[j];
    }
}

// ---- passes B and C: units of at most T entries of one region ----
// units per region; entry `regions` = 0 so the scan's last element is the
// number of units in use
template <typename CFG>
static __global__ void k_fbp_unit_counts(const uint32_t *__restrict__ off,
                                         uint32_t regions, uint32_t T,
                                         uint32_t *__restrict__ ucnt) {
    uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > regions) return;
    ucnt[r] = r == regions ? 0u : fbp_units(off[r + 1] - off[r], T);
}

// B: u16 keys, SHIFT 8; C: u8 keys, SHIFT 0
template <typename KIN, int SHIFT>
__global__ void __launch_bounds__(FBP_BLOCK)
k_fbp_count(const KIN *__restrict__ kin, const uint32_t *__restrict__ off,
            const uint32_t *__restrict__ uoff, uint32_t regions, uint32_t T,
            uint32_t *__restrict__ cnt) {
    __shared__ uint32_t lh[256];
    const uint32_t t = threadIdx.x, u = blockIdx.x;
    if (u >= uoff[regions]) return;   // surplus block of the host-side bound
    const uint32_t r = fbp_region_of(uoff, regions, u);
    uint32_t lo, hi;
    fbp_unit_range(off, uoff, r, u, T, lo, hi);
    lh[t] = 0;
    __syncthreads();
    for (uint32_t j = lo + t; j < hi; j += FBP_BLOCK)
        atomicAdd(&lh[fbp_bin<SHIFT>((uint32_t)kin[j])], 1u);
    __syncthreads();
    if (lh[t]) atomicAdd(&cnt[r * 256u + t], lh[t]);
}

// dynamic LDS: T values (u32) followed by T incoming keys
template <typename KIN, typename KOUT, int SHIFT, bool WRITE_KEYS>
__global__ void __launch_bounds__(FBP_BLOCK)
k_fbp_scatter(const KIN *__restrict__ kin, const uint32_t *__restrict__ vin,
              const uint32_t *__restrict__ off,
              const uint32_t *__restrict__ uoff, uint32_t regions, uint32_t T,
              uint32_t *__restrict__ cnt, const uint32_t *__restrict__ boff,
              KOUT *__restrict__ kout, uint32_t *__restrict__ vout) {
    extern __shared__ __align__(16) unsigned char fbp_dyn[];
    uint32_t *lv = reinterpret_cast<uint32_t *>(fbp_dyn);
    KIN *lk = reinterpret_cast<KIN *>(lv + T);
    __shared__ uint32_t lh[256], lcur[256], ldelta[256];
    __shared__ uint32_t wsum[FBP_BLOCK / 64];
    const uint32_t t = threadIdx.x, u = blockIdx.x;
    if (u >= uoff[regions]) return;
    const uint32_t r = fbp_region_of(uoff, regions, u);
    uint32_t lo, hi;
    fbp_unit_range(off, uoff, r, u, T, lo, hi);
    lh[t] = 0;
    __syncthreads();
    for (uint32_t j = lo + t; j < hi; j += FBP_BLOCK)
        atomicAdd(&lh[fbp_bin<SHIFT>((uint32_t)kin[j])], 1u);
    __syncthreads();
    const uint32_t mine = lh[t];
    const uint32_t ex = fbp_block_scan(mine, wsum);
    lcur[t] = ex;
    if (mine) {
        const uint32_t g = r * 256u + t;
        ldelta[t] = boff[g] + (atomicSub(&cnt[g], mine) - mine) - ex;
    }
    __syncthreads();
    for (uint32_t j = lo + t; j < hi; j += FBP_BLOCK) {
        KIN k = kin[j];
        uint32_t pos = atomicAdd(&lcur[fbp_bin<SHIFT>((uint32_t)k)], 1u);
        lv[pos] = vin[j];
        lk[pos] = k;
    }
    __syncthreads();
    const uint32_t len = hi - lo;   // <= T
    for (uint32_t j = t; j < len; j += FBP_BLOCK) {
        KIN k = lk[j];
        uint32_t dst = ldelta[fbp_bin<SHIFT>((uint32_t)k)] + j;
        vout[dst] = lv[j];
        if constexpr (WRITE_KEYS)
            kout[dst] = (KOUT)fbp_low<SHIFT>((uint32_t)k);
    }
}

}  // namespace em
