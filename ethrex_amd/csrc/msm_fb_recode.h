// ============================================================================
// Merged fixed-base geometry for large BN254 G1 MSMs: signed digits,
// NWIN_REAL scalar windows of C bits, ONE bucket space of 2^(C-1).
//
// With the table T[w*n + i] = 2^(C*w) * P_i resident (the bases are the
// proving-key queries: loaded once, reused across proofs), every window's
// digits land in the same buckets, so the bucket reduction is paid once
// instead of once per window and C can grow past the separate-window
// optimum of 17.  Adds per step: NWIN_REAL*n + 2^C instead of
// 15*(n + 2^17).
//
// This header holds only the geometry and the digit recode, host and
// device, with no dependency on the field headers:
// ethrex_amd/tools/fb_recode_check.cpp builds it alone.
// ============================================================================
#pragma once
#include <stdint.h>
#include <type_traits>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EM_FBM_HD __host__ __device__ __forceinline__
#else
#define EM_FBM_HD inline
#endif

namespace em {

template <int CB, int SBITS>
struct msm_cfg_fbm {
    static constexpr bool SIGNED = true;
    static constexpr int C = CB;                 // window bits
    static constexpr int IB = CB - 1;            // bucket-index bits
    static constexpr int NWIN = 1;               // bucket spaces (reduction)
    static constexpr int NWIN_REAL = (SBITS + CB - 1) / CB;  // scalar windows
    // the top window holds TOP_BITS < C bits; value + carry <= 2^TOP_BITS
    // must not exceed 2^(C-1), the largest magnitude a bucket id can carry,
    // and must never carry out
    static constexpr int TOP_BITS = SBITS - CB * (NWIN_REAL - 1);
    static_assert(TOP_BITS >= 1 && TOP_BITS <= CB - 1,
                  "top window must absorb the final carry");
    static constexpr uint32_t DMASK = (1u << IB) - 1;
    static constexpr uint32_t NBUCKETS = 1u << IB;
    static constexpr int DBITS = IB;
    static constexpr int SORT_BITS = IB;         // one global sort, id bits
    static constexpr int SEG = 16;
    static constexpr int NSEG = (1 << IB) / SEG;
    static constexpr int RED_BLOCK = 256;
    static constexpr bool TREE = true;
    static constexpr int NPART = NSEG / RED_BLOCK;
    // The top window's digits are < 2^TOP_BITS, so n entries pile into the
    // lowest buckets (n / 0.19*2^TOP_BITS each: 21 000 at 2^24, c=22,
    // against an average run of 96).  Runs are therefore cut into chunks
    // of at most L >= total/NBUCKETS entries, one walk thread ("slot")
    // each: sum_b max(1, ceil(len_b / L)) <= NBUCKETS + total/L <= NSLOT.
    static constexpr uint32_t NSLOT = 2u * NBUCKETS;
    static constexpr int CGRP = 16;              // chunks per combine group
};

template <typename T>
struct is_fbm : std::false_type {};
template <int CB, int SBITS>
struct is_fbm<msm_cfg_fbm<CB, SBITS>> : std::true_type {};

// the A/B set; the default is chosen in msm_create_t
using CfgFbm20 = msm_cfg_fbm<20, 254>;  // 13 windows, 2^19 buckets
using CfgFbm22 = msm_cfg_fbm<22, 254>;  // 12 windows, 2^21 buckets
using CfgFbm24 = msm_cfg_fbm<24, 254>;  // 11 windows, 2^23 buckets

// raw window w of a 256-bit little-endian scalar (bits [CB*w, CB*w + CB))
template <int CB>
EM_FBM_HD uint32_t fbm_digit(const uint64_t k[4], int w) {
    int bit = CB * w;
    int limb = bit >> 6, off = bit & 63;
    uint64_t d = k[limb] >> off;
    if (off > 64 - CB && limb < 3) d |= k[limb + 1] << (64 - off);
    return (uint32_t)d & ((1u << CB) - 1);
}

// one step of the balanced recode (the k_digits rule): t = raw + carry_in;
// t <= 2^(C-1) keeps d = +t, else d = t - 2^C with a carry into the next
// window.  Returns |d| (0 .. 2^(C-1)); neg and carry are updated.
template <int CB>
EM_FBM_HD uint32_t fbm_recode_step(uint32_t raw, uint32_t &carry,
                                   uint32_t &neg) {
    uint32_t t = raw + carry;
    if (t > (1u << (CB - 1))) {
        neg = 1;
        carry = 1;
        return (1u << CB) - t;
    }
    neg = 0;
    carry = 0;
    return t;
}

}  // namespace em
