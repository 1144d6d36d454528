// ============================================================================
// Bucket partition of the merged fixed-base MSM: index arithmetic.
//
// The walk needs the entries of each bucket contiguous plus the bucket
// offsets; it needs neither order inside a bucket, stability, nor the
// sorted keys.  So the IB = C-1 key bits are consumed from the top by an
// unstable three-pass partition whose key shrinks from pass to pass:
//
//   pass A  BITS_A = IB-16 bits   scalars        -> (u16 low key, u32 value)
//   pass B  8 bits                 (u16, u32)     -> (u8 low key,  u32 value)
//   pass C  8 bits                 (u8, u32)      -> u32 value
//
// The bins of one pass are the regions of the next.  A region is cut into
// work units of at most T entries; unit u of region r covers
// [off[r] + (u - uoff[r]) * T, ...) where uoff is the exclusive scan of the
// regions' unit counts.  The exclusive scan of pass C's 2^IB bin counts is
// the bucket offset array.
//
// This header holds only that arithmetic, host and device, with no
// dependency on the field headers: ethrex_amd/tools/fbm_partition_check.cpp
// builds it alone and emulates the three passes on the CPU.
// ============================================================================
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "msm_fb_recode.h"

namespace em {

constexpr uint32_t FBP_TILE_MAX = 8192;   // most entries one unit takes
constexpr uint32_t FBP_TILE_DEFAULT = 4096;

template <int IB_>
struct fbp_geom {
    static_assert(IB_ > 16 && IB_ - 16 <= 8, "pass A takes 1..8 bits");
    static constexpr int IB = IB_;
    static constexpr int BITS_A = IB - 16;
    static constexpr uint32_t NBIN_A = 1u << BITS_A;    // = regions of pass B
    static constexpr uint32_t NREG_B = NBIN_A;
    static constexpr uint32_t NREG_C = 1u << (IB - 8);  // = NREG_B * 256
    static constexpr uint32_t NBUCKETS = 1u << IB;      // = NREG_C * 256
};

// a pass splits its incoming key at bit SHIFT (A: 16, B: 8, C: 0): the top
// part is the bin, the low part is the key the next pass receives
constexpr int FBP_SHIFT_A = 16, FBP_SHIFT_B = 8, FBP_SHIFT_C = 0;
template <int SHIFT>
EM_FBM_HD uint32_t fbp_bin(uint32_t key) {
    return key >> SHIFT;
}
template <int SHIFT>
EM_FBM_HD uint32_t fbp_low(uint32_t key) {
    return key & ((1u << SHIFT) - 1u);
}

// units a region of `len` entries is cut into (none for an empty region)
EM_FBM_HD uint32_t fbp_units(uint32_t len, uint32_t T) {
    return (len + T - 1) / T;
}

// host-side grid bound: sum_r ceil(len_r / T) <= total/T + regions
inline uint32_t fbp_grid(size_t total, uint32_t T, uint32_t regions) {
    return (uint32_t)(total / T) + regions + 1;
}

// the region of unit u < uoff[regions]: the largest r with uoff[r] <= u
// (uoff non-decreasing, uoff[0] = 0; empty regions repeat their successor's
// value, so the largest such r is the one that owns the unit)
EM_FBM_HD uint32_t fbp_region_of(const uint32_t *uoff, uint32_t regions,
                                 uint32_t u) {
    uint32_t lo = 0, hi = regions;
    while (lo < hi) {
        uint32_t mid = (lo + hi + 1) >> 1;
        if (uoff[mid] <= u)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// entries [lo, hi) of unit u of region r
EM_FBM_HD void fbp_unit_range(const uint32_t *off, const uint32_t *uoff,
                              uint32_t r, uint32_t u, uint32_t T, uint32_t &lo,
                              uint32_t &hi) {
    uint32_t end = off[r + 1];
    lo = off[r] + (u - uoff[r]) * T;
    hi = end - lo > T ? lo + T : end;
}

}  // namespace em
