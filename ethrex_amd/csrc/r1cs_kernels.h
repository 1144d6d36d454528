// ============================================================================
// Sparse R1CS matrix times witness over BN254 Fr — gfx950 kernels on the fe9
// field core.  y = M z for a matrix packed by r1cs_pack.h (sliced-ELL short
// rows + chunked long rows, coefficients through a dictionary).
//
// A stored nonzero is {u32 col, u32 id}, read as one 8-B load per lane, 64
// consecutive entries per wave.  z[col] is one 32-B fe4m gather.  id 0 (+1)
// adds z[col] to the accumulator, id 1 (-1) adds it to a second accumulator
// that is subtracted once per lane at the end; only id >= 2 runs a
// Montgomery multiply with the dictionary entry.
//
// Bounds.  Every accumulation is add9_n: both operands are norm2p (limbs
// < 2^29, value < 2p) — z as stored by k_fr_from_be / the transforms, a
// product as mont_mul9 returns it (< 1.01p), an accumulator as add9_n
// returns it — so the limb sum is < 2^30 and the value sum < 4p, which is
// add9_n's contract, and the result is norm2p again.  Nothing is summed
// lazily, so the row length enters no bound.  mont_mul9 takes z (< 2p) and
// a dictionary entry (to_mont9 output, < 1.01p): inside its <= 8p / 2^30
// input rule.  pos - neg is subn9 (a, b norm2p).  Field addition is exact,
// so the order of the partial sums does not change the canonical result.
// ============================================================================
#pragma once
#include <hip/hip_runtime.h>
#include "ntt_kernels.h"   // fe4m_pack / fe4m_unpack

namespace em {

// a stored nonzero travels as uint2 {x = col, y = id}; a long-row chunk:
struct r1cs_chk {
    u32 off, len;
};

// acc += coeff(id) * z[col] on the (pos, neg) accumulator pair
__device__ __forceinline__ void r1cs_term(fe9 &pos, fe9 &neg, uint2 e,
                                          const fe9 *__restrict__ dict,
                                          const fe4 *__restrict__ z) {
    fe9 x = fe4m_unpack(z[e.x]);
    if (e.y == 0) {
        pos = add9_n<Fr9T>(pos, x);
    } else if (e.y == 1) {
        neg = add9_n<Fr9T>(neg, x);
    } else {
        pos = add9_n<Fr9T>(pos, mont_mul9<Fr9T>(x, dict[e.y]));
    }
}

// sum of v over the 64 lanes of the wave (every lane gets it)
__device__ __forceinline__ fe9 r1cs_wave_sum(fe9 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        fe9 o;
#pragma unroll
        for (int i = 0; i < 9; i++) o.v[i] = __shfl_xor(v.v[i], d, 64);
        v = add9_n<Fr9T>(v, o);
    }
    return v;
}

// Short rows: one lane per row of a 64-row slice, four slices per block.
// s_off[s] is the entry offset of slice s ([k][lane] inside), s_len the
// lane's row length (entries at k >= s_len are padding and are not read as
// terms), s_perm the row the lane's sum is stored to (0xffffffff: none).
__global__ void __launch_bounds__(256)
k_r1cs_rows_sell(const uint2 *__restrict__ ent, const u64 *__restrict__ s_off,
                 const u32 *__restrict__ s_len, const u32 *__restrict__ s_perm,
                 u32 n_slices, const fe9 *__restrict__ dict,
                 const fe4 *__restrict__ z, fe4 *__restrict__ y) {
    const u32 slice = blockIdx.x * 4 + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63;
    if (slice >= n_slices) return;
    const u64 base = s_off[slice];
    const u32 width = (u32)((s_off[slice + 1] - base) >> 6);
    const size_t j = (size_t)slice * 64 + lane;
    const u32 len = s_len[j];
    fe9 pos = fe9_zero(), neg = fe9_zero();
    for (u32 k = 0; k < width; k++) {
        if (k < len)
            r1cs_term(pos, neg, ent[base + (u64)k * 64 + lane], dict, z);
    }
    const u32 row = s_perm[j];
    if (row != 0xffffffffu) y[row] = fe4m_pack(subn9<Fr9T>(pos, neg));
}

// Long rows, step 1: one wave per chunk, lanes stride the chunk's entries;
// the wave's sum goes to part[chunk] (fe9, norm2p).
__global__ void __launch_bounds__(256)
k_r1cs_rows_long(const uint2 *__restrict__ ent,
                 const r1cs_chk *__restrict__ chunks, u32 n_chunks,
                 const fe9 *__restrict__ dict, const fe4 *__restrict__ z,
                 fe9 *__restrict__ part) {
    const u32 c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63;
    if (c >= n_chunks) return;    // wave-uniform
    const r1cs_chk ch = chunks[c];
    fe9 pos = fe9_zero(), neg = fe9_zero();
    for (u32 i = lane; i < ch.len; i += 64)
        r1cs_term(pos, neg, ent[(size_t)ch.off + i], dict, z);
    fe9 v = r1cs_wave_sum(subn9<Fr9T>(pos, neg));
    if (lane == 0) part[c] = v;
}

// Long rows, step 2: one wave per long row sums the row's chunk partials
// part[chunk_off[j] .. chunk_off[j+1]) and stores y[l_row[j]].
__global__ void __launch_bounds__(256)
k_r1cs_long_sum(const fe9 *__restrict__ part, const u32 *__restrict__ chunk_off,
                const u32 *__restrict__ l_row, u32 n_long,
                fe4 *__restrict__ y) {
    const u32 j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63;
    if (j >= n_long) return;      // wave-uniform
    const u32 end = chunk_off[j + 1];
    fe9 acc = fe9_zero();
    for (u32 c = chunk_off[j] + lane; c < end; c += 64)
        acc = add9_n<Fr9T>(acc, part[c]);
    acc = r1cs_wave_sum(acc);
    if (lane == 0) y[l_row[j]] = fe4m_pack(acc);
}

}  // namespace em
