// ============================================================================
// Radix-2 NTT over BN254 Fr — gfx950 kernels, on the fe9 (9x29-bit) field
// core (carry-free v_mad_u64_u32 columns; see gpu_field9.h).
//
// Transform (same definition as the oracle, oracle/bn254_oracle.c):
//   forward:  A_j = sum_i a_i w^(ij) mod r,  w = W28^(2^(28-log2 n))
//   inverse:  a_i = n^-1 sum_j A_j w^(-ij)
// In/out: 32-byte big-endian canonical Fr elements, natural order.
//
// RESIDENT FORMAT (round 2): the HBM-resident vector and the large twiddle
// tables are PACKED 4x64 Montgomery values ("fe4m", 32 B/element, value
// < 2p < 2^255) — the transform is HBM-bound and the 36-B fe9 format cost
// ~11% extra traffic plus line-straddling gathers.  Elements are unpacked
// to fe9 on load (pure bit repacking, ~30 VALU ops) and repacked on store;
// all arithmetic stays on the 29-bit-limb core.  Small per-row twiddle
// tables (<= 72 KB, L2-resident) stay fe9 to keep per-butterfly loads
// conversion-free.
//
// P1's inter-step twiddle w^(k*c) is read from a REORDERED table
// TW2[c][k] = w^(k*c) (c = row, k = element) so the per-row access is a
// coalesced stream instead of the old stride-c gather over an n-sized
// table (which fetched a full cache line per element).
//
// Two row-kernel shapes, A/B-measured (profiles/r02_summary.md):
// radix-2^2 at 1024 threads (4 waves/SIMD; the DEFAULT — occupancy hides
// the LDS+mul latency best) and radix-2^3 at 512 threads (3 DIT stages
// per LDS round trip, 1/3 the LDS traffic; EM_NTT_R8 selects it).
// EM_NTT_TD sets the radix-2^2 block size.  Both use a SKEWED LDS layout
// — the bit-reversed load scatter otherwise hits one bank group wave-wide
// — and dynamic LDS so 2048-element rows run 2 blocks/CU.
//
// Two paths (selected in api_ntt.hip):
//   13 <= logn <= 24: four-step fused (3 tiled transposes + 2 LDS row-NTT
//   passes); 25-26: two-level four-step; otherwise bit-reverse + logn
//   radix-2 stage launches.  All produce identical integer results (same
//   DFT), parity-pinned against the oracle.
// ============================================================================
#pragma once
#include <hip/hip_runtime.h>
#include "gpu_field.h"   // fe4: the packed 4x64 resident format
#include "gpu_field9.h"

namespace em {

// ---- packed 4x64 Montgomery <-> fe9 (values norm2p < 2p < 2^255) ----
__device__ __forceinline__ fe9 fe4m_unpack(const fe4 &x) {
    return fe9_from_u64x4(x.v);
}
__device__ __forceinline__ fe4 fe4m_pack(const fe9 &x) {
    fe4 r;
    fe9_to_u64x4(r.v, x);
    return r;
}

// ---- conversion / validation ----

// BE bytes -> packed Montgomery; flags err if elem >= r (canonical required)
__global__ void k_fr_from_be(const uint8_t *__restrict__ in,
                             fe4 *__restrict__ out, size_t n,
                             uint32_t *__restrict__ err) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 *w = (const u64 *)(in + 32 * i);
    u64 v[4] = {__builtin_bswap64(w[3]), __builtin_bswap64(w[2]),
                __builtin_bswap64(w[1]), __builtin_bswap64(w[0])};
    fe9 raw = fe9_from_u64x4(v);
    if (fe9_geq_raw(raw, bn254::FR9_P)) atomicOr(err, 1u);
    out[i] = fe4m_pack(to_mont9<Fr9T>(raw));
}

__global__ void k_fr_to_be(const fe4 *__restrict__ in, uint8_t *__restrict__ out,
                           size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe9 c = from_mont9<Fr9T>(fe4m_unpack(in[i]));
    u64 w[4];
    fe9_to_u64x4(w, c);
    u64 *o = (u64 *)(out + 32 * i);
    o[0] = __builtin_bswap64(w[3]);
    o[1] = __builtin_bswap64(w[2]);
    o[2] = __builtin_bswap64(w[1]);
    o[3] = __builtin_bswap64(w[0]);
}

// ---- twiddle / power-table generation ----
// out[j] = s * b^j, j < count (fe9 Montgomery); b2k[k] = b^(2^k), k < bits.
// The row twiddle tables are b = w, s = 1; the coset tables b = g^(+-2^k).
__global__ void k_gen_pow(fe9 *__restrict__ out, size_t count,
                          const fe9 *__restrict__ b2k, int bits, fe9 s) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    fe9 acc = s;
    size_t e = j;
    for (int k = 0; k < bits && e; k++, e >>= 1)
        if (e & 1) acc = mont_mul9<Fr9T>(acc, b2k[k]);
    out[j] = acc;
}

// reordered P1 table (fe4m, streamed): TW2[c*M + k] = w^(k*c), c < rows,
// k < M.  exponent k*c < M*rows = transform size, so <= `bits` bits.
__global__ void k_gen_tw2(fe4 *__restrict__ tw, uint32_t M, size_t rows,
                          const fe9 *__restrict__ w2k, int bits) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (size_t)M * rows) return;
    size_t c = j / M, k = j % M;
    fe9 acc = fe9_load(bn254::FR9_ONE);
    u64 e = (u64)c * k;
    for (int b = 0; b < bits && e; b++, e >>= 1)
        if (e & 1) acc = mont_mul9<Fr9T>(acc, w2k[b]);
    tw[j] = fe4m_pack(acc);
}

// ---- bit-reverse permutation (in-place swap; fallback path) ----
__global__ void k_bit_reverse(fe4 *__restrict__ a, size_t n, int logn) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    size_t j = __brevll(i) >> (64 - logn);
    if (j > i) {
        fe4 t = a[i];
        a[i] = a[j];
        a[j] = t;
    }
}

// ---- one radix-2 DIT stage (fallback path; tw table fe9) ----
__global__ void k_ntt_stage(fe4 *__restrict__ a, const fe9 *__restrict__ tw,
                            size_t n, int logn, int s) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (n >> 1)) return;
    size_t half = (size_t)1 << (s - 1);
    size_t j = t & (half - 1);
    size_t g = t >> (s - 1);
    size_t idx = (g << s) + j;
    fe9 u = fe4m_unpack(a[idx]);
    fe9 v = mont_mul9<Fr9T>(fe4m_unpack(a[idx + half]), tw[j << (logn - s)]);
    a[idx] = fe4m_pack(add9_n<Fr9T>(u, v));
    a[idx + half] = fe4m_pack(subm9<Fr9T>(u, v));  // b = mul output
}

// ---- four-step fused path ----
// n = N1*N2; A[r][c] = a[r*N2+c]:
//   T0: A1[c][r] = A[r][c]; P1: row NTT_N1 + TW2 twiddle;
//   T1; P2: row NTT_N2 (+ 1/n for iNTT); T2 -> natural order.

// tiled fe4 transpose, 32x32 tiles (+1 pad column for LDS banking);
// grid.z = batch of independent R x C sub-matrices at stride R*C
__global__ void __launch_bounds__(256)
k_transpose_fe4(const fe4 *__restrict__ src, fe4 *__restrict__ dst,
                uint32_t R, uint32_t C) {
    __shared__ fe4 tile[32][33];
    size_t base = (size_t)blockIdx.z * R * C;
    uint32_t c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 8 rows/pass
    for (uint32_t dy = ty; dy < 32; dy += 8)
        tile[dy][tx] = src[base + (size_t)(r0 + dy) * C + c0 + tx];
    __syncthreads();
    for (uint32_t dy = ty; dy < 32; dy += 8)
        dst[base + (size_t)(c0 + dy) * R + r0 + tx] = tile[tx][dy];
}

// ---- row NTT of length M = 2^logM, fully in LDS ----
// (fe9: 4096*36 B = 144 KiB, dynamic: (M + M/64) slots, so 2048-element
// rows run 2 blocks/CU (73 KiB) instead of being pinned at the 4096-row
// footprint.)  One body, ntt_row_body<RADIX_LOG2, COSET>, built from the
// pieces below; the block strides over the row, so any block size works.
// tw2 (fe4m, may be null): output k scaled by TW2[c*M + k], c = blockIdx
// & cmask; scale (fe9, may be null): iNTT 1/n factor.
//
// skewed LDS indexing: physical slot = i + (i >> 6).  The bit-reversed
// load scatter otherwise lands a whole wave on one bank group (rev of
// consecutive i strides 2048 elements; 9*2048 dwords = 0 mod 64 banks
// = a 64-way conflict); with the skew, lane l's slot moves by
// rev6(l)*65 -> 9*rev6(l) mod 64, a permutation of the banks.
__device__ __forceinline__ constexpr uint32_t row_sk(uint32_t i) {
    return i + (i >> 6);
}

// COSET (compile-time, so the plain COSET = 0 kernels carry none of it):
//   0  plain transform; cs_elem / cs_row unused.
//   1  coset forward, P1: element i is multiplied by cs_elem[i] = (g^N2)^i
//      on load and output row c additionally by cs_row[c] = g^c.
//   2  coset inverse, P2: output k of row k1 is multiplied by
//      cs_row[k1] = g^(-k1) n^-1 and cs_elem[k] = (g^(-N1))^k (scale unused).
// Both tables are fe9, at most 4096 entries, shared by all rows.

// bit-reversed load of one row into the skewed LDS row
template <int COSET>
__device__ __forceinline__ void
row_load(fe9 *smem, const fe4 *row, int logM,
         const fe9 *__restrict__ cs_elem) {
    const uint32_t M = 1u << logM;
    for (uint32_t i = threadIdx.x; i < M; i += blockDim.x) {
        uint32_t j = __brev(i) >> (32 - logM);
        if constexpr (COSET == 1)
            smem[row_sk(j)] = mont_mul9<Fr9T>(fe4m_unpack(row[i]), cs_elem[i]);
        else
            smem[row_sk(j)] = fe4m_unpack(row[i]);
    }
    __syncthreads();
}

// radix-2 DIT butterfly: (a, b) <- (a + b*w, a - b*w)
__device__ __forceinline__ void row_bfly(fe9 &a, fe9 &b, const fe9 &w) {
    fe9 v = mont_mul9<Fr9T>(b, w);
    b = subm9<Fr9T>(a, v);
    a = add9_n<Fr9T>(a, v);
}

// radix-2^3 round: stages s, s+1, s+2 on 8 register-resident elements
__device__ __forceinline__ void
row_round8(fe9 *smem, const fe9 *__restrict__ tw_row, int logM, int s) {
    const uint32_t M = 1u << logM, q = 1u << (s - 1);
    for (uint32_t t = threadIdx.x; t < (M >> 3); t += blockDim.x) {
        uint32_t j = t & (q - 1);
        uint32_t base = ((t >> (s - 1)) << (s + 2)) + j;
        fe9 e[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) e[k] = smem[row_sk(base + k * q)];
        // stage s: stride-q pairs, shared twiddle
        fe9 w0 = tw_row[j << (logM - s)];
        row_bfly(e[0], e[1], w0);
        row_bfly(e[2], e[3], w0);
        row_bfly(e[4], e[5], w0);
        row_bfly(e[6], e[7], w0);
        // stage s+1: stride-2q pairs, twiddles at j and j+q
        fe9 wa = tw_row[j << (logM - s - 1)];
        fe9 wb = tw_row[(j + q) << (logM - s - 1)];
        row_bfly(e[0], e[2], wa);
        row_bfly(e[1], e[3], wb);
        row_bfly(e[4], e[6], wa);
        row_bfly(e[5], e[7], wb);
        // stage s+2: stride-4q pairs, twiddles at j, j+q, j+2q, j+3q
        fe9 w4a = tw_row[j << (logM - s - 2)];
        fe9 w4b = tw_row[(j + q) << (logM - s - 2)];
        fe9 w4c = tw_row[(j + 2 * q) << (logM - s - 2)];
        fe9 w4d = tw_row[(j + 3 * q) << (logM - s - 2)];
        row_bfly(e[0], e[4], w4a);
        row_bfly(e[1], e[5], w4b);
        row_bfly(e[2], e[6], w4c);
        row_bfly(e[3], e[7], w4d);
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) smem[row_sk(base + k * q)] = e[k];
    }
    __syncthreads();
}

// radix-2^2 round: stages s, s+1 on 4 elements
__device__ __forceinline__ void
row_round4(fe9 *smem, const fe9 *__restrict__ tw_row, int logM, int s) {
    const uint32_t M = 1u << logM, q = 1u << (s - 1);
    for (uint32_t t = threadIdx.x; t < (M >> 2); t += blockDim.x) {
        uint32_t j = t & (q - 1);
        uint32_t idx = ((t >> (s - 1)) << (s + 1)) + j;
        fe9 w1 = tw_row[j << (logM - s)];
        fe9 a = smem[row_sk(idx)];
        fe9 b = mont_mul9<Fr9T>(smem[row_sk(idx + q)], w1);
        fe9 c = smem[row_sk(idx + 2 * q)];
        fe9 d = mont_mul9<Fr9T>(smem[row_sk(idx + 3 * q)], w1);
        fe9 t0 = add9_n<Fr9T>(a, b);
        fe9 t1 = subm9<Fr9T>(a, b);
        fe9 t2 = add9_n<Fr9T>(c, d);
        fe9 t3 = subm9<Fr9T>(c, d);
        fe9 u2 = mont_mul9<Fr9T>(t2, tw_row[j << (logM - s - 1)]);
        fe9 u3 = mont_mul9<Fr9T>(t3, tw_row[(j + q) << (logM - s - 1)]);
        smem[row_sk(idx)] = add9_n<Fr9T>(t0, u2);
        smem[row_sk(idx + 2 * q)] = subm9<Fr9T>(t0, u2);
        smem[row_sk(idx + q)] = add9_n<Fr9T>(t1, u3);
        smem[row_sk(idx + 3 * q)] = subm9<Fr9T>(t1, u3);
    }
    __syncthreads();
}

// radix-2 round: stage s
__device__ __forceinline__ void
row_round2(fe9 *smem, const fe9 *__restrict__ tw_row, int logM, int s) {
    const uint32_t M = 1u << logM, half = 1u << (s - 1);
    for (uint32_t t = threadIdx.x; t < (M >> 1); t += blockDim.x) {
        uint32_t j = t & (half - 1);
        uint32_t idx = ((t >> (s - 1)) << s) + j;
        fe9 u = smem[row_sk(idx)];
        fe9 v = mont_mul9<Fr9T>(smem[row_sk(idx + half)],
                                tw_row[j << (logM - s)]);
        smem[row_sk(idx)] = add9_n<Fr9T>(u, v);
        smem[row_sk(idx + half)] = subm9<Fr9T>(u, v);
    }
    __syncthreads();
}

// store epilogue: natural order, with the TW2 / 1/n (COSET = 0) or the
// coset (COSET = 1, 2) output factors
template <int COSET>
__device__ __forceinline__ void
row_store(const fe9 *smem, fe4 *row, int logM,
          const fe4 *__restrict__ tw2, const fe9 *__restrict__ scale,
          uint32_t cmask, const fe9 *__restrict__ cs_elem,
          const fe9 *__restrict__ cs_row) {
    const uint32_t M = 1u << logM;
    uint64_t c = blockIdx.x & cmask;
    const fe4 *t2row = tw2 ? tw2 + (size_t)c * M : nullptr;
    if constexpr (COSET == 0) {
        for (uint32_t k = threadIdx.x; k < M; k += blockDim.x) {
            fe9 x = smem[row_sk(k)];
            if (t2row) x = mont_mul9<Fr9T>(x, fe4m_unpack(t2row[k]));
            if (scale) x = mont_mul9<Fr9T>(x, *scale);
            row[k] = fe4m_pack(x);
        }
    } else {
        const fe9 rowc = cs_row[c];
        for (uint32_t k = threadIdx.x; k < M; k += blockDim.x) {
            fe9 x = mont_mul9<Fr9T>(smem[row_sk(k)], rowc);
            if constexpr (COSET == 1)
                x = mont_mul9<Fr9T>(x, fe4m_unpack(t2row[k]));
            else
                x = mont_mul9<Fr9T>(x, cs_elem[k]);
            row[k] = fe4m_pack(x);
        }
    }
}

// RADIX_LOG2 = 3: radix-2^3 rounds (three DIT stages per LDS round trip),
// then a radix-2^2 / radix-2 tail for logM % 3.  RADIX_LOG2 = 2: radix-2^2
// rounds and a radix-2 tail — 1.5x the LDS round trips, but 4 elements per
// thread, so it runs at 1024 threads and more waves/SIMD.
template <int RADIX_LOG2, int COSET>
__device__ __forceinline__ void
ntt_row_body(fe4 *__restrict__ data, int logM, const fe9 *__restrict__ tw_row,
             const fe4 *__restrict__ tw2, const fe9 *__restrict__ scale,
             uint32_t cmask, const fe9 *__restrict__ cs_elem,
             const fe9 *__restrict__ cs_row) {
    static_assert(RADIX_LOG2 == 3 || RADIX_LOG2 == 2, "row radix");
    static_assert(COSET >= 0 && COSET <= 2, "coset mode");
    extern __shared__ fe9 smem[];
    fe4 *row = data + (size_t)blockIdx.x * (1u << logM);
    row_load<COSET>(smem, row, logM, cs_elem);
    int s = 1;
    if constexpr (RADIX_LOG2 == 3)
        for (; s + 2 <= logM; s += 3) row_round8(smem, tw_row, logM, s);
    for (; s + 1 <= logM; s += 2) row_round4(smem, tw_row, logM, s);
    for (; s <= logM; s++) row_round2(smem, tw_row, logM, s);
    row_store<COSET>(smem, row, logM, tw2, scale, cmask, cs_elem, cs_row);
}

// The six entry points.  k_ntt_row4*: radix-2^2, the default, at 1024
// threads (EM_NTT_TD sets another block size); k_ntt_row*: radix-2^3 at
// 512 threads, selected by EM_NTT_R8.  The _coset kernels take COSET = 1
// or 2 (tw2 is required for COSET = 1).
__global__ void __launch_bounds__(512)
k_ntt_row(fe4 *__restrict__ data, int logM, const fe9 *__restrict__ tw_row,
          const fe4 *__restrict__ tw2, const fe9 *__restrict__ scale,
          uint32_t cmask = 0xffffffffu) {
    ntt_row_body<3, 0>(data, logM, tw_row, tw2, scale, cmask, nullptr, nullptr);
}

__global__ void __launch_bounds__(1024)
k_ntt_row4(fe4 *__restrict__ data, int logM, const fe9 *__restrict__ tw_row,
           const fe4 *__restrict__ tw2, const fe9 *__restrict__ scale,
           uint32_t cmask) {
    ntt_row_body<2, 0>(data, logM, tw_row, tw2, scale, cmask, nullptr, nullptr);
}

template <int COSET>
__global__ void __launch_bounds__(512)
k_ntt_row_coset(fe4 *__restrict__ data, int logM,
                const fe9 *__restrict__ tw_row, const fe4 *__restrict__ tw2,
                const fe9 *__restrict__ cs_elem,
                const fe9 *__restrict__ cs_row) {
    static_assert(COSET == 1 || COSET == 2, "coset mode");
    ntt_row_body<3, COSET>(data, logM, tw_row, tw2, nullptr, 0xffffffffu,
                           cs_elem, cs_row);
}

template <int COSET>
__global__ void __launch_bounds__(1024)
k_ntt_row4_coset(fe4 *__restrict__ data, int logM,
                 const fe9 *__restrict__ tw_row, const fe4 *__restrict__ tw2,
                 const fe9 *__restrict__ cs_elem,
                 const fe9 *__restrict__ cs_row) {
    static_assert(COSET == 1 || COSET == 2, "coset mode");
    ntt_row_body<2, COSET>(data, logM, tw_row, tw2, nullptr, 0xffffffffu,
                           cs_elem, cs_row);
}

// packed small-row NTT: 1024/M rows of length M <= 512 per block (the
// 144-KB k_ntt_row runs one block/CU and would idle 1-(M/4096) of its
// threads on the two-level path's 64/128-point inner rows).  One butterfly
// per thread per stage; rows packed smem[rr*M + j].  tw2 is the reordered
// [c][k] table of the INNER transform (c = row index & cmask).
__global__ void __launch_bounds__(512)
k_ntt_row_small(fe4 *__restrict__ data, int logM,
                const fe9 *__restrict__ tw_row,
                const fe4 *__restrict__ tw2,
                const fe9 *__restrict__ scale, uint32_t cmask) {
    __shared__ fe9 smem[1024];
    const uint32_t M = 1u << logM;
    size_t row0 = (size_t)blockIdx.x * (1024u >> logM);
    fe4 *base = data + row0 * M;
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) {
        uint32_t rr = i >> logM, j = i & (M - 1);
        smem[rr * M + (__brev(j) >> (32 - logM))] = fe4m_unpack(base[i]);
    }
    __syncthreads();
    for (int s = 1; s <= logM; s++) {
        uint32_t half = 1u << (s - 1);
        uint32_t t = threadIdx.x;  // 512 butterflies = 1024 elements
        uint32_t rr = t >> (logM - 1), ti = t & ((M >> 1) - 1);
        uint32_t j = ti & (half - 1);
        uint32_t idx = rr * M + ((ti >> (s - 1)) << s) + j;
        fe9 u = smem[idx];
        fe9 v = mont_mul9<Fr9T>(smem[idx + half], tw_row[j << (logM - s)]);
        smem[idx] = add9_n<Fr9T>(u, v);
        smem[idx + half] = subm9<Fr9T>(u, v);
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) {
        uint32_t rr = i >> logM, kk = i & (M - 1);
        uint64_t c = (uint64_t)((row0 + rr) & cmask);
        fe9 x = smem[i];
        if (tw2) x = mont_mul9<Fr9T>(x, fe4m_unpack(tw2[(size_t)c * M + kk]));
        if (scale) x = mont_mul9<Fr9T>(x, *scale);
        base[i] = fe4m_pack(x);
    }
}

// ---- scale by n^-1 (iNTT, fallback path) ----
__global__ void k_ntt_scale(fe4 *__restrict__ a, size_t n, int logn) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a[i] = fe4m_pack(mont_mul9<Fr9T>(fe4m_unpack(a[i]),
                                     fe9_load(bn254::FR9_INV_POW2[logn])));
}

// ---- coset / quotient support (DESIGN.md "Quotient polynomial") ----

// standalone coset scale: a[i] *= hi[i >> lo_bits] * lo[i & (2^lo_bits - 1)]
// (g^(+-i), and the 1/n of the inverse, split over two small tables)
__global__ void k_coset_scale(fe4 *__restrict__ a, size_t n,
                              const fe9 *__restrict__ hi,
                              const fe9 *__restrict__ lo, int lo_bits) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe9 x = mont_mul9<Fr9T>(fe4m_unpack(a[i]), hi[i >> lo_bits]);
    x = mont_mul9<Fr9T>(x, lo[i & (((size_t)1 << lo_bits) - 1)]);
    a[i] = fe4m_pack(x);
}

// c[i] = a[i] * b[i]
__global__ void k_fr_mul(const fe4 *__restrict__ a, const fe4 *__restrict__ b,
                         fe4 *__restrict__ c, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    c[i] = fe4m_pack(mont_mul9<Fr9T>(fe4m_unpack(a[i]), fe4m_unpack(b[i])));
}

// a[j] = (a[j] * b[j] - c[j]) * d: one pass, reads 3 vectors, writes 1.
// c is a stored value (norm2p, not a mul output) => subn9.
__global__ void k_quot_pointwise(fe4 *__restrict__ a,
                                 const fe4 *__restrict__ b,
                                 const fe4 *__restrict__ c, size_t n, fe9 d) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    fe9 ab = mont_mul9<Fr9T>(fe4m_unpack(a[j]), fe4m_unpack(b[j]));
    fe9 t = subn9<Fr9T>(ab, fe4m_unpack(c[j]));
    a[j] = fe4m_pack(mont_mul9<Fr9T>(t, d));
}

}  // namespace em
