// ============================================================================
// Batched Keccak-256 on gfx950 (the witness/statement
// hashing step feeding the prover — ExecBackend::execute_core's keccak/trie
// hashing; the reference computes these one at a time through hand-written
// x86/ARM asm, crates/common/crypto/keccak/mod.rs + keccak1600-x86_64.s).
//
// One LANE per message: the 25-lane u64 state lives in VGPRs (~50 VGPRs),
// keccak-f1600 is ~1900 64-bit VALU ops per permutation, and a 4096-lane
// launch already fills a CU's issue; messages are independent so the batch
// shape is embarrassingly parallel.  Original Keccak padding (0x01 ... 0x80),
// rate 136 — Ethereum keccak256, NOT SHA3-256.
//
// Parity: ethrex_amd/keccak.py (pure-Python restatement pinned by the
// canonical vectors keccak256("")=c5d246..., keccak256("abc")=4e0365...);
// GPU tests compare bit-exactly across rate-boundary lengths.
//
// k_keccak_pair / k_wrap_expand (bottom of this file) are fixed-length
// specialisations: the message is built directly in the rate lanes, so they
// need no byte staging.  Parity: ethrex_amd/witness.py wrap_vector.
// Kernels have internal linkage: api_keccak.hip and api_ntt.hip both
// include this header.
// ============================================================================
#pragma once
#include <hip/hip_runtime.h>
#include "gpu_field.h"   // fe4: the packed resident format
#include "gpu_field9.h"  // to_mont9<Fr9T>: the wrap expansion's output form

namespace em {

__device__ __constant__ static const uint64_t KRC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull,
    0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull,
    0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
    0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull,
    0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// rotation offsets r[x][y] (column-major x + 5y, as keccak.py's _ROT)
__device__ __constant__ static const int KROT[25] = {
    0,  36, 3,  41, 18,   // x = 0
    1,  44, 10, 45, 2,    // x = 1
    62, 6,  43, 15, 61,   // x = 2
    28, 55, 25, 21, 56,   // x = 3
    27, 20, 39, 8,  14};  // x = 4

__device__ __forceinline__ uint64_t krotl(uint64_t v, int n) {
    return n == 0 ? v : (v << n) | (v >> (64 - n));
}

__device__ void keccak_f1600(uint64_t a[25]) {
    for (int r = 0; r < 24; r++) {
        uint64_t c[5], d[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++)
            c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++)
            d[x] = c[(x + 4) % 5] ^ krotl(c[(x + 1) % 5], 1);
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) {
                b[y + 5 * ((2 * x + 3 * y) % 5)] =
                    krotl(a[x + 5 * y] ^ d[x], KROT[5 * x + y]);
            }
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++)
                a[x + 5 * y] =
                    b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] &
                                    b[(x + 2) % 5 + 5 * y]);
        a[0] ^= KRC[r];
    }
}

__device__ __forceinline__ uint64_t load_le64(const uint8_t *p) {
    if (((uintptr_t)p & 7) == 0) return *(const uint64_t *)p;
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

// one message per lane; offsets[n] delimits message i = [offs[i], offs[i+1])
static __global__ void __launch_bounds__(256)
k_keccak256_batch(const uint8_t *__restrict__ msgs,
                  const uint64_t *__restrict__ offs, size_t n,
                  uint8_t *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t lo = offs[i], hi = offs[i + 1];
    const uint8_t *p = msgs + lo;
    uint64_t rem = hi - lo;
    uint64_t st[25];
#pragma unroll
    for (int k = 0; k < 25; k++) st[k] = 0;
    while (rem >= 136) {
#pragma unroll
        for (int j = 0; j < 17; j++) st[j] ^= load_le64(p + 8 * j);
        keccak_f1600(st);
        p += 136;
        rem -= 136;
    }
    // final block with the original-Keccak pad10*1 (0x01 ... 0x80)
    uint64_t blk[17];
#pragma unroll
    for (int j = 0; j < 17; j++) blk[j] = 0;
    uint8_t *bb = (uint8_t *)blk;
    for (uint64_t k = 0; k < rem; k++) bb[k] = p[k];
    bb[rem] ^= 0x01;
    bb[135] ^= 0x80;
#pragma unroll
    for (int j = 0; j < 17; j++) st[j] ^= blk[j];
    keccak_f1600(st);
    uint64_t *o = (uint64_t *)(out + 32 * i);
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = st[j];
}

// ---- wrap vector v1 (DESIGN.md "Wrap vector v1"): the witness digests
// expanded on device into the NTT plan's resident fe4m vector ----

// one tree level: out[j] = keccak256(in[2j] || in[2j+1]) for j < len/2; an
// odd last digest is promoted unchanged by the lane j == len/2.  The 64-byte
// message is one rate block: lanes 0..7 data, lane 8 = 0x01 pad, lane 16 =
// the 0x80 closing bit.  Digest buffers are 8-byte aligned (ABI contract).
static __global__ void __launch_bounds__(256)
k_keccak_pair(const uint64_t *__restrict__ in, uint64_t *__restrict__ out,
              size_t len) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t half = len >> 1;
    if (j > half || (j == half && !(len & 1))) return;
    if (j == half) {
#pragma unroll
        for (int k = 0; k < 4; k++) out[4 * j + k] = in[4 * (len - 1) + k];
        return;
    }
    uint64_t st[25];
#pragma unroll
    for (int k = 0; k < 8; k++) st[k] = in[8 * j + k];
    st[8] = 0x01ull;
#pragma unroll
    for (int k = 9; k < 25; k++) st[k] = 0;
    st[16] = 0x8000000000000000ull;
    keccak_f1600(st);
#pragma unroll
    for (int k = 0; k < 4; k++) out[4 * j + k] = st[k];
}

struct wrap_domain {
    uint64_t v[4];  // the 32 domain bytes as little-endian lanes
};

// one lane per block j: the fixed 112-byte message
//   D(32) || R(32) || le64(m) || le64(j) || h_{j mod m}(32)
// is assembled directly in rate lanes 0..13 (lane 14 = 0x01 pad, lane 16 =
// 0x80 closing bit), permuted once, and state lanes 0..15 leave as four
// Fr elements: bytes [32t, 32t+32) read big-endian and taken to the plan's
// resident form exactly as k_fr_from_be does (to_mont9<Fr9T>, R' = 2^261,
// packed 4x64 = fe4m) into out[4j+t].  to_mont9 reduces as it converts: any
// x < 2^256 (~5.3 r) gives (x*R2 + m*r)/2^261 < 1.04 r — norm2p, the
// contract of every stored value; no canonical check, the raw values are
// meant to exceed r.
// j < 2^26 (n <= 2^28, the Fr two-adicity), so j mod m is a 32-bit
// remainder, or j itself when m does not fit 32 bits.
static __global__ void __launch_bounds__(256)
k_wrap_expand(const uint64_t *__restrict__ digests,
              const uint64_t *__restrict__ root, uint64_t m, wrap_domain dom,
              fe4 *__restrict__ out, size_t n) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * j >= n) return;
    size_t idx = m > 0xffffffffull ? j : (size_t)((uint32_t)j % (uint32_t)m);
    const uint64_t *h = digests + 4 * idx;
    uint64_t st[25];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        st[k] = dom.v[k];
        st[4 + k] = root[k];
        st[10 + k] = h[k];
    }
    st[8] = m;
    st[9] = (uint64_t)j;
    st[14] = 0x01ull;
    st[15] = 0;
    st[16] = 0x8000000000000000ull;
#pragma unroll
    for (int k = 17; k < 25; k++) st[k] = 0;
    keccak_f1600(st);
    ulonglong2 *o = (ulonglong2 *)(out + 4 * j);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (4 * j + t < n) {
            u64 raw[4] = {__builtin_bswap64(st[4 * t + 3]),
                          __builtin_bswap64(st[4 * t + 2]),
                          __builtin_bswap64(st[4 * t + 1]),
                          __builtin_bswap64(st[4 * t])};
            u64 e[4];
            fe9_to_u64x4(e, to_mont9<Fr9T>(fe9_from_u64x4(raw)));
            o[2 * t] = make_ulonglong2(e[0], e[1]);
            o[2 * t + 1] = make_ulonglong2(e[2], e[3]);
        }
    }
}

}  // namespace em
