// ============================================================================
// ethrex_mi355 C-ABI implementation — MI355X-native BN254 MSM/NTT core.
//
// See include/ethrex_mi355.h for the boundary contract (mirrors the in-repo
// ZisK accelerator FFI convention, crates/guest-program/src/crypto/zisk.rs:71-137)
// and DESIGN.md for the kernel design.  Threading: the backend is called
// from ONE actor on a blocking thread (crates/prover/src/prover.rs:241-251),
// so plans are not internally locked.
//
// NO CPU FALLBACK: every compute entry point requires a visible GPU and
// returns EM_ERR_HIP otherwise.
// ============================================================================
// api_ntt.hip — radix-2 NTT over BN254 Fr (plan + one-shot).
#include "em_api_common.h"
#include "../../include/ethrex_mi355.h"
#include "ntt_kernels.h"
#include "keccak_kernels.h"   // k_keccak_pair / k_wrap_expand (witness fill)

using namespace em;

// ============================ NTT plan ============================

struct em_ntt_plan {
    size_t n;
    int logn;
    bool fused = false;       // four-step path (13 <= logn <= 24)
    bool fused2 = false;      // two-level four-step (25 <= logn <= 26)
    int logN1 = 0, logN2 = 0;
    int logM1 = 0, logM2 = 0; // inner split of N2 (fused2)
    int cur = 0;              // which buffer holds the data: 0=d_data 1=d_work
    fe4 *d_data = nullptr;    // packed 4x64 Montgomery (fe4m), 32 B/elem
    fe4 *d_work = nullptr;    // fused: transpose ping-pong buffer
    uint8_t *d_bytes = nullptr;
    fe9 *d_tw = nullptr;      // fallback: forward twiddles, n/2
    fe9 *d_tw_inv = nullptr;
    fe4 *d_twfull = nullptr;      // fused: TW2[c][k] = w^(k*c), streamed
    fe4 *d_twfull_inv = nullptr;
    fe9 *d_twrow1 = nullptr;      // fused: N1/2 row twiddles (+inv)
    fe9 *d_twrow1_inv = nullptr;
    fe9 *d_twrow2 = nullptr;      // fused: N2/2 (+inv)
    fe9 *d_twrow2_inv = nullptr;
    fe4 *d_twfull2 = nullptr;     // fused2: inner TW2B[c][k], size N2 (+inv)
    fe4 *d_twfull2_inv = nullptr;
    fe9 *d_twrowA = nullptr;      // fused2: inner M1/2 row twiddles (+inv)
    fe9 *d_twrowA_inv = nullptr;
    fe9 *d_twrowB = nullptr;      // fused2: inner M2/2 (+inv)
    fe9 *d_twrowB_inv = nullptr;
    fe9 *d_ninv = nullptr;        // 1/n (fe9 Montgomery)
    uint32_t *d_err = nullptr;
    hipEvent_t ev[4];
    double last_ms[3] = {0, 0, 0};
    uint64_t *d_tree = nullptr;   // fill_from_digests: two ping-pong halves
    size_t tree_cap = 0;          //   of tree_cap digests each
    hipEvent_t ev_fill[2];
    bool ev_fill_ok = false;
    double last_fill_ms = 0;
};

// build w2k powers on host and launch k_gen_twiddles: tw[j] = w^j, j < count
static int gen_tw_table(fe9 *d_out, size_t count, int bits, bool inverse,
                        int log_size /* transform size 2^log_size */) {
    fe9 w = fe9_load(inverse ? bn254::FR9_W28_INV : bn254::FR9_W28);
    for (int k = bn254::FR_TWO_ADICITY; k > log_size; k--)
        w = mont_sqr9<Fr9T>(w);
    fe9 w2k[32];
    w2k[0] = log_size == 0 ? fe9_load(bn254::FR9_ONE) : w;
    for (int k = 1; k < bits && k < 32; k++) w2k[k] = mont_sqr9<Fr9T>(w2k[k - 1]);
    fe9 *d_w2k;
    HIP_TRY(hipMalloc(&d_w2k, sizeof(w2k)));
    HIP_TRY(hipMemcpy(d_w2k, w2k, sizeof(w2k), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gen_twiddles, dim3(blocks_for(count, 256)), dim3(256),
                       0, 0, d_out, count, d_w2k, bits);
    HIP_TRY(hipDeviceSynchronize());
    hipError_t e2 = hipFree(d_w2k);
    (void)e2;
    return EM_OK;
}

// row-kernel dispatch for the one-level path: default radix-2^3 at 512
// threads; EM_NTT_R4=1 selects the radix-2^2 variant, EM_NTT_TD sets its
// block size (512/768/1024) — A/B occupancy experiment.
static void launch_row(uint32_t nrows, int logM, fe4 *data,
                       const fe9 *tw_row, const fe4 *tw2, const fe9 *scale) {
    size_t lds = (((size_t)1 << logM) + (((size_t)1 << logM) >> 6)) *
                 sizeof(fe9);
    // default: radix-2^2 at 1024 threads (A/B best: 3.28 ms vs 3.38 for
    // the radix-2^3/512 shape at 2^24 — 4 waves/SIMD hides the LDS+mul
    // latency better than fewer round trips at 2 waves).  EM_NTT_R8
    // selects the radix-2^3 variant.
    static int r4 = std::getenv("EM_NTT_R8") ? 0 : 1;
    static int td = std::getenv("EM_NTT_TD") ? atoi(std::getenv("EM_NTT_TD"))
                                             : 1024;
    if (r4) {
        hipLaunchKernelGGL(k_ntt_row4, dim3(nrows), dim3(td), lds, 0, data,
                           logM, tw_row, tw2, scale, 0xffffffffu);
    } else {
        hipLaunchKernelGGL(k_ntt_row, dim3(nrows), dim3(512), lds, 0, data,
                           logM, tw_row, tw2, scale, 0xffffffffu);
    }
}

// reordered streamed table TW2[c*M + k] = w^(k*c) (fe4m), c < rows:
// P1's per-row twiddle read becomes a coalesced stream instead of a
// stride-c gather over an n-sized table (a full cache line per element).
static int gen_tw2_table(fe4 *d_out, uint32_t M, size_t rows, bool inverse,
                         int log_size /* transform size 2^log_size */) {
    fe9 w = fe9_load(inverse ? bn254::FR9_W28_INV : bn254::FR9_W28);
    for (int k = bn254::FR_TWO_ADICITY; k > log_size; k--)
        w = mont_sqr9<Fr9T>(w);
    fe9 w2k[32];
    w2k[0] = log_size == 0 ? fe9_load(bn254::FR9_ONE) : w;
    for (int k = 1; k < log_size && k < 32; k++)
        w2k[k] = mont_sqr9<Fr9T>(w2k[k - 1]);
    fe9 *d_w2k;
    HIP_TRY(hipMalloc(&d_w2k, sizeof(w2k)));
    HIP_TRY(hipMemcpy(d_w2k, w2k, sizeof(w2k), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_gen_tw2, dim3(blocks_for((size_t)M * rows, 256)),
                       dim3(256), 0, 0, d_out, M, rows, d_w2k, log_size);
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(d_w2k);
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_plan_create(size_t n, em_ntt_plan **plan) {
    if (!plan || n == 0 || (n & (n - 1))) return EM_ERR_INPUT;
    int logn = 0;
    while (((size_t)1 << logn) < n) logn++;
    if (logn > bn254::FR_TWO_ADICITY) return EM_ERR_INPUT;
    int rc = require_gpu();
    if (rc) return rc;
    em_ntt_plan *p = new em_ntt_plan();
    p->n = n;
    p->logn = logn;
    // one-level four-step up to 2^24 (A/B-measured best: 3.37 ms vs 3.76
    // for the two-level split at 2^24); two-level only where the row
    // length exceeds the LDS row kernel (2^25/26).  EM_NTT_TWOLEVEL
    // forces the two-level path for measurement.
    p->fused = (logn > 12 && logn <= 24);
    p->fused2 = (logn >= 25 && logn <= 26);
    if (std::getenv("EM_NTT_TWOLEVEL") && logn >= 22 && p->fused) {
        p->fused = false;
        p->fused2 = true;
    }
    size_t half = n > 1 ? n / 2 : 1;
    hipError_t e = hipSuccess;
    auto mal = [&](void **ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(ptr, bytes);
    };
    mal((void **)&p->d_data, n * sizeof(fe4));
    mal((void **)&p->d_bytes, n * 32);
    mal((void **)&p->d_err, 4);
    if (p->fused || p->fused2) {
        if (p->fused) {
            p->logN1 = (logn + 1) / 2;
            p->logN2 = logn / 2;
        } else {
            // two-level: outer P1 rows of 2^logN1 (through the batched
            // small-row kernel when logN1 <= 10, the dynamic-LDS row
            // kernel for 11-12); inner four-step over the 2^logN2 rows.
            // EM_NTT_SPLIT overrides logN1 for A/B measurement.
            p->logN1 = logn >= 25 ? 12 : logn - 16;
            if (const char *e = std::getenv("EM_NTT_SPLIT")) {
                int v = atoi(e);
                if (v >= logn - 16 && v <= 12 && logn - v >= 10)
                    p->logN1 = v;
            }
            p->logN2 = logn - p->logN1;
            p->logM1 = (p->logN2 + 1) / 2;
            p->logM2 = p->logN2 / 2;
        }
        mal((void **)&p->d_work, n * sizeof(fe4));
        mal((void **)&p->d_twfull, n * sizeof(fe4));
        mal((void **)&p->d_twfull_inv, n * sizeof(fe4));
        mal((void **)&p->d_twrow1, ((size_t)1 << (p->logN1 - 1)) * sizeof(fe9));
        mal((void **)&p->d_twrow1_inv, ((size_t)1 << (p->logN1 - 1)) * sizeof(fe9));
        mal((void **)&p->d_twrow2,
            ((size_t)1 << (p->logN2 > 0 ? p->logN2 - 1 : 0)) * sizeof(fe9));
        mal((void **)&p->d_twrow2_inv,
            ((size_t)1 << (p->logN2 > 0 ? p->logN2 - 1 : 0)) * sizeof(fe9));
        mal((void **)&p->d_ninv, sizeof(fe9));
        if (p->fused2) {
            mal((void **)&p->d_twfull2, ((size_t)1 << p->logN2) * sizeof(fe4));
            mal((void **)&p->d_twfull2_inv,
                ((size_t)1 << p->logN2) * sizeof(fe4));
            mal((void **)&p->d_twrowA,
                ((size_t)1 << (p->logM1 - 1)) * sizeof(fe9));
            mal((void **)&p->d_twrowA_inv,
                ((size_t)1 << (p->logM1 - 1)) * sizeof(fe9));
            mal((void **)&p->d_twrowB,
                ((size_t)1 << (p->logM2 - 1)) * sizeof(fe9));
            mal((void **)&p->d_twrowB_inv,
                ((size_t)1 << (p->logM2 - 1)) * sizeof(fe9));
        }
    } else {
        mal((void **)&p->d_tw, half * sizeof(fe9));
        mal((void **)&p->d_tw_inv, half * sizeof(fe9));
    }
    // the 4096-element rows need 146 KiB of dynamic LDS (opt-in above 64K)
    if (e == hipSuccess)
        e = hipFuncSetAttribute(
            (const void *)&k_ntt_row,
            hipFuncAttributeMaxDynamicSharedMemorySize,
            (int)((4096 + 64) * sizeof(fe9)));
    if (e == hipSuccess)
        e = hipFuncSetAttribute(
            (const void *)&k_ntt_row4,
            hipFuncAttributeMaxDynamicSharedMemorySize,
            (int)((4096 + 64) * sizeof(fe9)));
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipEventCreate(&p->ev[i]);
    if (e != hipSuccess) {
        ethrex_mi355_ntt_plan_destroy(p);
        return hip_fail(e, "ntt_plan_create");
    }
    if (p->fused || p->fused2) {
        int rc2;
        uint32_t N1g = 1u << p->logN1;
        if ((rc2 = gen_tw2_table(p->d_twfull, N1g, n / N1g, false, logn)))
            return rc2;
        if ((rc2 = gen_tw2_table(p->d_twfull_inv, N1g, n / N1g, true, logn)))
            return rc2;
        if ((rc2 = gen_tw_table(p->d_twrow1, (size_t)1 << (p->logN1 - 1),
                                p->logN1, false, p->logN1))) return rc2;
        if ((rc2 = gen_tw_table(p->d_twrow1_inv, (size_t)1 << (p->logN1 - 1),
                                p->logN1, true, p->logN1))) return rc2;
        if ((rc2 = gen_tw_table(p->d_twrow2, (size_t)1 << (p->logN2 - 1),
                                p->logN2, false, p->logN2))) return rc2;
        if ((rc2 = gen_tw_table(p->d_twrow2_inv, (size_t)1 << (p->logN2 - 1),
                                p->logN2, true, p->logN2))) return rc2;
        if (p->fused2) {
            size_t n2 = (size_t)1 << p->logN2;
            uint32_t M1g = 1u << p->logM1;
            if ((rc2 = gen_tw2_table(p->d_twfull2, M1g, n2 / M1g, false,
                                     p->logN2))) return rc2;
            if ((rc2 = gen_tw2_table(p->d_twfull2_inv, M1g, n2 / M1g, true,
                                     p->logN2))) return rc2;
            if ((rc2 = gen_tw_table(p->d_twrowA, (size_t)1 << (p->logM1 - 1),
                                    p->logM1, false, p->logM1))) return rc2;
            if ((rc2 = gen_tw_table(p->d_twrowA_inv,
                                    (size_t)1 << (p->logM1 - 1), p->logM1,
                                    true, p->logM1))) return rc2;
            if ((rc2 = gen_tw_table(p->d_twrowB, (size_t)1 << (p->logM2 - 1),
                                    p->logM2, false, p->logM2))) return rc2;
            if ((rc2 = gen_tw_table(p->d_twrowB_inv,
                                    (size_t)1 << (p->logM2 - 1), p->logM2,
                                    true, p->logM2))) return rc2;
        }
        fe9 ninv = fe9_load(bn254::FR9_INV_POW2[logn]);
        HIP_TRY(hipMemcpy(p->d_ninv, &ninv, sizeof(fe9), hipMemcpyHostToDevice));
    } else {
        int rc2;
        if ((rc2 = gen_tw_table(p->d_tw, half, logn ? logn : 1, false, logn)))
            return rc2;
        if ((rc2 = gen_tw_table(p->d_tw_inv, half, logn ? logn : 1, true, logn)))
            return rc2;
    }
    *plan = p;
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_plan_destroy(em_ntt_plan *p) {
    if (!p) return EM_ERR_INPUT;
    (void)hipFree(p->d_data);
    (void)hipFree(p->d_work);
    (void)hipFree(p->d_bytes);
    (void)hipFree(p->d_tw);
    (void)hipFree(p->d_tw_inv);
    (void)hipFree(p->d_twfull);
    (void)hipFree(p->d_twfull2);
    (void)hipFree(p->d_twfull2_inv);
    (void)hipFree(p->d_twrowA);
    (void)hipFree(p->d_twrowA_inv);
    (void)hipFree(p->d_twrowB);
    (void)hipFree(p->d_twrowB_inv);
    (void)hipFree(p->d_twfull_inv);
    (void)hipFree(p->d_twrow1);
    (void)hipFree(p->d_twrow1_inv);
    (void)hipFree(p->d_twrow2);
    (void)hipFree(p->d_twrow2_inv);
    (void)hipFree(p->d_ninv);
    (void)hipFree(p->d_err);
    (void)hipFree(p->d_tree);
    if (p->ev_fill_ok) {
        (void)hipEventDestroy(p->ev_fill[0]);
        (void)hipEventDestroy(p->ev_fill[1]);
    }
    delete p;
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_upload(em_ntt_plan *p, const uint8_t *elems32) {
    if (!p || !elems32) return EM_ERR_INPUT;
    HIP_TRY(hipMemset(p->d_err, 0, 4));
    HIP_TRY(hipMemcpy(p->d_bytes, elems32, p->n * 32, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_fr_from_be, dim3(blocks_for(p->n, 256)), dim3(256), 0, 0,
                       p->d_bytes, p->d_data, p->n, p->d_err);
    p->cur = 0;
    uint32_t err;
    HIP_TRY(hipMemcpy(&err, p->d_err, 4, hipMemcpyDeviceToHost));
    return err ? EM_ERR_INPUT : EM_OK;
}

// wrap vector v1: expand m device-resident keccak digests into
// the plan's n resident elements — pairwise keccak tree to the root R
// (~log2 m launches on ping-pong scratch), then one k_wrap_expand lane per
// four elements writing fe4m straight into d_data.  Nothing crosses PCIe
// but the 32 domain bytes (a kernel argument).
extern "C" int ethrex_mi355_ntt_fill_from_digests(em_ntt_plan *p,
                                                  const void *d_digests32,
                                                  size_t m,
                                                  const uint8_t domain[32]) {
    if (!p || !d_digests32 || !domain || m == 0) return EM_ERR_INPUT;
    size_t cap = (m + 1) / 2;
    if (m > 1 && cap > p->tree_cap) {
        (void)hipFree(p->d_tree);
        p->d_tree = nullptr;
        p->tree_cap = 0;
        HIP_TRY(hipMalloc((void **)&p->d_tree, 2 * cap * 32));
        p->tree_cap = cap;
    }
    if (!p->ev_fill_ok) {
        HIP_TRY(hipEventCreate(&p->ev_fill[0]));
        hipError_t e = hipEventCreate(&p->ev_fill[1]);
        if (e != hipSuccess) {
            (void)hipEventDestroy(p->ev_fill[0]);
            return hip_fail(e, "ntt_fill_from_digests");
        }
        p->ev_fill_ok = true;
    }
    wrap_domain dom;
    memcpy(dom.v, domain, 32);
    HIP_TRY(hipEventRecord(p->ev_fill[0], 0));
    const uint64_t *src = (const uint64_t *)d_digests32;
    int which = 0;
    for (size_t len = m; len > 1; len = (len + 1) / 2) {
        uint64_t *dst = p->d_tree + (which ? p->tree_cap * 4 : 0);
        hipLaunchKernelGGL(k_keccak_pair, dim3(blocks_for((len + 1) / 2, 256)),
                           dim3(256), 0, 0, src, dst, len);
        src = dst;
        which ^= 1;
    }
    hipLaunchKernelGGL(k_wrap_expand, dim3(blocks_for((p->n + 3) / 4, 256)),
                       dim3(256), 0, 0, (const uint64_t *)d_digests32, src,
                       (uint64_t)m, dom, p->d_data, p->n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(p->ev_fill[1], 0));
    HIP_TRY(hipDeviceSynchronize());
    p->cur = 0;
    float ms;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev_fill[0], p->ev_fill[1]));
    p->last_fill_ms = ms;
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_last_fill_ms(em_ntt_plan *p, double *ms) {
    if (!p || !ms) return EM_ERR_INPUT;
    *ms = p->last_fill_ms;
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_run(em_ntt_plan *p, int inverse) {
    if (!p) return EM_ERR_INPUT;
    size_t n = p->n;
    fe4 *cur = p->cur ? p->d_work : p->d_data;
    fe4 *oth = p->cur ? p->d_data : p->d_work;
    HIP_TRY(hipEventRecord(p->ev[0], 0));
    if (p->fused) {
        uint32_t N1 = 1u << p->logN1, N2 = 1u << p->logN2;
        // T0: A[r][c] -> A1[c][r]
        hipLaunchKernelGGL(k_transpose_fe4, dim3(N2 / 32, N1 / 32), dim3(256), 0,
                           0, cur, oth, N1, N2);
        HIP_TRY(hipEventRecord(p->ev[1], 0));
        // P1: row NTT_N1 over each of the N2 rows + w^(k1*c) twiddle
        launch_row(N2, p->logN1,
                   oth, inverse ? p->d_twrow1_inv : p->d_twrow1,
                   inverse ? p->d_twfull_inv : p->d_twfull,
                   (const fe9 *)nullptr);
        // T1
        hipLaunchKernelGGL(k_transpose_fe4, dim3(N1 / 32, N2 / 32), dim3(256), 0,
                           0, oth, cur, N2, N1);
        // P2: row NTT_N2 (+ 1/n scale on iNTT)
        launch_row(N1, p->logN2,
                   cur, inverse ? p->d_twrow2_inv : p->d_twrow2,
                   (const fe4 *)nullptr,
                   inverse ? p->d_ninv : (const fe9 *)nullptr);
        // T2: natural order
        hipLaunchKernelGGL(k_transpose_fe4, dim3(N2 / 32, N1 / 32), dim3(256), 0,
                           0, cur, oth, N1, N2);
        p->cur ^= 1;
    } else if (p->fused2) {
        // two-level four-step (25 <= logn <= 26): the outer P2 row length
        // (2^13/2^14) exceeds the 4096-element LDS row kernel, so each of
        // the N1 outer rows is itself transformed by a BATCHED inner
        // four-step (M1 x M2, both <= 2^7).  The inner transform is
        // natural-in / natural-out, so it composes exactly where the
        // one-level P2 sat.  8 full-array passes instead of logn.
        uint32_t N1 = 1u << p->logN1, N2 = 1u << p->logN2;
        uint32_t M1 = 1u << p->logM1, M2 = 1u << p->logM2;
        const fe9 *tr1 = inverse ? p->d_twrow1_inv : p->d_twrow1;
        const fe4 *tf = inverse ? p->d_twfull_inv : p->d_twfull;
        const fe4 *tf2 = inverse ? p->d_twfull2_inv : p->d_twfull2;
        const fe9 *trA = inverse ? p->d_twrowA_inv : p->d_twrowA;
        const fe9 *trB = inverse ? p->d_twrowB_inv : p->d_twrowB;
        // T0 + P1 + T1: outer column NTTs (length N1) + w_n^(k1 c)
        hipLaunchKernelGGL(k_transpose_fe4, dim3(N2 / 32, N1 / 32), dim3(256),
                           0, 0, cur, oth, N1, N2);
        HIP_TRY(hipEventRecord(p->ev[1], 0));
        if (p->logN1 <= 10) {
            hipLaunchKernelGGL(k_ntt_row_small, dim3(N2 * N1 / 1024),
                               dim3(512), 0, 0, oth, p->logN1, tr1, tf,
                               (const fe9 *)nullptr, 0xffffffffu);
        } else {
            launch_row(N2, p->logN1, oth, tr1, tf, (const fe9 *)nullptr);
        }
        hipLaunchKernelGGL(k_transpose_fe4, dim3(N1 / 32, N2 / 32), dim3(256),
                           0, 0, oth, cur, N2, N1);
        // inner batched four-step over the N1 rows of length N2 = M1*M2
        hipLaunchKernelGGL(k_transpose_fe4, dim3(M2 / 32, M1 / 32, N1),
                           dim3(256), 0, 0, cur, oth, M1, M2);
        hipLaunchKernelGGL(k_ntt_row_small, dim3(N1 * M2 * M1 / 1024),
                           dim3(512), 0, 0, oth, p->logM1, trA, tf2,
                           (const fe9 *)nullptr, M2 - 1);  // (see P1 above)
        hipLaunchKernelGGL(k_transpose_fe4, dim3(M1 / 32, M2 / 32, N1),
                           dim3(256), 0, 0, oth, cur, M2, M1);
        hipLaunchKernelGGL(k_ntt_row_small, dim3(N1 * M1 * M2 / 1024),
                           dim3(512), 0, 0, cur, p->logM2, trB,
                           (const fe4 *)nullptr,
                           inverse ? p->d_ninv : (const fe9 *)nullptr,
                           0xffffffffu);
        hipLaunchKernelGGL(k_transpose_fe4, dim3(M2 / 32, M1 / 32, N1),
                           dim3(256), 0, 0, cur, oth, M1, M2);
        // outer T2 -> natural order
        hipLaunchKernelGGL(k_transpose_fe4, dim3(N2 / 32, N1 / 32), dim3(256),
                           0, 0, oth, cur, N1, N2);
        // data ends in `cur` (8 passes): no buffer flip
    } else {
        if (n > 1) {
            hipLaunchKernelGGL(k_bit_reverse, dim3(blocks_for(n, 256)), dim3(256),
                               0, 0, cur, n, p->logn);
        }
        HIP_TRY(hipEventRecord(p->ev[1], 0));
        const fe9 *tw = inverse ? p->d_tw_inv : p->d_tw;
        for (int s = 1; s <= p->logn; s++) {
            hipLaunchKernelGGL(k_ntt_stage, dim3(blocks_for(n / 2, 256)),
                               dim3(256), 0, 0, cur, tw, n, p->logn, s);
        }
        if (inverse) {
            hipLaunchKernelGGL(k_ntt_scale, dim3(blocks_for(n, 256)), dim3(256),
                               0, 0, cur, n, p->logn);
        }
    }
    HIP_TRY(hipEventRecord(p->ev[2], 0));
    HIP_TRY(hipDeviceSynchronize());
    float ms;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
    p->last_ms[0] = ms;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev[1], p->ev[2]));
    p->last_ms[1] = ms;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[2]));
    p->last_ms[2] = ms;
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_download(em_ntt_plan *p, uint8_t *elems32) {
    if (!p || !elems32) return EM_ERR_INPUT;
    fe4 *cur = p->cur ? p->d_work : p->d_data;
    hipLaunchKernelGGL(k_fr_to_be, dim3(blocks_for(p->n, 256)), dim3(256), 0, 0,
                       cur, p->d_bytes, p->n);
    HIP_TRY(hipMemcpy(elems32, p->d_bytes, p->n * 32, hipMemcpyDeviceToHost));
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_last_times(em_ntt_plan *p, double times_ms[3]) {
    if (!p || !times_ms) return EM_ERR_INPUT;
    memcpy(times_ms, p->last_ms, sizeof p->last_ms);
    return EM_OK;
}

// ============================ one-shot NTT ============================

extern "C" int ethrex_mi355_bn254_fr_ntt(uint8_t *elems32, size_t n, int inverse) {
    if (!elems32 || n == 0) return EM_ERR_INPUT;
    em_ntt_plan *p = nullptr;
    int rc = ethrex_mi355_ntt_plan_create(n, &p);
    if (rc) return rc;
    rc = ethrex_mi355_ntt_upload(p, elems32);
    if (!rc) rc = ethrex_mi355_ntt_run(p, inverse);
    if (!rc) rc = ethrex_mi355_ntt_download(p, elems32);
    ethrex_mi355_ntt_plan_destroy(p);
    return rc;
}

// device pointer to the CURRENT data buffer (packed fe4m Montgomery) — the
// wrap-pipeline handoff: the MSM plan converts these in place on device
// (ethrex_mi355_msm_scalars_from_ntt), no PCIe round trip (sp1.rs:122-134
// wrap flow: the witness NTT output feeds the proving MSM).
extern "C" int ethrex_mi355_ntt_device_data(em_ntt_plan *p, const void **ptr,
                                            size_t *n) {
    if (!p || !ptr) return EM_ERR_INPUT;
    *ptr = p->cur ? p->d_work : p->d_data;
    if (n) *n = p->n;
    return EM_OK;
}
