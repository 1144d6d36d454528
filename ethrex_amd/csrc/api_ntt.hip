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
#include "r1cs_kernels.h"     // sparse A z / B z / C z
#include "r1cs_pack.h"        // host CSR validation + packing

#include <vector>

using namespace em;

// ============================ NTT plan ============================

// transform shape + twiddle set of one size: everything a transform needs
// except the data buffers.  Shared by em_ntt_plan (one vector) and
// em_quot_plan (three vectors over one twiddle set).
struct ntt_tw {
    size_t n = 0;
    int logn = 0;
    bool fused = false;       // four-step path (13 <= logn <= 24)
    bool fused2 = false;      // two-level four-step (25 <= logn <= 26)
    int logN1 = 0, logN2 = 0;
    int logM1 = 0, logM2 = 0; // inner split of N2 (fused2)
    // the direction-dependent tables: dir[0] forward, dir[1] inverse
    struct dir_tw {
        fe9 *tw = nullptr;    // fallback: stage twiddles, n/2
        fe4 *full = nullptr;  // fused: TW2[c][k] = w^(k*c), streamed
        fe9 *row1 = nullptr;  // fused: N1/2 row twiddles
        fe9 *row2 = nullptr;  // fused: N2/2
        fe4 *full2 = nullptr; // fused2: inner TW2B[c][k], size N2
        fe9 *rowA = nullptr;  // fused2: inner M1/2 row twiddles
        fe9 *rowB = nullptr;  // fused2: inner M2/2
    } dir[2];
    fe9 *d_ninv = nullptr;        // 1/n (fe9 Montgomery)
    // coset tables (built on first coset use, ntt_tw_coset_init).  Index
    // split i = hi * 2^lo_bits + lo with cs_logA high bits / cs_logB low
    // bits forward and the reverse inverse — (logN1, logN2) on the
    // four-step path, so the row kernels can use them per row / element:
    //   cs_f_hi[r] = (g^(2^logB))^r      2^logA entries
    //   cs_f_lo[c] = g^c                 2^logB entries
    //   cs_i_hi[k2] = (g^-(2^logA))^k2   2^logB entries
    //   cs_i_lo[k1] = g^-k1 / n          2^logA entries
    bool coset_ok = false;
    int cs_logA = 0, cs_logB = 0;
    fe9 *cs_f_hi = nullptr, *cs_f_lo = nullptr;
    fe9 *cs_i_hi = nullptr, *cs_i_lo = nullptr;
};

struct em_ntt_plan : ntt_tw {
    int cur = 0;              // which buffer holds the data: 0=d_data 1=d_work
    fe4 *d_data = nullptr;    // packed 4x64 Montgomery (fe4m), 32 B/elem
    fe4 *d_work = nullptr;    // fused: transpose ping-pong buffer
    uint8_t *d_bytes = nullptr;
    uint32_t *d_err = nullptr;
    hipEvent_t ev[4];
    double last_ms[3] = {0, 0, 0};
    uint64_t *d_tree = nullptr;   // fill_from_digests: two ping-pong halves
    size_t tree_cap = 0;          //   of tree_cap digests each
    hipEvent_t ev_fill[2];
    bool ev_fill_ok = false;
    double last_fill_ms = 0;
};

// ---- table generation ----

static fe9 sqr_times(fe9 x, int k) {
    for (int i = 0; i < k; i++) x = mont_sqr9<Fr9T>(x);
    return x;
}

// the 2^log_size-th root of unity of that direction (Montgomery)
static fe9 root_of_unity(int log_size, bool inverse) {
    return sqr_times(fe9_load(inverse ? bn254::FR9_W28_INV : bn254::FR9_W28),
                     bn254::FR_TWO_ADICITY - log_size);
}

// the generators' square ladder: b2k[k] = base^(2^k), k < LADDER_BITS
constexpr int LADDER_BITS = 32;
static void ladder_fill(fe9 b2k[LADDER_BITS], fe9 base) {
    b2k[0] = base;
    for (int k = 1; k < LADDER_BITS; k++) b2k[k] = mont_sqr9<Fr9T>(b2k[k - 1]);
}

// one device scratch buffer for the ladder per ntt_tw_create /
// ntt_tw_coset_init call, freed on every exit path.  set() and the generator
// launches are all on the null stream, so a ladder is not overwritten
// before the launch reading it has run.
struct gen_ladder {
    fe9 *d = nullptr;
    ~gen_ladder() { (void)hipFree(d); }
    int set(fe9 base) {
        fe9 b2k[LADDER_BITS];
        ladder_fill(b2k, base);
        if (!d) HIP_TRY(hipMalloc((void **)&d, sizeof(b2k)));
        HIP_TRY(hipMemcpy(d, b2k, sizeof(b2k), hipMemcpyHostToDevice));
        return EM_OK;
    }
};

// *out (allocated here unless it already is) [j] = s * base^j, j < count
static int gen_pow_table(gen_ladder &L, fe9 **out, size_t count, fe9 base,
                         fe9 s) {
    if (!*out) HIP_TRY(hipMalloc((void **)out, count * sizeof(fe9)));
    int rc = L.set(base);
    if (rc) return rc;
    hipLaunchKernelGGL(k_gen_pow, dim3(blocks_for(count, 256)), dim3(256), 0,
                       0, *out, count, L.d, LADDER_BITS, s);
    return EM_OK;
}

// row twiddles of a 2^log_size transform: (*out)[j] = w^j, j < 2^(log_size-1)
static int gen_row_table(gen_ladder &L, fe9 **out, int log_size, bool inverse) {
    return gen_pow_table(L, out, (size_t)1 << (log_size > 0 ? log_size - 1 : 0),
                         root_of_unity(log_size, inverse),
                         fe9_load(bn254::FR9_ONE));
}

// reordered streamed table TW2[c*M + k] = w^(k*c) (fe4m), c < rows, of a
// 2^log_size = M*rows transform: P1's per-row twiddle read becomes a
// coalesced stream instead of a stride-c gather over an n-sized table (a
// full cache line per element).
static int gen_tw2_table(gen_ladder &L, fe4 **out, uint32_t M, size_t rows,
                         int log_size, bool inverse) {
    if (!*out) HIP_TRY(hipMalloc((void **)out, (size_t)M * rows * sizeof(fe4)));
    int rc = L.set(root_of_unity(log_size, inverse));
    if (rc) return rc;
    hipLaunchKernelGGL(k_gen_tw2, dim3(blocks_for((size_t)M * rows, 256)),
                       dim3(256), 0, 0, *out, M, rows, L.d, log_size);
    return EM_OK;
}

// the coset generator g = 5 (Montgomery), the multiplicative generator of
// Fr that gnark-crypto and arkworks use for BN254
static fe9 coset_gen() {
    fe9 five = fe9_zero();
    five.v[0] = 5;
    return to_mont9<Fr9T>(five);
}

// ---- row-kernel dispatch ----
// Default: radix-2^2 at 1024 threads (A/B best: 3.28 ms vs 3.38 for the
// radix-2^3/512 shape at 2^24 — 4 waves/SIMD hides the LDS+mul latency
// better than fewer round trips at 2 waves).  EM_NTT_R8 selects the
// radix-2^3 kernels at 512 threads; EM_NTT_TD sets the radix-2^2 block
// size (an A/B knob, not validated).  Both are read once per process.
struct row_cfg {
    bool r8;
    int td;
};
static const row_cfg &row_config() {
    static const row_cfg c = {
        std::getenv("EM_NTT_R8") != nullptr,
        std::getenv("EM_NTT_TD") ? atoi(std::getenv("EM_NTT_TD")) : 1024};
    return c;
}

// skewed LDS row of 2^logM elements: M + M/64 fe9 slots
static size_t row_lds_bytes(int logM) {
    size_t M = (size_t)1 << logM;
    return (M + (M >> 6)) * sizeof(fe9);
}

// the 4096-element rows need 146 KiB of dynamic LDS (opt-in above 64K);
// applied once (per device, and a process uses one)
static int row_lds_opt_in() {
    static const void *const kernels[] = {
        (const void *)&k_ntt_row,          (const void *)&k_ntt_row4,
        (const void *)&k_ntt_row_coset<1>, (const void *)&k_ntt_row_coset<2>,
        (const void *)&k_ntt_row4_coset<1>, (const void *)&k_ntt_row4_coset<2>};
    static int done_dev = -1;
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    if (dev == done_dev) return EM_OK;
    for (const void *k : kernels)
        HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)row_lds_bytes(12)));
    done_dev = dev;
    return EM_OK;
}

// one row pass: nrows blocks, one 2^logM row each.  COSET = 0: plain
// (scale may be null); 1: P1 of the coset forward transform, 2: P2 of the
// coset inverse (cs_elem / cs_row, see ntt_kernels.h).
template <int COSET>
static void launch_row(uint32_t nrows, int logM, fe4 *data, const fe9 *tw_row,
                       const fe4 *tw2, const fe9 *scale,
                       const fe9 *cs_elem = nullptr,
                       const fe9 *cs_row = nullptr) {
    const row_cfg &c = row_config();
    const dim3 grid(nrows), block(c.r8 ? 512 : c.td);
    const size_t lds = row_lds_bytes(logM);
    if constexpr (COSET == 0) {
        hipLaunchKernelGGL(c.r8 ? k_ntt_row : k_ntt_row4, grid, block, lds, 0,
                           data, logM, tw_row, tw2, scale, 0xffffffffu);
    } else {
        hipLaunchKernelGGL(c.r8 ? k_ntt_row_coset<COSET>
                                : k_ntt_row4_coset<COSET>,
                           grid, block, lds, 0, data, logM, tw_row, tw2,
                           cs_elem, cs_row);
    }
}

// ---- twiddle set ----

// n a power of two <= 2^28 (checked by the callers); on failure the
// caller frees what was allocated (ntt_tw_free)
static int ntt_tw_create(ntt_tw *p, size_t n) {
    int logn = 0;
    while (((size_t)1 << logn) < n) logn++;
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
    if (p->fused) {
        p->logN1 = (logn + 1) / 2;
        p->logN2 = logn / 2;
    } else if (p->fused2) {
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
    int rc = row_lds_opt_in();
    if (rc) return rc;
    gen_ladder L;
    for (int inv = 0; inv < 2; inv++) {
        ntt_tw::dir_tw &d = p->dir[inv];
        if (!p->fused && !p->fused2) {
            if ((rc = gen_row_table(L, &d.tw, logn, inv))) return rc;
            continue;
        }
        uint32_t N1 = 1u << p->logN1;
        if ((rc = gen_tw2_table(L, &d.full, N1, n / N1, logn, inv))) return rc;
        if ((rc = gen_row_table(L, &d.row1, p->logN1, inv))) return rc;
        if ((rc = gen_row_table(L, &d.row2, p->logN2, inv))) return rc;
        if (!p->fused2) continue;
        uint32_t M1 = 1u << p->logM1;
        if ((rc = gen_tw2_table(L, &d.full2, M1, ((size_t)1 << p->logN2) / M1,
                                p->logN2, inv))) return rc;
        if ((rc = gen_row_table(L, &d.rowA, p->logM1, inv))) return rc;
        if ((rc = gen_row_table(L, &d.rowB, p->logM2, inv))) return rc;
    }
    if (p->fused || p->fused2) {
        fe9 ninv = fe9_load(bn254::FR9_INV_POW2[logn]);
        HIP_TRY(hipMalloc((void **)&p->d_ninv, sizeof(fe9)));
        HIP_TRY(hipMemcpy(p->d_ninv, &ninv, sizeof(fe9), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return EM_OK;
}

// coset tables, on first coset use
static int ntt_tw_coset_init(ntt_tw *p) {
    if (p->coset_ok) return EM_OK;
    if (p->fused) {
        p->cs_logA = p->logN1;
        p->cs_logB = p->logN2;
    } else {
        p->cs_logA = (p->logn + 1) / 2;
        p->cs_logB = p->logn / 2;
    }
    size_t nA = (size_t)1 << p->cs_logA, nB = (size_t)1 << p->cs_logB;
    fe9 one = fe9_load(bn254::FR9_ONE);
    fe9 g = coset_gen();
    fe9 ginv = mont_inv9<Fr9T>(g);
    fe9 ninv = fe9_load(bn254::FR9_INV_POW2[p->logn]);
    gen_ladder L;
    int rc;
    if ((rc = gen_pow_table(L, &p->cs_f_hi, nA, sqr_times(g, p->cs_logB), one)))
        return rc;
    if ((rc = gen_pow_table(L, &p->cs_f_lo, nB, g, one))) return rc;
    if ((rc = gen_pow_table(L, &p->cs_i_hi, nB, sqr_times(ginv, p->cs_logA),
                            one))) return rc;
    if ((rc = gen_pow_table(L, &p->cs_i_lo, nA, ginv, ninv))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    p->coset_ok = true;
    return EM_OK;
}

static bool ntt_size_ok(size_t n) {
    return n != 0 && !(n & (n - 1)) &&
           n <= ((size_t)1 << bn254::FR_TWO_ADICITY);
}

extern "C" int ethrex_mi355_ntt_plan_create(size_t n, em_ntt_plan **plan) {
    if (!plan || !ntt_size_ok(n)) return EM_ERR_INPUT;
    int rc = require_gpu();
    if (rc) return rc;
    em_ntt_plan *p = new em_ntt_plan();
    rc = ntt_tw_create(p, n);
    hipError_t e = hipSuccess;
    auto mal = [&](void **ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(ptr, bytes);
    };
    if (!rc) {
        mal((void **)&p->d_data, n * sizeof(fe4));
        mal((void **)&p->d_bytes, n * 32);
        mal((void **)&p->d_err, 4);
        if (p->fused || p->fused2) mal((void **)&p->d_work, n * sizeof(fe4));
        for (int i = 0; i < 4 && e == hipSuccess; i++)
            e = hipEventCreate(&p->ev[i]);
        if (e != hipSuccess) rc = hip_fail(e, "ntt_plan_create");
    }
    if (rc) {
        ethrex_mi355_ntt_plan_destroy(p);
        return rc;
    }
    *plan = p;
    return EM_OK;
}

static void ntt_tw_free(ntt_tw *p) {
    for (fe9 *t : {p->cs_f_hi, p->cs_f_lo, p->cs_i_hi, p->cs_i_lo, p->d_ninv})
        (void)hipFree(t);
    for (ntt_tw::dir_tw &d : p->dir)
        for (void *t : {(void *)d.tw, (void *)d.full, (void *)d.row1,
                        (void *)d.row2, (void *)d.full2, (void *)d.rowA,
                        (void *)d.rowB})
            (void)hipFree(t);
}

extern "C" int ethrex_mi355_ntt_plan_destroy(em_ntt_plan *p) {
    if (!p) return EM_ERR_INPUT;
    ntt_tw_free(p);
    (void)hipFree(p->d_data);
    (void)hipFree(p->d_work);
    (void)hipFree(p->d_bytes);
    (void)hipFree(p->d_err);
    (void)hipFree(p->d_tree);
    if (p->ev_fill_ok) {
        (void)hipEventDestroy(p->ev_fill[0]);
        (void)hipEventDestroy(p->ev_fill[1]);
    }
    delete p;
    return EM_OK;
}

// n canonical big-endian elements -> fe4m in d_out, through the n*32-byte
// device staging area d_stage; EM_ERR_INPUT if an element is >= r
static int fr_upload_be(const uint8_t *elems32, size_t n, uint8_t *d_stage,
                        fe4 *d_out, uint32_t *d_err) {
    HIP_TRY(hipMemset(d_err, 0, 4));
    HIP_TRY(hipMemcpy(d_stage, elems32, n * 32, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_fr_from_be, dim3(blocks_for(n, 256)), dim3(256), 0, 0,
                       d_stage, d_out, n, d_err);
    uint32_t err;
    HIP_TRY(hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost));
    return err ? EM_ERR_INPUT : EM_OK;
}

// the reverse: n fe4m elements of d_in -> big-endian bytes on the host
static int fr_download_be(uint8_t *elems32, size_t n, const fe4 *d_in,
                          uint8_t *d_stage) {
    hipLaunchKernelGGL(k_fr_to_be, dim3(blocks_for(n, 256)), dim3(256), 0, 0,
                       d_in, d_stage, n);
    HIP_TRY(hipMemcpy(elems32, d_stage, n * 32, hipMemcpyDeviceToHost));
    return EM_OK;
}

extern "C" int ethrex_mi355_ntt_upload(em_ntt_plan *p, const uint8_t *elems32) {
    if (!p || !elems32) return EM_ERR_INPUT;
    p->cur = 0;
    return fr_upload_be(elems32, p->n, p->d_bytes, p->d_data, p->d_err);
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

// Enqueue one transform of `cur` on the null stream (no sync).  `oth` is
// the transpose ping-pong buffer of the four-step paths (unused, may be
// null, on the stage-by-stage path); *flipped tells whether the result is
// in `oth`.  ev_mid, when given, is recorded after the first pass (the
// [0]/[1] split of ntt_last_times).  coset: 0 plain; 1 the coset transform
// of that direction — fused into P1 (forward) / P2 (inverse) on the
// four-step path, the standalone k_coset_scale pass elsewhere and under
// EM_NTT_COSET_UNFUSED.  The coset inverse takes its 1/n from the coset
// tables, so the transform's own 1/n is skipped.  With coset = 0 the launch
// sequence is what ethrex_mi355_ntt_run has always issued.
static int ntt_exec(const ntt_tw *p, fe4 *cur, fe4 *oth, int inverse,
                    int coset, hipEvent_t *ev_mid, bool *flipped) {
    size_t n = p->n;
    static int unfused = std::getenv("EM_NTT_COSET_UNFUSED") ? 1 : 0;
    const bool cs_fused = coset && p->fused && !unfused;
    const bool cs_pass = coset && !cs_fused;   // standalone scale pass
    const fe9 *ninv = (inverse && !coset) ? p->d_ninv : (const fe9 *)nullptr;
    const ntt_tw::dir_tw &d = p->dir[inverse ? 1 : 0];
    // four-step shape: n = N1 * N2, and N2 = M1 * M2 on the two-level path
    const uint32_t N1 = 1u << p->logN1, N2 = 1u << p->logN2;
    const uint32_t M1 = 1u << p->logM1, M2 = 1u << p->logM2;
    // `batch` R x C matrices src -> their transposes dst
    auto transpose = [](const fe4 *src, fe4 *dst, uint32_t R, uint32_t C,
                        uint32_t batch) {
        hipLaunchKernelGGL(k_transpose_fe4, dim3(C / 32, R / 32, batch),
                           dim3(256), 0, 0, src, dst, R, C);
    };
    // `total` elements as packed 2^logM rows, 1024 elements per block
    auto row_small = [](size_t total, int logM, fe4 *data, const fe9 *tw_row,
                        const fe4 *tw2, const fe9 *scale, uint32_t cmask) {
        hipLaunchKernelGGL(k_ntt_row_small, dim3((uint32_t)(total / 1024)),
                           dim3(512), 0, 0, data, logM, tw_row, tw2, scale,
                           cmask);
    };
    *flipped = false;
    if (cs_pass && !inverse)
        hipLaunchKernelGGL(k_coset_scale, dim3(blocks_for(n, 256)), dim3(256),
                           0, 0, cur, n, p->cs_f_hi, p->cs_f_lo, p->cs_logB);
    if (p->fused || p->fused2) {
        // T0: A[r][c] -> A1[c][r]
        transpose(cur, oth, N1, N2, 1);
        if (ev_mid) HIP_TRY(hipEventRecord(*ev_mid, 0));
        // P1: row NTT_N1 over each of the N2 rows + w^(k1*c) twiddle
        if (cs_fused && !inverse)
            launch_row<1>(N2, p->logN1, oth, d.row1, d.full, nullptr,
                          p->cs_f_hi, p->cs_f_lo);
        else if (p->fused2 && p->logN1 <= 10)
            row_small(n, p->logN1, oth, d.row1, d.full, nullptr,
                      0xffffffffu);
        else
            launch_row<0>(N2, p->logN1, oth, d.row1, d.full, nullptr);
        // T1
        transpose(oth, cur, N2, N1, 1);
    }
    if (p->fused) {
        // P2: row NTT_N2 (+ 1/n scale on iNTT)
        if (cs_fused && inverse)
            launch_row<2>(N1, p->logN2, cur, d.row2, nullptr, nullptr,
                          p->cs_i_hi, p->cs_i_lo);
        else
            launch_row<0>(N1, p->logN2, cur, d.row2, nullptr, ninv);
        // T2: natural order
        transpose(cur, oth, N1, N2, 1);
        *flipped = true;
    } else if (p->fused2) {
        // two-level four-step (25 <= logn <= 26): the outer P2 row length
        // (2^13/2^14) exceeds the 4096-element LDS row kernel, so each of
        // the N1 outer rows is itself transformed by a BATCHED inner
        // four-step (M1 x M2, both <= 2^7).  The inner transform is
        // natural-in / natural-out, so it composes exactly where the
        // one-level P2 sat.  8 full-array passes instead of logn.
        transpose(cur, oth, M1, M2, N1);
        row_small(n, p->logM1, oth, d.rowA, d.full2, nullptr, M2 - 1);
        transpose(oth, cur, M2, M1, N1);
        row_small(n, p->logM2, cur, d.rowB, nullptr, ninv, 0xffffffffu);
        transpose(cur, oth, M1, M2, N1);
        // outer T2 -> natural order
        transpose(oth, cur, N1, N2, 1);
        // data ends in `cur` (8 passes): no buffer flip
    } else {
        if (n > 1) {
            hipLaunchKernelGGL(k_bit_reverse, dim3(blocks_for(n, 256)), dim3(256),
                               0, 0, cur, n, p->logn);
        }
        if (ev_mid) HIP_TRY(hipEventRecord(*ev_mid, 0));
        for (int s = 1; s <= p->logn; s++) {
            hipLaunchKernelGGL(k_ntt_stage, dim3(blocks_for(n / 2, 256)),
                               dim3(256), 0, 0, cur, d.tw, n, p->logn, s);
        }
        if (inverse && !coset) {
            hipLaunchKernelGGL(k_ntt_scale, dim3(blocks_for(n, 256)), dim3(256),
                               0, 0, cur, n, p->logn);
        }
    }
    if (cs_pass && inverse)
        hipLaunchKernelGGL(k_coset_scale, dim3(blocks_for(n, 256)), dim3(256),
                           0, 0, *flipped ? oth : cur, n, p->cs_i_hi,
                           p->cs_i_lo, p->cs_logA);
    return EM_OK;
}

static int ntt_plan_run(em_ntt_plan *p, int inverse, int coset) {
    fe4 *cur = p->cur ? p->d_work : p->d_data;
    fe4 *oth = p->cur ? p->d_data : p->d_work;
    HIP_TRY(hipEventRecord(p->ev[0], 0));
    bool flipped;
    int rc = ntt_exec(p, cur, oth, inverse, coset, &p->ev[1], &flipped);
    if (rc) return rc;
    if (flipped) p->cur ^= 1;
    HIP_TRY(hipEventRecord(p->ev[2], 0));
    HIP_TRY(hipGetLastError());   // a launch the runtime refused
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

extern "C" int ethrex_mi355_ntt_run(em_ntt_plan *p, int inverse) {
    if (!p) return EM_ERR_INPUT;
    return ntt_plan_run(p, inverse, 0);
}

// coset transform (g = 5): forward = NTT of a_i g^i, inverse = iNTT then
// g^-i; same buffer rules as ntt_run
extern "C" int ethrex_mi355_ntt_run_coset(em_ntt_plan *p, int inverse) {
    if (!p) return EM_ERR_INPUT;
    int rc = ntt_tw_coset_init(p);
    if (rc) return rc;
    return ntt_plan_run(p, inverse, 1);
}

extern "C" int ethrex_mi355_ntt_download(em_ntt_plan *p, uint8_t *elems32) {
    if (!p || !elems32) return EM_ERR_INPUT;
    return fr_download_be(elems32, p->n, p->cur ? p->d_work : p->d_data,
                          p->d_bytes);
}

extern "C" int ethrex_mi355_ntt_last_times(em_ntt_plan *p, double times_ms[3]) {
    if (!p || !times_ms) return EM_ERR_INPUT;
    memcpy(times_ms, p->last_ms, sizeof p->last_ms);
    return EM_OK;
}

// ============================ one-shot NTT ============================

static int ntt_oneshot(uint8_t *elems32, size_t n, int inverse, int coset) {
    if (!elems32 || n == 0) return EM_ERR_INPUT;
    em_ntt_plan *p = nullptr;
    int rc = ethrex_mi355_ntt_plan_create(n, &p);
    if (rc) return rc;
    rc = ethrex_mi355_ntt_upload(p, elems32);
    if (!rc)
        rc = coset ? ethrex_mi355_ntt_run_coset(p, inverse)
                   : ethrex_mi355_ntt_run(p, inverse);
    if (!rc) rc = ethrex_mi355_ntt_download(p, elems32);
    ethrex_mi355_ntt_plan_destroy(p);
    return rc;
}

extern "C" int ethrex_mi355_bn254_fr_ntt(uint8_t *elems32, size_t n, int inverse) {
    return ntt_oneshot(elems32, n, inverse, 0);
}

extern "C" int ethrex_mi355_bn254_fr_coset_ntt(uint8_t *elems32, size_t n,
                                               int inverse) {
    return ntt_oneshot(elems32, n, inverse, 1);
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

// ===================== quotient polynomial (Groth16 H) =====================
// h = coset_inv((coset_fwd(intt(a)) . coset_fwd(intt(b)) - coset_fwd(intt(c)))
//               * (g^n - 1)^-1)   (DESIGN.md "Quotient polynomial").
// One twiddle set, three resident vectors and one work buffer: the four
// buffers rotate — a four-step transform leaves its result in the work
// buffer, which then becomes that slot, and the slot's old buffer becomes
// the work buffer.  The work buffer doubles as the byte staging area of
// upload/download (n * 32 bytes either way).

struct em_quot_plan {
    ntt_tw tw;
    fe4 *buf[4] = {nullptr, nullptr, nullptr, nullptr};
    int slot[3] = {0, 1, 2};  // buf index of a, b, c
    int work = 3;             // buf index of the work buffer
    bool loaded[3] = {false, false, false};
    bool has_h = false;       // h sits in slot a
    uint32_t *d_err = nullptr;
    fe9 dconst;               // (g^n - 1)^-1, Montgomery
    hipEvent_t ev[5];
    int n_ev = 0;
    double last_ms[5] = {0, 0, 0, 0, 0};
};

extern "C" int ethrex_mi355_quot_plan_create(size_t n, em_quot_plan **plan) {
    if (!plan || !ntt_size_ok(n)) return EM_ERR_INPUT;
    int rc = require_gpu();
    if (rc) return rc;
    em_quot_plan *q = new em_quot_plan();
    rc = ntt_tw_create(&q->tw, n);
    if (!rc) rc = ntt_tw_coset_init(&q->tw);
    if (!rc) {
        hipError_t e = hipSuccess;
        for (int i = 0; i < 4 && e == hipSuccess; i++)
            e = hipMalloc((void **)&q->buf[i], n * sizeof(fe4));
        if (e == hipSuccess) e = hipMalloc((void **)&q->d_err, 4);
        for (; q->n_ev < 5 && e == hipSuccess; q->n_ev++)
            e = hipEventCreate(&q->ev[q->n_ev]);
        if (e != hipSuccess) {
            if (q->n_ev) q->n_ev--;   // the failed slot holds no event
            rc = hip_fail(e, "quot_plan_create");
        }
    }
    if (rc) {
        ethrex_mi355_quot_plan_destroy(q);
        return rc;
    }
    // d = (g^n - 1)^-1; g^n != 1 for every n <= 2^28 (g generates Fr*)
    fe9 gn = sqr_times(coset_gen(), q->tw.logn);
    q->dconst = mont_inv9<Fr9T>(subn9<Fr9T>(gn, fe9_load(bn254::FR9_ONE)));
    *plan = q;
    return EM_OK;
}

extern "C" int ethrex_mi355_quot_plan_destroy(em_quot_plan *q) {
    if (!q) return EM_ERR_INPUT;
    ntt_tw_free(&q->tw);
    for (int i = 0; i < 4; i++) (void)hipFree(q->buf[i]);
    (void)hipFree(q->d_err);
    for (int i = 0; i < q->n_ev; i++) (void)hipEventDestroy(q->ev[i]);
    delete q;
    return EM_OK;
}

extern "C" int ethrex_mi355_quot_upload(em_quot_plan *q, int which,
                                        const uint8_t *elems32) {
    if (!q || !elems32 || which < 0 || which > 2) return EM_ERR_INPUT;
    q->loaded[which] = false;
    if (which == 0) q->has_h = false;
    int rc = fr_upload_be(elems32, q->tw.n, (uint8_t *)q->buf[q->work],
                          q->buf[q->slot[which]], q->d_err);
    if (rc) return rc;
    q->loaded[which] = true;
    return EM_OK;
}

extern "C" int ethrex_mi355_quot_load_device(em_quot_plan *q, int which,
                                             const void *d_fe4m) {
    if (!q || !d_fe4m || which < 0 || which > 2) return EM_ERR_INPUT;
    q->loaded[which] = false;
    if (which == 0) q->has_h = false;
    HIP_TRY(hipMemcpy(q->buf[q->slot[which]], d_fe4m,
                      q->tw.n * sizeof(fe4), hipMemcpyDeviceToDevice));
    q->loaded[which] = true;
    return EM_OK;
}

// c = a (.) b; needs a and b loaded
extern "C" int ethrex_mi355_quot_mul_ab_into_c(em_quot_plan *q) {
    if (!q || !q->loaded[0] || !q->loaded[1]) return EM_ERR_INPUT;
    size_t n = q->tw.n;
    hipLaunchKernelGGL(k_fr_mul, dim3(blocks_for(n, 256)), dim3(256), 0, 0,
                       q->buf[q->slot[0]], q->buf[q->slot[1]],
                       q->buf[q->slot[2]], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    q->loaded[2] = true;
    return EM_OK;
}

// one transform of slot `which`, rotating the buffers if it flipped
static int quot_exec(em_quot_plan *q, int which, int inverse, int coset) {
    bool flipped;
    int rc = ntt_exec(&q->tw, q->buf[q->slot[which]], q->buf[q->work],
                      inverse, coset, nullptr, &flipped);
    if (rc) return rc;
    if (flipped) {
        int t = q->slot[which];
        q->slot[which] = q->work;
        q->work = t;
    }
    return EM_OK;
}

extern "C" int ethrex_mi355_quot_run(em_quot_plan *q) {
    if (!q || !q->loaded[0] || !q->loaded[1] || !q->loaded[2])
        return EM_ERR_INPUT;
    size_t n = q->tw.n;
    int rc;
    q->loaded[0] = q->loaded[1] = q->loaded[2] = false;
    q->has_h = false;
    HIP_TRY(hipEventRecord(q->ev[0], 0));
    for (int v = 0; v < 3; v++)
        if ((rc = quot_exec(q, v, 1, 0))) return rc;
    HIP_TRY(hipEventRecord(q->ev[1], 0));
    for (int v = 0; v < 3; v++)
        if ((rc = quot_exec(q, v, 0, 1))) return rc;
    HIP_TRY(hipEventRecord(q->ev[2], 0));
    hipLaunchKernelGGL(k_quot_pointwise, dim3(blocks_for(n, 256)), dim3(256),
                       0, 0, q->buf[q->slot[0]], q->buf[q->slot[1]],
                       q->buf[q->slot[2]], n, q->dconst);
    HIP_TRY(hipEventRecord(q->ev[3], 0));
    if ((rc = quot_exec(q, 0, 1, 1))) return rc;
    HIP_TRY(hipEventRecord(q->ev[4], 0));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    float ms;
    for (int i = 0; i < 4; i++) {
        HIP_TRY(hipEventElapsedTime(&ms, q->ev[i], q->ev[i + 1]));
        q->last_ms[i] = ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, q->ev[0], q->ev[4]));
    q->last_ms[4] = ms;
    q->has_h = true;
    return EM_OK;
}

extern "C" int ethrex_mi355_quot_download(em_quot_plan *q, uint8_t *elems32) {
    if (!q || !elems32 || !q->has_h) return EM_ERR_INPUT;
    return fr_download_be(elems32, q->tw.n, q->buf[q->slot[0]],
                          (uint8_t *)q->buf[q->work]);
}

extern "C" int ethrex_mi355_quot_device_data(em_quot_plan *q, const void **ptr,
                                             size_t *n) {
    if (!q || !ptr || !q->has_h) return EM_ERR_INPUT;
    *ptr = q->buf[q->slot[0]];
    if (n) *n = q->tw.n;
    return EM_OK;
}

extern "C" int ethrex_mi355_quot_last_times(em_quot_plan *q,
                                            double times_ms[5]) {
    if (!q || !times_ms) return EM_ERR_INPUT;
    memcpy(times_ms, q->last_ms, sizeof q->last_ms);
    return EM_OK;
}

// ===================== R1CS evaluation (A z, B z, C z) =====================
// y = M z for the three sparse constraint matrices of a circuit (DESIGN.md
// "R1CS evaluation").  upload_matrix validates and repacks the CSR on the
// host (r1cs_pack.h: setup, not a run); eval is two or three launches on
// the null stream; the results are resident fe4m vectors that
// ethrex_mi355_quot_load_device takes device to device.

// short/long row threshold and long-row chunk: the measured defaults
// (profiles/r1cs.md) or EM_R1CS_T / EM_R1CS_CHUNK, read once per process
constexpr uint32_t R1CS_T_DEFAULT = 32;
constexpr uint32_t R1CS_CHUNK_DEFAULT = 1024;
struct r1cs_cfg {
    uint32_t T, chunk;
};
static const r1cs_cfg &r1cs_config() {
    static const r1cs_cfg c = [] {
        r1cs_cfg v = {R1CS_T_DEFAULT, R1CS_CHUNK_DEFAULT};
        if (const char *e = std::getenv("EM_R1CS_T")) {
            long long t = atoll(e);
            if (t >= 0) v.T = t > 0xffffffffll ? 0xffffffffu : (uint32_t)t;
        }
        if (const char *e = std::getenv("EM_R1CS_CHUNK")) {
            long long t = atoll(e);
            if (t >= 1 && t <= (1 << 24))
                v.chunk = (uint32_t)((t + 63) / 64 * 64);
        }
        return v;
    }();
    return c;
}

struct r1cs_mat {
    bool loaded = false;
    bool has_y = false;
    size_t n_rows = 0;
    uint32_t n_slices = 0, n_chunks = 0, n_long = 0;
    fe9 *d_dict = nullptr;
    uint2 *d_s_ent = nullptr;
    u64 *d_s_off = nullptr;
    u32 *d_s_len = nullptr, *d_s_perm = nullptr;
    uint2 *d_l_ent = nullptr;
    r1cs_chk *d_l_chunk = nullptr;
    u32 *d_l_chunk_off = nullptr, *d_l_row = nullptr;
    fe9 *d_part = nullptr;
    fe4 *d_y = nullptr;       // n results, allocated with the plan
};

struct em_r1cs_plan {
    size_t n = 0, n_vars = 0;
    fe4 *d_z = nullptr;
    uint8_t *d_stage = nullptr;   // max(n, n_vars) * 32 bytes
    uint32_t *d_err = nullptr;
    bool has_z = false;
    r1cs_mat m[3];
    hipEvent_t ev[2];
    int n_ev = 0;
    double last_ms[3] = {0, 0, 0};
};

static void r1cs_mat_free(r1cs_mat &m) {
    for (void *t : {(void *)m.d_dict, (void *)m.d_s_ent, (void *)m.d_s_off,
                    (void *)m.d_s_len, (void *)m.d_s_perm, (void *)m.d_l_ent,
                    (void *)m.d_l_chunk, (void *)m.d_l_chunk_off,
                    (void *)m.d_l_row, (void *)m.d_part})
        (void)hipFree(t);
    m.d_dict = nullptr;
    m.d_s_ent = m.d_l_ent = nullptr;
    m.d_s_off = nullptr;
    m.d_s_len = m.d_s_perm = m.d_l_chunk_off = m.d_l_row = nullptr;
    m.d_l_chunk = nullptr;
    m.d_part = nullptr;
    m.loaded = m.has_y = false;
}

extern "C" int ethrex_mi355_r1cs_plan_create(size_t n, size_t n_vars,
                                             em_r1cs_plan **plan) {
    if (!plan || !ntt_size_ok(n) || n_vars == 0 ||
        n_vars >= ((size_t)1 << 32))
        return EM_ERR_INPUT;
    int rc = require_gpu();
    if (rc) return rc;
    em_r1cs_plan *p = new em_r1cs_plan();
    p->n = n;
    p->n_vars = n_vars;
    hipError_t e = hipMalloc((void **)&p->d_z, n_vars * sizeof(fe4));
    if (e == hipSuccess)
        e = hipMalloc((void **)&p->d_stage, (n > n_vars ? n : n_vars) * 32);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_err, 4);
    for (int w = 0; w < 3 && e == hipSuccess; w++)
        e = hipMalloc((void **)&p->m[w].d_y, n * sizeof(fe4));
    for (; p->n_ev < 2 && e == hipSuccess; p->n_ev++)
        e = hipEventCreate(&p->ev[p->n_ev]);
    if (e != hipSuccess) {
        if (p->n_ev) p->n_ev--;   // the failed slot holds no event
        rc = hip_fail(e, "r1cs_plan_create");
        ethrex_mi355_r1cs_plan_destroy(p);
        return rc;
    }
    *plan = p;
    return EM_OK;
}

extern "C" int ethrex_mi355_r1cs_plan_destroy(em_r1cs_plan *p) {
    if (!p) return EM_ERR_INPUT;
    for (r1cs_mat &m : p->m) {
        r1cs_mat_free(m);
        (void)hipFree(m.d_y);
    }
    (void)hipFree(p->d_z);
    (void)hipFree(p->d_stage);
    (void)hipFree(p->d_err);
    for (int i = 0; i < p->n_ev; i++) (void)hipEventDestroy(p->ev[i]);
    delete p;
    return EM_OK;
}

// *dst = device copy of `count` elements of src (nothing for count == 0)
template <typename D, typename S>
static int r1cs_to_device(D **dst, const S *src, size_t count) {
    static_assert(sizeof(D) == sizeof(S), "same layout");
    if (count == 0) return EM_OK;
    HIP_TRY(hipMalloc((void **)dst, count * sizeof(D)));
    HIP_TRY(hipMemcpy(*dst, src, count * sizeof(D), hipMemcpyHostToDevice));
    return EM_OK;
}

static int r1cs_mat_to_device(r1cs_mat &m, const em_r1cs::r1cs_packed &pk) {
    // dictionary: canonical words -> fe9 Montgomery (host; upload is setup)
    std::vector<fe9> dict(pk.dict.size());
    for (size_t i = 0; i < dict.size(); i++)
        dict[i] = to_mont9<Fr9T>(fe9_from_u64x4(pk.dict[i].data()));
    int rc;
    if ((rc = r1cs_to_device(&m.d_dict, dict.data(), dict.size()))) return rc;
    if ((rc = r1cs_to_device(&m.d_s_ent, pk.s_ent.data(), pk.s_ent.size())))
        return rc;
    if ((rc = r1cs_to_device(&m.d_s_off, pk.s_off.data(), pk.s_off.size())))
        return rc;
    if ((rc = r1cs_to_device(&m.d_s_len, pk.s_len.data(), pk.s_len.size())))
        return rc;
    if ((rc = r1cs_to_device(&m.d_s_perm, pk.s_perm.data(), pk.s_perm.size())))
        return rc;
    if ((rc = r1cs_to_device(&m.d_l_ent, pk.l_ent.data(), pk.l_ent.size())))
        return rc;
    if ((rc = r1cs_to_device(&m.d_l_chunk, pk.l_chunk.data(),
                             pk.l_chunk.size()))) return rc;
    if ((rc = r1cs_to_device(&m.d_l_chunk_off, pk.l_chunk_off.data(),
                             pk.l_chunk_off.size()))) return rc;
    if ((rc = r1cs_to_device(&m.d_l_row, pk.l_row.data(), pk.l_row.size())))
        return rc;
    if (!pk.l_chunk.empty())
        HIP_TRY(hipMalloc((void **)&m.d_part, pk.l_chunk.size() * sizeof(fe9)));
    m.n_rows = pk.n_rows;
    m.n_slices = (uint32_t)pk.n_slices();
    m.n_chunks = (uint32_t)pk.l_chunk.size();
    m.n_long = (uint32_t)pk.l_row.size();
    return EM_OK;
}

extern "C" int ethrex_mi355_r1cs_upload_matrix(em_r1cs_plan *p, int which,
                                               const uint64_t *row_offs,
                                               const uint32_t *cols,
                                               const uint8_t *coeffs32,
                                               size_t n_rows) {
    if (!p || which < 0 || which > 2) return EM_ERR_INPUT;
    r1cs_mat &m = p->m[which];
    r1cs_mat_free(m);             // unloaded until the new one is in place
    const r1cs_cfg &cfg = r1cs_config();
    em_r1cs::r1cs_packed pk;
    int rc = em_r1cs::r1cs_pack(row_offs, cols, coeffs32, n_rows, p->n,
                                p->n_vars, cfg.T, cfg.chunk, pk);
    if (rc) return EM_ERR_INPUT;
    rc = r1cs_mat_to_device(m, pk);
    if (rc) {
        r1cs_mat_free(m);
        return rc;
    }
    m.loaded = true;
    return EM_OK;
}

static void r1cs_new_witness(em_r1cs_plan *p, bool ok) {
    p->has_z = ok;
    for (r1cs_mat &m : p->m) m.has_y = false;
}

extern "C" int ethrex_mi355_r1cs_upload_witness(em_r1cs_plan *p,
                                                const uint8_t *z32) {
    if (!p || !z32) return EM_ERR_INPUT;
    r1cs_new_witness(p, false);
    int rc = fr_upload_be(z32, p->n_vars, p->d_stage, p->d_z, p->d_err);
    if (rc) return rc;
    r1cs_new_witness(p, true);
    return EM_OK;
}

extern "C" int ethrex_mi355_r1cs_witness_from_device(em_r1cs_plan *p,
                                                     const void *d_fe4m,
                                                     uint64_t offset) {
    if (!p || !d_fe4m) return EM_ERR_INPUT;
    r1cs_new_witness(p, false);
    HIP_TRY(hipMemcpy(p->d_z, (const fe4 *)d_fe4m + offset,
                      p->n_vars * sizeof(fe4), hipMemcpyDeviceToDevice));
    r1cs_new_witness(p, true);
    return EM_OK;
}

extern "C" int ethrex_mi355_r1cs_eval(em_r1cs_plan *p, int which) {
    if (!p || which < 0 || which > 2) return EM_ERR_INPUT;
    r1cs_mat &m = p->m[which];
    if (!m.loaded || !p->has_z) return EM_ERR_INPUT;
    m.has_y = false;
    HIP_TRY(hipEventRecord(p->ev[0], 0));
    if (m.n_rows < p->n)
        HIP_TRY(hipMemsetAsync(m.d_y + m.n_rows, 0,
                               (p->n - m.n_rows) * sizeof(fe4), 0));
    if (m.n_slices)
        hipLaunchKernelGGL(k_r1cs_rows_sell, dim3(blocks_for(m.n_slices, 4)),
                           dim3(256), 0, 0, m.d_s_ent, m.d_s_off, m.d_s_len,
                           m.d_s_perm, m.n_slices, m.d_dict, p->d_z, m.d_y);
    if (m.n_chunks) {
        hipLaunchKernelGGL(k_r1cs_rows_long, dim3(blocks_for(m.n_chunks, 4)),
                           dim3(256), 0, 0, m.d_l_ent, m.d_l_chunk, m.n_chunks,
                           m.d_dict, p->d_z, m.d_part);
        hipLaunchKernelGGL(k_r1cs_long_sum, dim3(blocks_for(m.n_long, 4)),
                           dim3(256), 0, 0, m.d_part, m.d_l_chunk_off,
                           m.d_l_row, m.n_long, m.d_y);
    }
    HIP_TRY(hipEventRecord(p->ev[1], 0));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    float ms;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
    p->last_ms[which] = ms;
    m.has_y = true;
    return EM_OK;
}

extern "C" int ethrex_mi355_r1cs_download(em_r1cs_plan *p, int which,
                                          uint8_t *elems32) {
    if (!p || !elems32 || which < 0 || which > 2 || !p->m[which].has_y)
        return EM_ERR_INPUT;
    return fr_download_be(elems32, p->n, p->m[which].d_y, p->d_stage);
}

extern "C" int ethrex_mi355_r1cs_device_data(em_r1cs_plan *p, int which,
                                             const void **ptr, size_t *n) {
    if (!p || !ptr || which < 0 || which > 2 || !p->m[which].has_y)
        return EM_ERR_INPUT;
    *ptr = p->m[which].d_y;
    if (n) *n = p->n;
    return EM_OK;
}

extern "C" int ethrex_mi355_r1cs_last_times(em_r1cs_plan *p,
                                            double times_ms[3]) {
    if (!p || !times_ms) return EM_ERR_INPUT;
    memcpy(times_ms, p->last_ms, sizeof p->last_ms);
    return EM_OK;
}
