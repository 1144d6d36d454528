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
// msm_api_impl.h — the curve-templated MSM plan machinery.  Included by
// one TU per curve (api_msm_bn254/bls/g2.hip); every function is static so
// each TU instantiates only its own curve.
#pragma once
#include "em_api_common.h"  // before rocprim: it needs <cstring> in scope

#include <rocprim/rocprim.hpp>

#include "../../include/ethrex_mi355.h"
#include "gpu_field.h"
#include "gpu_g1_9.h"
#include "msm_kernels.h"
#include "msm_fbm_partition_kernels.h"

using namespace em;

// ============================ MSM plans ============================
// One templated plan implementation serves both curves:
//   Bn254G1: 64-B points, ark from_be_bytes_mod_order scalar reduction
//   BlsG1:   96-B points (canonical + subgroup-checked), raw 256-bit scalars
// The C ABI exposes separate opaque types (em_msm_plan / em_bls_msm_plan).

// The sort chain's outputs and the emitted window records, one set per step
// parity: the async path double-buffers them (step k+1 sorts while step k
// walks); the sync path runs parity 0.
struct msm_step_bufs {
    uint32_t *keys_out = nullptr;  // sorted keys (u16 per window if keys16)
    uint32_t *vals_out = nullptr;  // sorted point indices (+ sign bits)
    uint32_t *offsets = nullptr;   // NBUCKETS + 1 (merged mode: per slot)
    uint32_t *sched = nullptr;     // length-sorted bucket (slot) ids
    uint8_t *out = nullptr;        // NWIN_MAX Jacobian window records
};

template <typename C>
struct msm_plan_t {
    using F = typename C::F;
    static constexpr int PB = pt_bytes<C>::AFF;  // affine point bytes
    static constexpr int JB = pt_bytes<C>::JAC;  // Jacobian partial bytes
    static constexpr int AB = PB;                // affine out bytes
    static constexpr int SB = msm_curve<C>::BN_SCALARS ? 254 : 256;
    size_t n;
    int cbits;                        // window config: 8 (small) or 16
    g1aT<C> *d_pts = nullptr;
    g1aT<C> *d_pts_ext = nullptr;     // fixed-base table (FB_NWIN * n)
    bool fixed_base = false;
    // merged fixed-base mode (large BN254 G1, msm_fb_recode.h): window bits
    // c, or 0 = off.  d_pts_ext then holds NWIN_REAL * n table rows, built
    // by upload_points / gen_points; sb[].offsets/sched are per walk slot.
    int fb_c = 0;
    uint32_t fb_chunk = 0;            // L: most entries one walk slot takes
    int fb_len_bits = 0;              // L < 2^fb_len_bits (schedule sort)
    double fb_precompute_ms = 0;
    uint64_t fb_table_bytes = 0;
    uint32_t *d_fb_boff = nullptr;    // per-bucket offsets (NBUCKETS + 1)
    g1jT<C> *d_fb_slots = nullptr;    // per-slot walk results (NSLOT)
    // bucket partition (msm_fbm_partition.h) in place of the pair sort:
    // unit size T, or 0 = the rocPRIM chain (EM_MSM_FBM_SORT=rocprim)
    uint32_t fbp_tile = 0;
    uint32_t *d_fbp = nullptr;        // pass counters, offsets, unit scans
    uint8_t *d_inf = nullptr;
    fe4 *d_scalars = nullptr;
    uint8_t *d_scratch = nullptr;     // PB*n bytes: point/scalar byte staging
    uint32_t *d_keys = nullptr;       // 16n
    uint32_t *d_vals = nullptr;
    msm_step_bufs sb[2];
    void *d_sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    uint32_t *d_blen = nullptr;       // bucket lengths (schedule keys)
    uint32_t *d_blen_out = nullptr;
    uint32_t *d_bids = nullptr;       // bucket ids
    g1jT<C> *d_buckets = nullptr;     // NBUCKET_TOTAL
    g1jT<C> *d_seg_sum = nullptr;     // NWIN*NSEG
    g1jT<C> *d_seg_wsum = nullptr;
    g1jT<C> *d_partials = nullptr;    // NWIN*NBLK_PER_WIN
    g1jT<C> *d_windows = nullptr;     // NWIN
    uint32_t *d_err = nullptr;
    // batch-affine pairing tree (large BN254 MSMs only; see msm_kernels.h)
    bool use_tree = false;
    int tree_levels = 0;
    g1aT<C> *d_lvl[2] = {nullptr, nullptr};   // level ping/pong buffers
    feL<F::L> *d_aux = nullptr;               // denominator prefix products
    uint32_t *d_loff[2] = {nullptr, nullptr}; // level offsets ping/pong
    uint32_t *d_cnt = nullptr;                // per-bucket pair counts
    void *d_scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    bool keys16 = false;   // per-window sorts use u16 in-window-id keys
    bool have_scalars = false;
    bool have_points = false;
    hipEvent_t ev[6];
    double last_ms[5] = {0, 0, 0, 0, 0};
    // async pipelined path: the sort chain (HBM-heavy) of step k+1 runs on
    // s_sort concurrently with the compute chain (VALU-heavy bucket walk +
    // reduction) of step k on s_comp.  Sort outputs are double-buffered by
    // step parity (sb[]); depth-2 backpressure via ev_comp_done.
    hipStream_t s_sort = nullptr, s_comp = nullptr;
    uint8_t *h_out[2] = {nullptr, nullptr};   // pinned window staging
    hipEvent_t ev_sort_done[2], ev_comp_done[2];
    // per-parity hipGraphs of the sort and compute chains: one step costs
    // ~70 kernel dispatches (15 per-window rocPRIM sorts alone); captured
    // once (all pointers are parity-fixed) and replayed as 2 graph
    // launches — the async step's gap over the compute chain is host
    // dispatch pacing.  Rebuilt if the point table changes (precompute).
    hipGraphExec_t gx_sort[2] = {nullptr, nullptr};
    hipGraphExec_t gx_comp[2] = {nullptr, nullptr};
    const void *gx_pts[2] = {nullptr, nullptr};
    // contention gating: the bucket walk launches as two segments; the
    // NEXT step's sort chain (HBM+issue-hungry rocPRIM kernels) waits for
    // segment A (~80% of the work), so sorts contend only with the walk's
    // tail instead of its whole duration (async step 27.9 -> see ledger)
    hipEvent_t ev_walkA[2];
    // a pending pipelined result: h_out[par] holds nwin UNSCALED Jacobian
    // window records; delivery runs the host Horner (cbits doublings + 1
    // add per window) and writes affine (out_mode 0) or Jacobian (1) bytes
    struct {
        uint8_t *dest;
        int out_mode;
        int nwin;
        int cbits;
        bool valid;
    } pend[2] = {{nullptr, 0, 0, 0, false}, {nullptr, 0, 0, 0, false}};
    int apar = 0;
};

// sb[].out / h_out hold up to NWIN_MAX Jacobian window records (c=8: 32 windows)
constexpr int NWIN_MAX = 32;

template <typename C>
static int msm_sync_t(msm_plan_t<C> *p);
template <typename C>
static void host_windows_horner(const uint8_t *wire, int nwin, int cbits,
                                uint8_t *out, int out_mode);

template <typename C>
static int msm_destroy_t(msm_plan_t<C> *p) {
    if (!p) return EM_ERR_INPUT;
    if (p->s_comp) {
        (void)hipStreamSynchronize(p->s_sort);
        (void)hipStreamSynchronize(p->s_comp);
    }
    (void)hipFree(p->d_pts);
    (void)hipFree(p->d_pts_ext);
    (void)hipFree(p->d_fb_boff);
    (void)hipFree(p->d_fb_slots);
    (void)hipFree(p->d_fbp);
    (void)hipFree(p->d_inf);
    (void)hipFree(p->d_scalars);
    (void)hipFree(p->d_scratch);
    (void)hipFree(p->d_keys);
    (void)hipFree(p->d_vals);
    (void)hipFree(p->d_sort_tmp);
    (void)hipFree(p->d_blen);
    (void)hipFree(p->d_blen_out);
    (void)hipFree(p->d_bids);
    (void)hipFree(p->d_buckets);
    (void)hipFree(p->d_seg_sum);
    (void)hipFree(p->d_seg_wsum);
    (void)hipFree(p->d_partials);
    (void)hipFree(p->d_windows);
    (void)hipFree(p->d_err);
    (void)hipFree(p->d_lvl[0]);
    (void)hipFree(p->d_lvl[1]);
    (void)hipFree(p->d_aux);
    (void)hipFree(p->d_loff[0]);
    (void)hipFree(p->d_loff[1]);
    (void)hipFree(p->d_cnt);
    (void)hipFree(p->d_scan_tmp);
    for (auto &b : p->sb) {
        (void)hipFree(b.keys_out);
        (void)hipFree(b.vals_out);
        (void)hipFree(b.offsets);
        (void)hipFree(b.sched);
        (void)hipFree(b.out);
    }
    if (p->h_out[0]) (void)hipHostFree(p->h_out[0]);
    if (p->h_out[1]) (void)hipHostFree(p->h_out[1]);
    for (int i = 0; i < 2; i++) {
        if (p->gx_sort[i]) (void)hipGraphExecDestroy(p->gx_sort[i]);
        if (p->gx_comp[i]) (void)hipGraphExecDestroy(p->gx_comp[i]);
    }
    if (p->s_sort) (void)hipStreamDestroy(p->s_sort);
    if (p->s_comp) (void)hipStreamDestroy(p->s_comp);
    delete p;
    return EM_OK;
}

// ---- merged fixed-base mode: selection and per-c dispatch ----
// Default on for BN254 G1 plans of n >= FBM_MIN_N when the table fits:
// free device memory (hipMemGetInfo; EM_MSM_FB_FREE_BYTES overrides the
// probe) must cover 1.5x the table (the table, plus the sorted pairs in
// three copies = a third of it, plus slack) and 6 GiB for the bucket/slot
// arrays.  EM_MSM_FB=0 forces the separate-window path, EM_MSM_FB=<c>
// (20, 22, 24) forces the mode at any n.  Table indices ride in the sorted
// values next to the sign bits, so NWIN_REAL * n must stay below 2^30.
constexpr int FBM_DEFAULT_C = 22;
constexpr size_t FBM_MIN_N = (size_t)1 << 23;

// d_fbp layout for 2^IB buckets, in u32 words: the bin counters of passes A
// and B (adjacent: zeroed by one launch), their scans, and the unit counts
// and unit offsets that passes B and C share
struct fbp_layout {
    size_t cnt_a, cnt_b, off_a, off_b, ucnt, uoff, words;
};
static inline fbp_layout fbp_lay(uint32_t nbuckets) {
    const size_t na = (size_t)(nbuckets >> 16) + 1;   // NBIN_A + 1
    const size_t nc = (size_t)(nbuckets >> 8) + 1;    // NREG_C + 1
    fbp_layout l;
    l.cnt_a = 0;
    l.cnt_b = na;
    l.off_a = na + nc;
    l.off_b = 2 * na + nc;
    l.ucnt = 2 * na + 2 * nc;
    l.uoff = 2 * na + 3 * nc;
    l.words = 2 * na + 4 * nc;
    return l;
}
static inline size_t fbp_words(uint32_t nbuckets) { return fbp_lay(nbuckets).words; }

template <typename FN>
static int fbm_dispatch(int c, FN fn) {
    switch (c) {
    case 20: return fn(CfgFbm20{});
    case 22: return fn(CfgFbm22{});
    case 24: return fn(CfgFbm24{});
    }
    return EM_ERR_INPUT;
}

template <typename C>
static int fbm_select(size_t n) {
    if constexpr (!msm_curve<C>::FB_MERGED) {
        return 0;
    } else {
        int c = 0;
        if (const char *ev = std::getenv("EM_MSM_FB")) {
            c = atoi(ev);
            if (c != 20 && c != 22 && c != 24) return 0;
        } else if (n >= FBM_MIN_N && std::getenv("EM_MSM_TREE") == nullptr) {
            c = FBM_DEFAULT_C;
        } else {
            return 0;
        }
        size_t nwr = (size_t)((254 + c - 1) / c);
        if (nwr * n >= ((size_t)1 << 30)) return 0;  // SGN_IDX
        size_t table = nwr * n * sizeof(g1aT<C>);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
        if (const char *fv = std::getenv("EM_MSM_FB_FREE_BYTES"))
            free_b = (size_t)strtoull(fv, nullptr, 10);
        if (free_b < table + table / 2 + ((size_t)6 << 30)) return 0;
        return c;
    }
}

// The one config ladder: calls fn(cfg_tag) with the configuration this plan
// runs and returns its result.  The if constexpr guards keep a curve from
// instantiating a config (and its kernels) that it never runs.
template <typename C, typename FN>
static int msm_with_cfg(msm_plan_t<C> *p, FN fn) {
    if constexpr (msm_curve<C>::FB_MERGED) {
        if (p->fb_c) return fbm_dispatch(p->fb_c, fn);
    }
    if constexpr (!msm_curve<C>::SIGNED_ONLY) {
        if (p->fixed_base) return fn(CfgFB{});
    }
    if (p->cbits == 8) return fn(msm_cfg<8, msm_plan_t<C>::SB>{});
    if constexpr (msm_curve<C>::BN_SCALARS) {
        if (p->cbits == 17) return fn(CfgSg254{});
    }
    if constexpr (msm_curve<C>::SIGNED_ONLY)
        return EM_ERR_INPUT;  // unreachable: create picks 8 or 17
    else
        return fn(msm_cfg<16, msm_plan_t<C>::SB>{});
}

template <typename C>
static int msm_create_t(size_t n, msm_plan_t<C> **plan) {
    if (!plan || n == 0) return EM_ERR_INPUT;
    int rc = require_gpu();
    if (rc) return rc;
    auto *p = new msm_plan_t<C>();
    p->n = n;
    p->fb_c = fbm_select<C>(n);
    if (p->fb_c) {
        // the table first: if it does not fit after all, run today's path
        size_t nwr = (size_t)((254 + p->fb_c - 1) / p->fb_c);
        p->fb_table_bytes = nwr * n * sizeof(g1aT<C>);
        if (hipMalloc((void **)&p->d_pts_ext, p->fb_table_bytes) !=
            hipSuccess) {
            (void)hipGetLastError();
            p->d_pts_ext = nullptr;
            p->fb_table_bytes = 0;
            p->fb_c = 0;
        }
    }
    // small MSMs (blob-KZG-sized) use c=8: the fixed bucket-reduction tail
    // shrinks 256x.  Large BN254 MSMs default to SIGNED c=17 (15 windows:
    // 6% fewer point adds at the same bucket count; scalars are reduced mod
    // r so the top window absorbs the carry).  BLS scalars are raw 256-bit
    // (blst SCALAR_BITS=256) — no carry headroom — and stay unsigned c=16.
    // EM_MSM_TREE selects the unsigned c=16 config (the env-gated
    // batch-affine experiment is built for that geometry).
    if (n <= 65536)
        p->cbits = 8;
    else if (msm_curve<C>::BN_SCALARS &&
             (msm_curve<C>::SIGNED_ONLY ||
              std::getenv("EM_MSM_TREE") == nullptr))
        p->cbits = 17;
    else
        p->cbits = 16;
    if (p->cbits == 17 && n >= ((size_t)1 << 30)) {  // SGN_IDX
        if (msm_curve<C>::SIGNED_ONLY) {
            delete p;
            g_last_err = "msm_plan_create: n >= 2^30 unsupported";
            return EM_ERR_INPUT;
        }
        p->cbits = 16;
    }
    // total: sorted (key, value) pairs per step; nsched: entries of the
    // walk schedule (buckets; merged mode: slots)
    int nwin = 0, nseg_tot = 0, npart = 0, sort_bits = 0;
    uint32_t nbuckets = 0;
    size_t total = 0, nsched = 0;
    msm_with_cfg(p, [&](auto cfg) {
        using G = decltype(cfg);
        nwin = G::NWIN;
        nbuckets = G::NBUCKETS;
        nseg_tot = G::NWIN * G::NSEG;
        npart = G::NPART;
        sort_bits = G::SORT_BITS;
        if constexpr (is_fbm<G>::value) {
            total = n * (size_t)G::NWIN_REAL;
            nsched = G::NSLOT;
        } else {
            total = n * (size_t)G::NWIN;
            nsched = G::NBUCKETS;
        }
        return EM_OK;
    });
    // per-window sorts (n >= 2^23) carry only the 16-bit in-window id as
    // the key: 25% less sort traffic, half the key memory
    p->keys16 = n >= ((size_t)1 << 23);
    if (p->fb_c) {
        p->keys16 = false;  // one global sort over u32 bucket ids
        // slot length cap: 1.25x the average run, never below it (the
        // NSLOT bound), EM_MSM_FB_CHUNK overrides for experiments
        size_t avg = (total + nbuckets - 1) / nbuckets;
        size_t L = (avg * 5 + 3) / 4;
        if (const char *cv = std::getenv("EM_MSM_FB_CHUNK"))
            L = (size_t)strtoull(cv, nullptr, 10);
        if (L < avg) L = avg;
        if (L < 8) L = 8;
        p->fb_chunk = (uint32_t)L;
        while ((L >> p->fb_len_bits) != 0) p->fb_len_bits++;
        // stage 1 groups by bucket with the partition unless
        // EM_MSM_FBM_SORT=rocprim asks for the pair sort (A/B, fallback);
        // EM_MSM_FBM_TILE sets the unit size (tests: many units per region)
        const char *sv = std::getenv("EM_MSM_FBM_SORT");
        if (sv == nullptr || std::strcmp(sv, "rocprim") != 0) {
            size_t T = FBP_TILE_DEFAULT;
            if (const char *tv = std::getenv("EM_MSM_FBM_TILE"))
                T = (size_t)strtoull(tv, nullptr, 10);
            if (T < 1) T = 1;
            if (T > FBP_TILE_MAX) T = FBP_TILE_MAX;
            p->fbp_tile = (uint32_t)T;
        }
    }
    const size_t kb = p->keys16 ? 2 : 4;
    hipError_t e = hipSuccess;
    auto mal = [&](void **ptr, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc(ptr, bytes);
    };
    mal((void **)&p->d_pts, n * sizeof(g1aT<C>));
    mal((void **)&p->d_inf, n);
    mal((void **)&p->d_scalars, n * sizeof(fe4));
    mal((void **)&p->d_scratch, n * (size_t)msm_plan_t<C>::PB);
    mal((void **)&p->d_keys, total * kb);
    mal((void **)&p->d_vals, total * 4);
    for (auto &b : p->sb) {
        mal((void **)&b.keys_out, total * kb);
        mal((void **)&b.vals_out, total * 4);
        mal((void **)&b.offsets, (nsched + 1) * 4);
        mal((void **)&b.sched, nsched * 4);
        mal((void **)&b.out, (size_t)NWIN_MAX * msm_plan_t<C>::JB);
    }
    mal((void **)&p->d_blen, nsched * 4);
    mal((void **)&p->d_blen_out, nsched * 4);
    mal((void **)&p->d_bids, nsched * 4);
    mal((void **)&p->d_buckets, (size_t)nbuckets * sizeof(g1jT<C>));
    if constexpr (msm_curve<C>::FB_MERGED) if (p->fb_c) {
        mal((void **)&p->d_fb_boff, ((size_t)nbuckets + 1) * 4);
        mal((void **)&p->d_fb_slots, nsched * sizeof(g1jT<C>));
        mal((void **)&p->d_cnt, ((size_t)nbuckets + 1) * 4);
        mal((void **)&p->d_loff[0], ((size_t)nbuckets + 1) * 4);
        mal((void **)&p->d_loff[1], ((size_t)nbuckets + 1) * 4);
        if (e == hipSuccess)
            e = rocprim::exclusive_scan(nullptr, p->scan_tmp_bytes, p->d_cnt,
                                        p->d_loff[0], 0u,
                                        (size_t)nbuckets + 1);
        if (e == hipSuccess) e = hipMalloc(&p->d_scan_tmp, p->scan_tmp_bytes);
        // partition counters: the largest scan is the one sized above
        if (p->fbp_tile) mal((void **)&p->d_fbp, fbp_words(nbuckets) * 4);
    }
    mal((void **)&p->d_seg_sum, (size_t)nseg_tot * sizeof(g1jT<C>));
    mal((void **)&p->d_seg_wsum, (size_t)nseg_tot * sizeof(g1jT<C>));
    mal((void **)&p->d_partials, (size_t)npart * sizeof(g1jT<C>));
    mal((void **)&p->d_windows, (size_t)nwin * sizeof(g1jT<C>));
    mal((void **)&p->d_err, 4);
    if (e == hipSuccess) {
        if (p->keys16)
            e = rocprim::radix_sort_pairs(
                nullptr, p->sort_tmp_bytes, (const uint16_t *)p->d_keys,
                (uint16_t *)p->sb[0].keys_out, p->d_vals, p->sb[0].vals_out,
                n, 0, 16);
        else
            e = rocprim::radix_sort_pairs(
                nullptr, p->sort_tmp_bytes, p->d_keys, p->sb[0].keys_out,
                p->d_vals, p->sb[0].vals_out, total, 0, sort_bits);
        size_t tmp_len = 0;
        if (e == hipSuccess)
            e = rocprim::radix_sort_pairs(nullptr, tmp_len, p->d_blen,
                                          p->d_blen_out, p->d_bids,
                                          p->sb[0].sched, nsched, 0, 32);
        if (tmp_len > p->sort_tmp_bytes) p->sort_tmp_bytes = tmp_len;
        if (e == hipSuccess) e = hipMalloc(&p->d_sort_tmp, p->sort_tmp_bytes);
    }
    // batch-affine pairing tree: EXPERIMENTAL alternative bucket walk for
    // large BN254 MSMs (opt-in via EM_MSM_TREE=1).  Parity-green, but the
    // per-round bisect (profiles/r01_summary.md) measured it at 60 ms vs
    // 29.8 ms for the flat XYZZ walk at 2^24: the two-pass level structure
    // has strictly worse memory-level parallelism than the single prefetched
    // XYZZ stream, and the batched-inversion chains serialize.  Kept for
    // round-2 experiments; the product path stays XYZZ.
    if constexpr (std::is_same_v<C, Bn254G1>) {
        size_t avg = total / CfgL254::NBUCKETS;
        if (p->cbits == 16 && avg >= 8 && e == hipSuccess && !p->fb_c &&
            std::getenv("EM_MSM_TREE") != nullptr) {
            p->use_tree = true;
            int lg = 0;
            while ((avg >> lg) > 1) lg++;  // floor log2(avg run length)
            p->tree_levels = lg - 2;
            if (p->tree_levels < 1) p->tree_levels = 1;
            if (p->tree_levels > 8) p->tree_levels = 8;
            size_t c0 = total / 2 + CfgL254::NBUCKETS + 1;
            size_t c1 = total / 4 + CfgL254::NBUCKETS + 1;
            mal((void **)&p->d_lvl[0], c0 * sizeof(g1aT<C>));
            mal((void **)&p->d_lvl[1], c1 * sizeof(g1aT<C>));
            mal((void **)&p->d_aux,
                (size_t)AUX_PLANES * c0 * sizeof(feL<msm_plan_t<C>::F::L>));
            mal((void **)&p->d_loff[0], ((size_t)CfgL254::NBUCKETS + 1) * 4);
            mal((void **)&p->d_loff[1], ((size_t)CfgL254::NBUCKETS + 1) * 4);
            mal((void **)&p->d_cnt, ((size_t)CfgL254::NBUCKETS + 1) * 4);
            if (e == hipSuccess) {
                e = rocprim::exclusive_scan(nullptr, p->scan_tmp_bytes,
                                            p->d_cnt, p->d_loff[0], 0u,
                                            (size_t)CfgL254::NBUCKETS + 1);
                if (e == hipSuccess)
                    e = hipMalloc(&p->d_scan_tmp, p->scan_tmp_bytes);
            }
            if (e == hipErrorOutOfMemory) {
                // tree buffers don't fit (very large n): fall back to the
                // XYZZ bucket walk rather than failing plan creation
                (void)hipFree(p->d_lvl[0]);
                (void)hipFree(p->d_lvl[1]);
                (void)hipFree(p->d_aux);
                (void)hipFree(p->d_loff[0]);
                (void)hipFree(p->d_loff[1]);
                (void)hipFree(p->d_cnt);
                (void)hipFree(p->d_scan_tmp);
                p->d_lvl[0] = p->d_lvl[1] = nullptr;
                p->d_aux = nullptr;
                p->d_loff[0] = p->d_loff[1] = nullptr;
                p->d_cnt = nullptr;
                p->d_scan_tmp = nullptr;
                p->use_tree = false;
                e = hipSuccess;
                (void)hipGetLastError();
            }
        }
    }
    for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipEventCreate(&p->ev[i]);
    // async pipelined path: streams, pinned staging and ordering events
    // EQUAL-priority streams (default).  The pass-B experiment that gave
    // s_comp higher priority STARVED the low-priority sort stream: the
    // kernel timeline showed the sorts serializing into a 4.3 ms gap
    // AFTER each bucket walk instead of overlapping it (ROCm priority
    // queues only dispatch low-priority work when the high-priority
    // queue is idle).  EM_MSM_PRIO=1 re-enables the priority variant.
    if (std::getenv("EM_MSM_PRIO")) {
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (e == hipSuccess)
            e = hipStreamCreateWithPriority(&p->s_sort,
                                            hipStreamNonBlocking, prio_lo);
        if (e == hipSuccess)
            e = hipStreamCreateWithPriority(&p->s_comp,
                                            hipStreamNonBlocking, prio_hi);
    } else {
        if (e == hipSuccess)
            e = hipStreamCreateWithFlags(&p->s_sort, hipStreamNonBlocking);
        if (e == hipSuccess)
            e = hipStreamCreateWithFlags(&p->s_comp, hipStreamNonBlocking);
    }
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        if (e == hipSuccess)
            e = hipHostMalloc((void **)&p->h_out[i],
                              (size_t)NWIN_MAX * msm_plan_t<C>::JB);
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&p->ev_sort_done[i],
                                        hipEventDisableTiming);
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&p->ev_comp_done[i],
                                        hipEventDisableTiming);
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&p->ev_walkA[i],
                                        hipEventDisableTiming);
        // record once so the first hipStreamWaitEvent sees a signaled event
        if (e == hipSuccess) e = hipEventRecord(p->ev_comp_done[i], 0);
        if (e == hipSuccess) e = hipEventRecord(p->ev_walkA[i], 0);
    }
    if (e != hipSuccess) {
        msm_destroy_t(p);
        return hip_fail(e, "msm_plan_create");
    }
    *plan = p;
    return EM_OK;
}

// merged fixed-base mode: (re)build T[w*n + i] = 2^(c*w) * P_i from the
// points just loaded.  Setup work, once per point set; the time is kept
// for last_times()/fb_info.
template <typename C>
static int fbm_build_table(msm_plan_t<C> *p) {
    if constexpr (msm_curve<C>::FB_MERGED) {
        if (!p->fb_c) return EM_OK;
        HIP_TRY(hipEventRecord(p->ev[0], 0));
        fbm_dispatch(p->fb_c, [&](auto cfg) {
            using G = decltype(cfg);
            hipLaunchKernelGGL((k_fbm_precompute<C, G>),
                               dim3(blocks_for(p->n, 256)), dim3(256), 0, 0,
                               p->d_pts, p->d_inf, p->n, p->d_pts_ext);
            return 0;
        });
        HIP_TRY(hipEventRecord(p->ev[1], 0));
        HIP_TRY(hipDeviceSynchronize());
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
        p->fb_precompute_ms = ms;
    }
    return EM_OK;
}

template <typename C>
static int msm_upload_points_t(msm_plan_t<C> *p, const uint8_t *points) {
    if (!p || !points) return EM_ERR_INPUT;
    int rc0 = msm_sync_t(p);
    if (rc0) return rc0;
    constexpr int PB = msm_plan_t<C>::PB;
    HIP_TRY(hipMemset(p->d_err, 0, 4));
    HIP_TRY(hipMemcpy(p->d_scratch, points, p->n * PB, hipMemcpyHostToDevice));
    if constexpr (msm_curve<C>::OWN_IO) {
        msm_curve<C>::launch_parse_points(p->d_scratch, p->d_pts, p->d_inf,
                                          p->n, p->d_err);
    } else if constexpr (std::is_same_v<C, BlsG2>) {
        hipLaunchKernelGGL(k_bls_g2_parse_points, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_scratch, p->d_pts, p->d_inf,
                           p->n, p->d_err);
    } else if constexpr (std::is_same_v<C, BlsG1>) {
        hipLaunchKernelGGL(k_bls_parse_points, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_scratch, p->d_pts, p->d_inf,
                           p->n, p->d_err);
    } else {
        hipLaunchKernelGGL(k_parse_points, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_scratch, p->d_pts, p->d_inf,
                           p->n, p->d_err);
    }
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, p->d_err, 4, hipMemcpyDeviceToHost));
    if (err & 2u) {
        g_last_err = "non-canonical coordinate";
        return EM_ERR_INPUT;
    }
    if (err & 4u) {
        g_last_err = msm_curve<C>::SUBGROUP_ERR;
        return EM_ERR_POINT;
    }
    if (err) return EM_ERR_POINT;
    int rcf = fbm_build_table(p);
    if (rcf) return rcf;
    p->have_points = true;
    p->fixed_base = false;
    return EM_OK;
}

template <typename C>
static int msm_gen_points_t(msm_plan_t<C> *p, uint64_t start) {
    if (!p) return EM_ERR_INPUT;
    int rc0 = msm_sync_t(p);  // drain async steps: d_pts is live on s_comp
    if (rc0) return rc0;
    if constexpr (msm_curve<C>::OWN_IO) {
        msm_curve<C>::launch_gen_points(p->d_pts, p->d_inf, p->n, start);
    } else if constexpr (std::is_same_v<C, BlsG2>) {
        hipLaunchKernelGGL(k_bls_g2_gen_points, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_pts, p->d_inf, p->n, start);
    } else if constexpr (std::is_same_v<C, BlsG1>) {
        hipLaunchKernelGGL(k_bls_gen_points, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_pts, p->d_inf, p->n, start);
    } else {
        hipLaunchKernelGGL(k_gen_points, dim3(blocks_for(p->n, 256)), dim3(256),
                           0, 0, p->d_pts, p->d_inf, p->n, start);
    }
    HIP_TRY(hipDeviceSynchronize());
    int rcf = fbm_build_table(p);
    if (rcf) return rcf;
    p->have_points = true;
    p->fixed_base = false;
    return EM_OK;
}

template <typename C>
static int msm_download_points_t(msm_plan_t<C> *p, uint8_t *out) {
    if (!p || !out || !p->have_points) return EM_ERR_INPUT;
    int rc0 = msm_sync_t(p);  // drain async steps: d_scratch races otherwise
    if (rc0) return rc0;
    constexpr int PB = msm_plan_t<C>::PB;
    if constexpr (msm_curve<C>::OWN_IO) {
        msm_curve<C>::launch_points_to_be(p->d_pts, p->d_inf, p->d_scratch,
                                          p->n);
    } else if constexpr (std::is_same_v<C, BlsG2>) {
        hipLaunchKernelGGL(k_bls_g2_points_to_be, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_pts, p->d_inf, p->d_scratch,
                           p->n);
    } else if constexpr (std::is_same_v<C, BlsG1>) {
        hipLaunchKernelGGL(k_bls_points_to_be, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_pts, p->d_inf, p->d_scratch,
                           p->n);
    } else {
        hipLaunchKernelGGL(k_points_to_be, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_pts, p->d_inf, p->d_scratch,
                           p->n);
    }
    HIP_TRY(hipMemcpy(out, p->d_scratch, p->n * PB, hipMemcpyDeviceToHost));
    return EM_OK;
}

// build the fixed-base table (blob-KZG mode: points fixed across blobs).
// requires the small-config plan (n <= 65536); ~5 ms once per setup.
template <typename C>
static int msm_precompute_t(msm_plan_t<C> *p) {
    if (!p || !p->have_points) return EM_ERR_INPUT;
    int rc0 = msm_sync_t(p);  // drain async steps before rebuilding tables
    if (rc0) return rc0;
    if (p->cbits != 8) {
        g_last_err = "fixed-base precompute requires n <= 65536";
        return EM_ERR_INPUT;
    }
    if (!p->d_pts_ext) {
        hipError_t e =
            hipMalloc((void **)&p->d_pts_ext,
                      (size_t)FB_NWIN * p->n * sizeof(g1aT<C>));
        if (e != hipSuccess) return hip_fail(e, "fb precompute alloc");
    }
    hipLaunchKernelGGL((k_fb_precompute<C>),
                       dim3(blocks_for(p->n * FB_NWIN, 256)), dim3(256), 0, 0,
                       p->d_pts, p->d_inf, p->n, p->d_pts_ext);
    HIP_TRY(hipDeviceSynchronize());
    p->fixed_base = true;
    return EM_OK;
}

template <typename C>
static int msm_upload_scalars_t(msm_plan_t<C> *p, const uint8_t *scalars32) {
    if (!p || !scalars32) return EM_ERR_INPUT;
    int rc0 = msm_sync_t(p);
    if (rc0) return rc0;
    HIP_TRY(hipMemcpy(p->d_scratch, scalars32, p->n * 32, hipMemcpyHostToDevice));
    if constexpr (!msm_curve<C>::BN_SCALARS) {
        // raw 256-bit scalars, no reduction (blst SCALAR_BITS = 256)
        hipLaunchKernelGGL(k_bls_parse_scalars, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_scratch, p->d_scalars, p->n);
    } else {
        // ark from_be_bytes_mod_order reduction
        hipLaunchKernelGGL(k_parse_scalars, dim3(blocks_for(p->n, 256)),
                           dim3(256), 0, 0, p->d_scratch, p->d_scalars, p->n);
    }
    HIP_TRY(hipDeviceSynchronize());
    p->have_scalars = true;
    return EM_OK;
}

// HOST window combine: fold the 2^(C*w) window factors over the nwin
// UNSCALED Jacobian window records with a Horner pass
//   acc = W_{n-1}; repeat { acc = 2^C * acc + W_w }  (C doublings + 1 add)
// then emit affine (out_mode 0) or Jacobian wire (out_mode 1) bytes.
// ~240 doublings on the host field core cost ~0.2 ms (BN254) / ~2 ms (G2
// over Fp2) and — on the pipelined path — fully overlap the next step's
// GPU work; on the GPU they were the serial latency tail of the reduction
// (one lane per window; 9.7 ms/launch for G2).  This also covers the
// Jacobian->affine conversion host_jac_to_affine used to do.
template <typename C>
static void host_windows_horner(const uint8_t *wire, int nwin, int cbits,
                                uint8_t *out, int out_mode) {
    constexpr int JB = pt_bytes<C>::JAC;
    g1jT<C> acc = g1_inf9<C>();
    for (int w = nwin - 1; w >= 0; w--) {
        if (w != nwin - 1)
            for (int d = 0; d < cbits; d++) acc = g1_dbl9<C>(acc);
        g1jT<C> t;
        if (g1_jac_from_be9<C>(t, wire + (size_t)w * JB))
            acc = g1_add9<C>(acc, t);
    }
    if (out_mode == 0)
        g1_to_affine_be9<C>(out, acc);
    else
        g1_jac_be9<C>(out, acc);
}

// deliver a completed pipelined result to its caller's buffer
template <typename C>
static int msm_deliver(msm_plan_t<C> *p, int par) {
    if (!p->pend[par].valid) return EM_OK;
    HIP_TRY(hipEventSynchronize(p->ev_comp_done[par]));
    host_windows_horner<C>(p->h_out[par], p->pend[par].nwin,
                           p->pend[par].cbits, p->pend[par].dest,
                           p->pend[par].out_mode);
    p->pend[par].valid = false;
    return EM_OK;
}

// deliver the OLDEST pending pipelined step (blocking only on its compute
// chain) WITHOUT draining the pipeline: later enqueued steps keep running.
// The N>1 exchange loop uses this to overlap AllGather + combine of step k
// with the GPU compute of step k+1.
template <typename C>
static int msm_wait_one_t(msm_plan_t<C> *p) {
    if (!p) return EM_ERR_INPUT;
    if (!p->s_comp) return EM_OK;
    if (p->pend[p->apar].valid) return msm_deliver(p, p->apar);
    if (p->pend[p->apar ^ 1].valid) return msm_deliver(p, p->apar ^ 1);
    return EM_OK;
}

// drain the pipeline (also called before any sync-path operation)
template <typename C>
static int msm_sync_t(msm_plan_t<C> *p) {
    if (!p) return EM_ERR_INPUT;
    if (!p->s_comp) return EM_OK;
    HIP_TRY(hipStreamSynchronize(p->s_sort));
    HIP_TRY(hipStreamSynchronize(p->s_comp));
    int rc = msm_deliver(p, p->apar ^ 1);
    if (rc) return rc;
    return msm_deliver(p, p->apar);
}

// ======================= the MSM step, in four stages =======================
// sort chain -> walk -> reduce -> emit.  Each stage only enqueues kernels
// and rocPRIM calls on the stream it is given, reading and writing the step
// buffers of one parity (p->sb[par], p->d_loff[par]), so the same code runs
// directly on a stream and under hipGraph capture.  Event records belong to
// the callers: msm_run_sync_cfg (run / run_partial: parity 0 on the null
// stream, phase events between the stages) and msm_run_async_cfg (two
// streams, per-parity graphs).  CFG is a window config (msm_cfg), the blob
// fixed-base config (CfgFB) or a merged fixed-base config (msm_cfg_fbm).
#define EM_HT(call)                         \
    do {                                    \
        hipError_t _e = (call);             \
        if (_e != hipSuccess) return _e;    \
    } while (0)

// the points the walk gathers from: both fixed-base modes read the table
template <typename C, typename CFG>
static const g1aT<C> *msm_walk_pts(const msm_plan_t<C> *p) {
    constexpr bool TABLE = std::is_same_v<CFG, CfgFB> || is_fbm<CFG>::value;
    return TABLE ? p->d_pts_ext : p->d_pts;
}

// EM_MSM_SPLIT=<pct> (experiment, async direct path only): the walk launches
// as two segments and the next step's sort chain waits for the first
static int msm_split_pct() {
    static int pct = std::getenv("EM_MSM_SPLIT")
                         ? atoi(std::getenv("EM_MSM_SPLIT"))
                         : 0;
    return pct;
}

// Stage 1 of the merged fixed-base mode, grouping: the three-pass bucket
// partition (msm_fbm_partition_kernels.h).  Leaves sb[par].vals_out grouped
// by bucket id and d_fb_boff[0..NBUCKETS], as the pair sort + k_offsets do.
// Intermediates live in buffers the pair sort would use: pass A writes u16
// keys to d_keys and values to d_vals, pass B writes u8 keys behind the u16
// keys (d_keys holds 4 bytes per entry) and values to sb[par].keys_out.
// All sizes given to rocPRIM and every grid are host constants.
template <typename C, typename CFG>
static hipError_t fbm_enqueue_partition(msm_plan_t<C> *p, int par,
                                        hipStream_t st) {
    using G = fbp_geom<CFG::IB>;
    const msm_step_bufs &b = p->sb[par];
    const size_t total = p->n * (size_t)CFG::NWIN_REAL;
    const uint32_t T = p->fbp_tile;
    const fbp_layout l = fbp_lay(G::NBUCKETS);
    uint32_t *cnt_a = p->d_fbp + l.cnt_a, *cnt_b = p->d_fbp + l.cnt_b;
    uint32_t *off_a = p->d_fbp + l.off_a, *off_b = p->d_fbp + l.off_b;
    uint32_t *ucnt = p->d_fbp + l.ucnt, *uoff = p->d_fbp + l.uoff;
    uint32_t *cnt_c = p->d_cnt;       // NBUCKETS + 1; stage 1 reuses it after
    uint16_t *k16 = (uint16_t *)p->d_keys;
    uint8_t *k8 = (uint8_t *)p->d_keys + total * 2;
    uint32_t *v1 = p->d_vals, *v2 = b.keys_out;
    auto scan = [&](uint32_t *in, uint32_t *out, size_t len) {
        size_t stmp = p->scan_tmp_bytes;
        return rocprim::exclusive_scan(p->d_scan_tmp, stmp, in, out, 0u, len,
                                       rocprim::plus<uint32_t>(), st);
    };
    auto units = [&](const uint32_t *off, uint32_t regions) {
        hipLaunchKernelGGL((k_fbp_unit_counts<CFG>),
                           dim3(blocks_for((size_t)regions + 1, 256)),
                           dim3(256), 0, st, off, regions, T, ucnt);
        return scan(ucnt, uoff, (size_t)regions + 1);
    };
    const uint32_t nab = (uint32_t)(l.off_a - l.cnt_a);   // cnt_a and cnt_b
    hipLaunchKernelGGL((k_fbp_zero<CFG>), dim3(blocks_for(nab, 256)),
                       dim3(256), 0, st, cnt_a, nab);
    hipLaunchKernelGGL((k_fbp_zero<CFG>),
                       dim3(blocks_for((size_t)G::NBUCKETS + 1, 256)),
                       dim3(256), 0, st, cnt_c, G::NBUCKETS + 1);
    // pass A: scalars -> (u16, u32) in NBIN_A bins
    hipLaunchKernelGGL((k_fbp_count_a<CFG>),
                       dim3(blocks_for(p->n, FBP_BLOCK * FBP_A_SPT)),
                       dim3(FBP_BLOCK), 0, st, p->d_scalars, p->d_inf, p->n,
                       cnt_a);
    EM_HT(scan(cnt_a, off_a, (size_t)G::NBIN_A + 1));
    hipLaunchKernelGGL((k_fbp_scatter_a<CFG>),
                       dim3(blocks_for(p->n, FBP_BLOCK)), dim3(FBP_BLOCK), 0,
                       st, p->d_scalars, p->d_inf, p->n, cnt_a, off_a, k16, v1);
    // pass B: regions = pass A's bins -> (u8, u32)
    EM_HT(units(off_a, G::NREG_B));
    const dim3 grid_b(fbp_grid(total, T, G::NREG_B));
    hipLaunchKernelGGL((k_fbp_count<uint16_t, FBP_SHIFT_B>), grid_b,
                       dim3(FBP_BLOCK), 0, st, k16, off_a, uoff, G::NREG_B, T,
                       cnt_b);
    EM_HT(scan(cnt_b, off_b, (size_t)G::NREG_C + 1));
    hipLaunchKernelGGL((k_fbp_scatter<uint16_t, uint8_t, FBP_SHIFT_B, true>),
                       grid_b, dim3(FBP_BLOCK), (size_t)T * 6, st, k16, v1,
                       off_a, uoff, G::NREG_B, T, cnt_b, off_b, k8, v2);
    // pass C: regions = pass B's bins -> values; its scan is d_fb_boff
    EM_HT(units(off_b, G::NREG_C));
    const dim3 grid_c(fbp_grid(total, T, G::NREG_C));
    hipLaunchKernelGGL((k_fbp_count<uint8_t, FBP_SHIFT_C>), grid_c,
                       dim3(FBP_BLOCK), 0, st, k8, off_b, uoff, G::NREG_C, T,
                       cnt_c);
    EM_HT(scan(cnt_c, p->d_fb_boff, (size_t)G::NBUCKETS + 1));
    hipLaunchKernelGGL((k_fbp_scatter<uint8_t, uint8_t, FBP_SHIFT_C, false>),
                       grid_c, dim3(FBP_BLOCK), (size_t)T * 5, st, k8, v2,
                       off_b, uoff, G::NREG_C, T, cnt_c, p->d_fb_boff,
                       (uint8_t *)nullptr, b.vals_out);
    return hipSuccess;
}

// Stage 1, sort chain: scalar digits -> radix sort by bucket -> bucket
// offsets -> length-sorted walk schedule (kills wave divergence in the walk).
template <typename C, typename CFG>
static hipError_t msm_enqueue_sort_chain(msm_plan_t<C> *p, int par,
                                         hipStream_t st) {
    const msm_step_bufs &b = p->sb[par];
    size_t tmp = p->sort_tmp_bytes;
    if constexpr (is_fbm<CFG>::value) {
        // merged fixed-base: digits of all windows -> ONE radix sort over
        // the c-1 id bits -> bucket offsets -> runs cut into slots of <=
        // fb_chunk entries (counts, exclusive scan, refined offsets)
        const size_t total = p->n * (size_t)CFG::NWIN_REAL;
        constexpr uint32_t NB = CFG::NBUCKETS, NS = CFG::NSLOT;
        uint32_t *coff = p->d_loff[par];
        if (p->fbp_tile) {
            EM_HT((fbm_enqueue_partition<C, CFG>(p, par, st)));
        } else {
            hipLaunchKernelGGL((k_fbm_digits<CFG>),
                               dim3(blocks_for(p->n, 256)), dim3(256), 0, st,
                               p->d_scalars, p->d_inf, p->d_keys, p->d_vals,
                               p->n);
            EM_HT(rocprim::radix_sort_pairs(p->d_sort_tmp, tmp, p->d_keys,
                                            b.keys_out, p->d_vals, b.vals_out,
                                            total, 0, CFG::SORT_BITS, st));
            hipLaunchKernelGGL((k_offsets<CFG>),
                               dim3(blocks_for((size_t)NB + 1, 256)),
                               dim3(256), 0, st, b.keys_out, total,
                               p->d_fb_boff);
        }
        hipLaunchKernelGGL((k_fbm_chunk_counts<CFG>),
                           dim3(blocks_for((size_t)NB + 1, 256)), dim3(256), 0,
                           st, p->d_fb_boff, p->d_cnt, p->fb_chunk);
        size_t stmp = p->scan_tmp_bytes;
        EM_HT(rocprim::exclusive_scan(p->d_scan_tmp, stmp, p->d_cnt, coff, 0u,
                                      (size_t)NB + 1,
                                      rocprim::plus<uint32_t>(), st));
        hipLaunchKernelGGL((k_fbm_slot_offsets<CFG>),
                           dim3(blocks_for((size_t)NS + 1, 256)), dim3(256), 0,
                           st, p->d_fb_boff, coff, b.offsets, p->fb_chunk,
                           (uint32_t)total);
        hipLaunchKernelGGL((k_bucket_lengths<CfgFbmWalk>), dim3(NS / 256),
                           dim3(256), 0, st, b.offsets, p->d_blen, p->d_bids);
        tmp = p->sort_tmp_bytes;
        EM_HT(rocprim::radix_sort_pairs(p->d_sort_tmp, tmp, p->d_blen,
                                        p->d_blen_out, p->d_bids, b.sched,
                                        (size_t)NS, 0, p->fb_len_bits, st));
    } else {
        constexpr bool FB = std::is_same_v<CFG, CfgFB>;
        const size_t total = p->n * (size_t)(FB ? FB_NWIN : CFG::NWIN);
        const bool k16 = !FB && p->keys16;
        if constexpr (FB) {
            hipLaunchKernelGGL(k_fb_digits, dim3(blocks_for(total, 256)),
                               dim3(256), 0, st, p->d_scalars, p->d_inf,
                               p->d_keys, p->d_vals, p->n);
        } else if (p->keys16) {
            hipLaunchKernelGGL((k_digits<CFG, uint16_t>),
                               dim3(blocks_for(p->n, 256)), dim3(256), 0, st,
                               p->d_scalars, p->d_inf, (uint16_t *)p->d_keys,
                               p->d_vals, p->n);
        } else {
            hipLaunchKernelGGL((k_digits<CFG>), dim3(blocks_for(p->n, 256)),
                               dim3(256), 0, st, p->d_scalars, p->d_inf,
                               p->d_keys, p->d_vals, p->n);
        }
        // The window bits of a key are constant within each window's segment
        // [w*n, (w+1)*n), so for large MSMs NWIN per-window sorts over just
        // the digit bits replace one global sort over digit+window bits — one
        // fewer radix pass over the full pair array.  Small MSMs keep the
        // single sort (per-call overhead dominates at small n).
        if (k16) {
            for (int w = 0; w < CFG::NWIN; w++) {
                tmp = p->sort_tmp_bytes;
                size_t off = (size_t)w * p->n;
                EM_HT(rocprim::radix_sort_pairs(
                    p->d_sort_tmp, tmp, (const uint16_t *)p->d_keys + off,
                    (uint16_t *)b.keys_out + off, p->d_vals + off,
                    b.vals_out + off, p->n, 0, CFG::DBITS, st));
            }
            hipLaunchKernelGGL(
                (k_offsets_seg<CFG>),
                dim3(blocks_for((size_t)CFG::NBUCKETS + 1, 256)), dim3(256), 0,
                st, (const uint16_t *)b.keys_out, p->n, b.offsets);
        } else {
            EM_HT(rocprim::radix_sort_pairs(p->d_sort_tmp, tmp, p->d_keys,
                                            b.keys_out, p->d_vals, b.vals_out,
                                            total, 0, CFG::SORT_BITS, st));
            hipLaunchKernelGGL(
                (k_offsets<CFG>),
                dim3(blocks_for((size_t)CFG::NBUCKETS + 1, 256)), dim3(256), 0,
                st, b.keys_out, total, b.offsets);
        }
        hipLaunchKernelGGL((k_bucket_lengths<CFG>),
                           dim3(blocks_for(CFG::NBUCKETS, 256)), dim3(256), 0,
                           st, b.offsets, p->d_blen, p->d_bids);
        tmp = p->sort_tmp_bytes;
        EM_HT(rocprim::radix_sort_pairs(p->d_sort_tmp, tmp, p->d_blen,
                                        p->d_blen_out, p->d_bids, b.sched,
                                        (size_t)CFG::NBUCKETS, 0, 32, st));
    }
    return hipSuccess;
}

// Stage 2, walk: one thread per scheduled bucket (merged mode: per slot of
// the table), XYZZ accumulation with the lazy signed add.  `mid` is the
// EM_MSM_SPLIT experiment: when set, the window walk launches as two
// segments with `mid` recorded between them (after the walk if the split
// point degenerates); it is never set under capture.
template <typename C, typename CFG>
static hipError_t msm_enqueue_walk(msm_plan_t<C> *p, int par, hipStream_t st,
                                   hipEvent_t mid = nullptr) {
    const msm_step_bufs &b = p->sb[par];
    const g1aT<C> *pts = msm_walk_pts<C, CFG>(p);
    if constexpr (is_fbm<CFG>::value) {
        hipLaunchKernelGGL((k_bucket_acc<C, CfgFbmWalk>),
                           dim3(CFG::NSLOT / 256), dim3(256), 0, st, pts,
                           b.vals_out, b.offsets, b.sched, p->d_fb_slots, 0u);
    } else {
        constexpr uint32_t NB = CFG::NBUCKETS;
        auto walk = [&](uint32_t count, uint32_t base) {
            hipLaunchKernelGGL((k_bucket_acc<C, CFG>),
                               dim3(blocks_for(count, 256)), dim3(256), 0, st,
                               pts, b.vals_out, b.offsets, b.sched,
                               p->d_buckets, base);
        };
        uint32_t head = NB;
        if (mid) {
            uint32_t pct = (uint32_t)msm_split_pct();
            uint32_t cut = (uint32_t)(((uint64_t)NB * pct) / 100) / 256 * 256;
            if (cut != 0 && cut < NB) head = cut;
        }
        walk(head, 0u);
        if (mid) EM_HT(hipEventRecord(mid, st));
        if (head < NB) walk(NB - head, head);
    }
    return hipSuccess;
}

// Stage 2, alternate (EM_MSM_TREE experiment; sync path, BN254 G1 unsigned
// c=16 only): batch-affine pairing tree over the sorted runs, then the XYZZ
// walk over the last level cleans up the short tails.
template <typename C, typename CFG>
static hipError_t msm_enqueue_tree_walk(msm_plan_t<C> *p, int par,
                                        hipStream_t st) {
    const msm_step_bufs &b = p->sb[par];
    constexpr uint32_t NB = CFG::NBUCKETS;
    const size_t total = p->n * (size_t)CFG::NWIN;
    const uint32_t cap = (uint32_t)(total / 2 + NB + 1);
    const uint32_t *o_in = b.offsets;
    size_t bound = total;
    for (int l = 0; l < p->tree_levels; l++) {
        uint32_t *o_out = p->d_loff[l & 1];
        hipLaunchKernelGGL(k_pair_counts, dim3(blocks_for((size_t)NB + 1, 256)),
                           dim3(256), 0, st, o_in, p->d_cnt, NB, CFG::DMASK,
                           l == 0 ? 1 : 0);
        size_t stmp = p->scan_tmp_bytes;
        EM_HT(rocprim::exclusive_scan(p->d_scan_tmp, stmp, p->d_cnt, o_out, 0u,
                                      (size_t)NB + 1,
                                      rocprim::plus<uint32_t>(), st));
        size_t pbound = bound / 2 + NB;
        size_t nthreads = (pbound + PAIR_K - 1) / PAIR_K;
        g1aT<C> *dst = p->d_lvl[l & 1];
        if (l == 0) {
            hipLaunchKernelGGL((k_pair_level<C, true>),
                               dim3(blocks_for(nthreads, 256)), dim3(256), 0,
                               st, p->d_pts, b.vals_out, o_in, o_out, p->d_aux,
                               cap, dst, NB);
        } else {
            hipLaunchKernelGGL((k_pair_level<C, false>),
                               dim3(blocks_for(nthreads, 256)), dim3(256), 0,
                               st, p->d_lvl[(l & 1) ^ 1], nullptr, o_in, o_out,
                               p->d_aux, cap, dst, NB);
        }
        o_in = o_out;
        bound = pbound;
    }
    hipLaunchKernelGGL((k_bucket_acc<C, CFG, false>),
                       dim3(blocks_for(NB, 256)), dim3(256), 0, st,
                       p->d_lvl[(p->tree_levels - 1) & 1], nullptr, o_in,
                       b.sched, p->d_buckets);
    return hipSuccess;
}

// Stage 3, reduce: buckets -> per-window sums (merged mode first folds the
// walk's slots back into buckets; both fixed-base modes reduce NWIN = 1)
template <typename C, typename CFG>
static void msm_enqueue_reduce(msm_plan_t<C> *p, int par, hipStream_t st) {
    if constexpr (is_fbm<CFG>::value) {
        hipLaunchKernelGGL((k_fbm_combine_groups<C, CFG>),
                           dim3(CFG::NSLOT / 256), dim3(256), 0, st,
                           p->d_loff[par], p->d_fb_slots);
        hipLaunchKernelGGL((k_fbm_combine_buckets<C, CFG>),
                           dim3(blocks_for(CFG::NBUCKETS, 256)), dim3(256), 0,
                           st, p->d_loff[par], p->d_fb_slots, p->d_buckets);
    }
    hipLaunchKernelGGL((k_segment_reduce<C, CFG>),
                       dim3(blocks_for(CFG::NWIN * CFG::NSEG, 256)), dim3(256),
                       0, st, p->d_buckets, p->d_seg_sum, p->d_seg_wsum);
    hipLaunchKernelGGL((k_weighted_reduce<C, CFG>),
                       dim3(blocks_for(CFG::NWIN * CFG::NSEG, CFG::RED_BLOCK)),
                       dim3(CFG::RED_BLOCK), 0, st, p->d_seg_sum,
                       p->d_seg_wsum, p->d_partials);
    hipLaunchKernelGGL((k_window_sum<C, CFG>), dim3(CFG::NWIN), dim3(64), 0,
                       st, p->d_partials, p->d_windows);
}

// Stage 4, emit: the CFG::NWIN unscaled window sums as Jacobian wire
// records for the host Horner
template <typename C, typename CFG>
static void msm_enqueue_emit(msm_plan_t<C> *p, int par, hipStream_t st) {
    hipLaunchKernelGGL((k_emit_windows<C, CFG>), dim3(1), dim3(64), 0, st,
                       p->d_windows, p->sb[par].out);
}

// sync path (run / run_partial), after msm_sync_t has drained the pipeline:
// the stages at parity 0 on the null stream, the phase events between them
template <typename C, typename CFG>
static int msm_run_sync_cfg(msm_plan_t<C> *p, uint8_t *out, int out_mode) {
    constexpr int JB = msm_plan_t<C>::JB;
    HIP_TRY(hipEventRecord(p->ev[0], 0));
    hipError_t e = msm_enqueue_sort_chain<C, CFG>(p, 0, 0);
    if (e != hipSuccess) return hip_fail(e, "sort chain");
    HIP_TRY(hipEventRecord(p->ev[1], 0));
    bool tree_done = false;
    if constexpr (std::is_same_v<C, Bn254G1> && std::is_same_v<CFG, CfgL254>) {
        if (p->use_tree) {
            e = msm_enqueue_tree_walk<C, CFG>(p, 0, 0);
            tree_done = true;
        }
    }
    if (!tree_done) e = msm_enqueue_walk<C, CFG>(p, 0, 0);
    if (e != hipSuccess) return hip_fail(e, "bucket walk");
    HIP_TRY(hipEventRecord(p->ev[2], 0));
    msm_enqueue_reduce<C, CFG>(p, 0, 0);
    HIP_TRY(hipEventRecord(p->ev[3], 0));
    msm_enqueue_emit<C, CFG>(p, 0, 0);
    HIP_TRY(hipEventRecord(p->ev[4], 0));
    uint8_t wire[CFG::NWIN * JB];
    HIP_TRY(hipMemcpy(wire, p->sb[0].out, sizeof wire, hipMemcpyDeviceToHost));
    host_windows_horner<C>(wire, CFG::NWIN, CFG::C, out, out_mode);
    HIP_TRY(hipDeviceSynchronize());
    // digits+sort, walk, reduce, emit, total
    const int a[5] = {0, 1, 2, 3, 0}, b[5] = {1, 2, 3, 4, 4};
    for (int i = 0; i < 5; i++) {
        float ms;
        HIP_TRY(hipEventElapsedTime(&ms, p->ev[a[i]], p->ev[b[i]]));
        p->last_ms[i] = ms;
    }
    return EM_OK;
}

// capture one chain as a hipGraph on `st` and instantiate it
template <typename F>
static int msm_capture_graph(hipStream_t st, hipGraphExec_t *exec, F enqueue,
                             const char *what) {
    hipGraph_t g = nullptr;
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    hipError_t ec = enqueue();
    hipError_t e2 = hipStreamEndCapture(st, &g);
    if (ec != hipSuccess || e2 != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        return hip_fail(ec != hipSuccess ? ec : e2, what);
    }
    hipError_t e3 = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e3 != hipSuccess) return hip_fail(e3, what);
    return EM_OK;
}

// one pipelined step: sort chain on s_sort (buffers chosen by step parity),
// compute chain (walk, reduce, emit) on s_comp ordered behind it by event.
// Returns after ENQUEUE; the result lands in `out` by the time msm_sync (or
// the depth-2 backpressure of a later run_async) returns.  The proving loop
// runs many MSMs back-to-back, so steady-state cost = max(sort chain,
// compute chain) instead of their sum.
//
// A step is ~70 dispatches (15 per-window rocPRIM sorts alone), so by
// default both chains are CAPTURED per parity as hipGraphs and replayed
// as two graph launches — the measured async-over-compute-chain gap was
// host dispatch pacing.  All pointers are parity-fixed; graphs rebuild if
// the point table changes (fixed-base precompute).  EM_MSM_GRAPH=0
// disables; the EM_MSM_SPLIT gate experiment implies the direct path, and
// so does the tree experiment (which then runs the plain XYZZ walk here).
template <typename C, typename CFG>
static int msm_run_async_cfg(msm_plan_t<C> *p, uint8_t *out, int out_mode) {
    const g1aT<C> *pts = msm_walk_pts<C, CFG>(p);
    int par = p->apar;
    int rc = msm_deliver(p, par);  // free this parity's slots (step k-2)
    if (rc) return rc;
    hipStream_t ss = p->s_sort, sc = p->s_comp;
    static bool graph_on = std::getenv("EM_MSM_GRAPH")
                               ? atoi(std::getenv("EM_MSM_GRAPH")) != 0
                               : true;
    const bool split_on = msm_split_pct() > 0;
    bool use_graph = graph_on && !split_on && !p->use_tree;
    // ev_walkA[par] gates the NEXT step's sort chain.  Gate off (A/B-measured
    // default: gating the sorts on part of the walk only LOST time — the
    // async gap is host pacing, which the graph path removes instead): it is
    // recorded before the walk.  EM_MSM_SPLIT: the window walk records it.
    hipEvent_t mid =
        split_on && !is_fbm<CFG>::value ? p->ev_walkA[par] : nullptr;
    auto comp_chain = [&](hipEvent_t m) -> hipError_t {
        EM_HT((msm_enqueue_walk<C, CFG>(p, par, sc, m)));
        msm_enqueue_reduce<C, CFG>(p, par, sc);
        msm_enqueue_emit<C, CFG>(p, par, sc);
        return hipSuccess;
    };
    HIP_TRY(hipStreamWaitEvent(ss, p->ev_comp_done[par], 0));
    // contention gate: wait for the PREVIOUS step's walk segment A
    HIP_TRY(hipStreamWaitEvent(ss, p->ev_walkA[par ^ 1], 0));
    if (use_graph &&
        (p->gx_sort[par] == nullptr || p->gx_pts[par] != (const void *)pts)) {
        if (p->gx_sort[par]) {
            (void)hipGraphExecDestroy(p->gx_sort[par]);
            p->gx_sort[par] = nullptr;
        }
        if (p->gx_comp[par]) {
            (void)hipGraphExecDestroy(p->gx_comp[par]);
            p->gx_comp[par] = nullptr;
        }
        rc = msm_capture_graph(
            ss, &p->gx_sort[par],
            [&]() { return msm_enqueue_sort_chain<C, CFG>(p, par, ss); },
            "sort-chain graph capture");
        if (rc) return rc;
        rc = msm_capture_graph(
            sc, &p->gx_comp[par], [&]() { return comp_chain(nullptr); },
            "compute-chain graph capture");
        if (rc) return rc;
        p->gx_pts[par] = (const void *)pts;
    }
    // ---- sort chain ----
    if (use_graph) {
        HIP_TRY(hipGraphLaunch(p->gx_sort[par], ss));
    } else {
        hipError_t ec = msm_enqueue_sort_chain<C, CFG>(p, par, ss);
        if (ec != hipSuccess) return hip_fail(ec, "sort chain (async)");
    }
    HIP_TRY(hipEventRecord(p->ev_sort_done[par], ss));
    // ---- compute chain ----
    HIP_TRY(hipStreamWaitEvent(sc, p->ev_sort_done[par], 0));
    if (!mid) HIP_TRY(hipEventRecord(p->ev_walkA[par], sc));
    if (use_graph) {
        HIP_TRY(hipGraphLaunch(p->gx_comp[par], sc));
    } else {
        hipError_t ec = comp_chain(mid);
        if (ec != hipSuccess) return hip_fail(ec, "compute chain (async)");
    }
    HIP_TRY(hipMemcpyAsync(p->h_out[par], p->sb[par].out,
                           (size_t)CFG::NWIN * msm_plan_t<C>::JB,
                           hipMemcpyDeviceToHost, sc));
    HIP_TRY(hipEventRecord(p->ev_comp_done[par], sc));
    p->pend[par] = {out, out_mode, CFG::NWIN, CFG::C, true};
    p->apar ^= 1;
    return EM_OK;
}

template <typename C>
static int msm_run_async_t(msm_plan_t<C> *p, uint8_t *out, int out_mode = 0) {
    if (!p || !out) return EM_ERR_INPUT;
    if (!p->have_points || !p->have_scalars) {
        g_last_err = "msm_run_async: points/scalars not uploaded";
        return EM_ERR_INPUT;
    }
    return msm_with_cfg(p, [&](auto cfg) {
        return msm_run_async_cfg<C, decltype(cfg)>(p, out, out_mode);
    });
}

template <typename C>
static int msm_run_inner_t(msm_plan_t<C> *p, uint8_t *out, int out_mode) {
    if (!p || !out) return EM_ERR_INPUT;
    if (!p->have_points || !p->have_scalars) {
        g_last_err = "msm_run: points/scalars not uploaded";
        return EM_ERR_INPUT;
    }
    int rc = msm_sync_t(p);  // drain any pipelined steps first
    if (rc) return rc;
    return msm_with_cfg(p, [&](auto cfg) {
        return msm_run_sync_cfg<C, decltype(cfg)>(p, out, out_mode);
    });
}

// opaque ABI types
struct em_msm_plan : msm_plan_t<Bn254G1> {};
struct em_bls_msm_plan : msm_plan_t<BlsG1> {};
struct em_bls_g2_msm_plan : msm_plan_t<BlsG2> {};

// generic 1-thread op runner: in_bytes staged, out_bytes copied back
template <typename K>
static int run_single(K kern, const uint8_t *a, size_t la, const uint8_t *b,
                      size_t lb, uint8_t *out, size_t lo) {
    int rc = require_gpu();
    if (rc) return rc;
    uint8_t *d_in, *d_out;
    uint32_t *d_err;
    HIP_TRY(hipMalloc(&d_in, la + lb));
    HIP_TRY(hipMalloc(&d_out, lo));
    HIP_TRY(hipMalloc(&d_err, 4));
    HIP_TRY(hipMemset(d_err, 0, 4));
    HIP_TRY(hipMemcpy(d_in, a, la, hipMemcpyHostToDevice));
    if (lb) HIP_TRY(hipMemcpy(d_in + la, b, lb, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, 0, d_in, d_out, d_err);
    uint32_t err;
    HIP_TRY(hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost));
    if (!err) HIP_TRY(hipMemcpy(out, d_out, lo, hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_err);
    if (err & 2u) return EM_ERR_INPUT;
    return err ? EM_ERR_POINT : EM_OK;
}
