// Host check of the merged fixed-base bucket partition's index arithmetic
// (csrc/msm_fbm_partition.h).  Emulates the three passes on the CPU the way
// the kernels run them: per-unit histograms flushed into cnt[region*256 +
// bin], an exclusive scan, one range reservation per non-empty bin per unit
// (counting cnt down), units found with fbp_region_of / fbp_unit_range on a
// grid of fbp_grid blocks.  Units run in a shuffled order, as blocks may.
//
// Inputs: random keys, all-equal keys, all-zero keys, keys < 1024 only and
// the maximum key only; each at T in {1, 7, 256} and c in {20, 22, 24}.
// Asserted: every write stays inside its bin's range and hits a free slot,
// the output is a permutation of the input values grouped by key, the
// offsets equal the prefix counts, every unit lies within the grid bound,
// and all counters are back at zero.
//
//   hipcc -x hip --offload-host-only -O2 -std=c++17 -I ../csrc \
//         fbm_partition_check.cpp -o fbm_partition_check
//
// Exit status 0 = all cases agree; prints one "c=<c> ok" line per geometry.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <hip/hip_runtime.h>

#include "msm_fbm_partition.h"

using namespace em;
typedef uint64_t u64;

static u64 rng_s = 0x9e3779b97f4a7c15ull;
static u64 rnd() {
    rng_s ^= rng_s << 13;
    rng_s ^= rng_s >> 7;
    rng_s ^= rng_s << 17;
    return rng_s;
}

static int g_fail = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::fprintf(stderr, "FAIL ");    \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");       \
            if (++g_fail > 20) std::exit(1);  \
        }                                     \
    } while (0)

static std::vector<uint32_t> excl_scan(const std::vector<uint32_t> &v) {
    std::vector<uint32_t> o(v.size());
    uint32_t run = 0;
    for (size_t i = 0; i < v.size(); i++) {
        o[i] = run;
        run += v[i];
    }
    return o;
}

struct pairs {
    std::vector<uint32_t> key, val;   // key: what this pass still has to sort
};

// the unit list of a pass: (region, lo, hi) for every block of the grid that
// owns a unit, in shuffled order
struct unit {
    uint32_t r, lo, hi;
};
static std::vector<unit> make_units(const std::vector<uint32_t> &off,
                                    uint32_t regions, uint32_t T,
                                    size_t total, const char *what) {
    std::vector<uint32_t> ucnt(regions + 1, 0);
    for (uint32_t r = 0; r < regions; r++)
        ucnt[r] = fbp_units(off[r + 1] - off[r], T);
    std::vector<uint32_t> uoff = excl_scan(ucnt);
    const uint32_t grid = fbp_grid(total, T, regions);
    CHECK(uoff[regions] <= grid, "%s: %u units > grid %u", what, uoff[regions],
          grid);
    std::vector<unit> us;
    size_t covered = 0;
    for (uint32_t u = 0; u < grid; u++) {
        if (u >= uoff[regions]) continue;   // surplus block
        unit x;
        x.r = fbp_region_of(uoff.data(), regions, u);
        CHECK(x.r < regions && uoff[x.r] <= u && u < uoff[x.r + 1],
              "%s: unit %u -> region %u", what, u, x.r);
        if (x.r >= regions) continue;
        fbp_unit_range(off.data(), uoff.data(), x.r, u, T, x.lo, x.hi);
        CHECK(x.lo < x.hi && x.hi - x.lo <= T && x.lo >= off[x.r] &&
                  x.hi <= off[x.r + 1],
              "%s: unit %u range [%u, %u)", what, u, x.lo, x.hi);
        covered += x.hi - x.lo;
        us.push_back(x);
    }
    CHECK(covered == total, "%s: units cover %zu of %zu", what, covered, total);
    for (size_t i = us.size(); i > 1; i--)
        std::swap(us[i - 1], us[rnd() % i]);
    return us;
}

// one count -> scan -> scatter pass over `in`, split at bit SHIFT; `off` are
// the region bounds (regions + 1), `off_out` receives the scan of the
// regions * nbin bin counts (+ 1 entry = total)
template <int SHIFT>
static pairs run_pass(const pairs &in, const std::vector<uint32_t> &off,
                      uint32_t regions, uint32_t nbin, uint32_t T,
                      std::vector<uint32_t> &off_out, const char *what) {
    const size_t total = in.key.size();
    std::vector<unit> us = make_units(off, regions, T, total, what);
    std::vector<uint32_t> cnt((size_t)regions * nbin + 1, 0);
    std::vector<uint32_t> lh(nbin);
    for (const unit &x : us) {
        std::fill(lh.begin(), lh.end(), 0u);
        for (uint32_t j = x.lo; j < x.hi; j++) {
            uint32_t b = fbp_bin<SHIFT>(in.key[j]);
            CHECK(b < nbin, "%s: bin %u", what, b);
            if (b < nbin) lh[b]++;
        }
        for (uint32_t b = 0; b < nbin; b++) cnt[(size_t)x.r * nbin + b] += lh[b];
    }
    off_out = excl_scan(cnt);
    pairs out;
    out.key.assign(total, 0);
    out.val.assign(total, 0);
    std::vector<uint8_t> used(total, 0);
    std::vector<uint32_t> start(nbin);
    for (size_t i = us.size(); i > 1; i--)
        std::swap(us[i - 1], us[rnd() % i]);
    for (const unit &x : us) {
        std::fill(lh.begin(), lh.end(), 0u);
        for (uint32_t j = x.lo; j < x.hi; j++)
            lh[fbp_bin<SHIFT>(in.key[j]) % nbin]++;
        for (uint32_t b = 0; b < nbin; b++) {
            if (!lh[b]) continue;
            size_t g = (size_t)x.r * nbin + b;
            CHECK(cnt[g] >= lh[b], "%s: counter underflow", what);
            cnt[g] -= lh[b];                 // atomicSub: old - mine
            start[b] = off_out[g] + cnt[g];
        }
        for (uint32_t j = x.lo; j < x.hi; j++) {
            uint32_t b = fbp_bin<SHIFT>(in.key[j]) % nbin;
            size_t g = (size_t)x.r * nbin + b;
            uint32_t dst = start[b]++;
            bool ok = dst >= off_out[g] && dst < off_out[g + 1] && !used[dst];
            CHECK(ok, "%s: write %u outside bin [%u, %u) or taken", what, dst,
                  off_out[g], off_out[g + 1]);
            if (!ok) continue;
            used[dst] = 1;
            out.key[dst] = fbp_low<SHIFT>(in.key[j]);
            out.val[dst] = in.val[j];
        }
    }
    for (uint32_t c : cnt) CHECK(c == 0, "%s: counter left at %u", what, c);
    return out;
}

template <typename G>
static void check_input(const std::vector<uint32_t> &keys, uint32_t T,
                        const char *what) {
    const uint32_t total = (uint32_t)keys.size();
    pairs in;
    in.key = keys;
    in.val.resize(total);
    for (uint32_t i = 0; i < total; i++) in.val[i] = i;
    // pass A: one region (the whole input); the kernel's units are blocks of
    // scalars, here chunks of T entries
    std::vector<uint32_t> off0 = {0u, total}, off_a, off_b, boff;
    pairs a = run_pass<FBP_SHIFT_A>(in, off0, 1, G::NBIN_A, T, off_a, "pass A");
    pairs b = run_pass<FBP_SHIFT_B>(a, off_a, G::NREG_B, 256, T, off_b, "pass B");
    pairs c = run_pass<FBP_SHIFT_C>(b, off_b, G::NREG_C, 256, T, boff, "pass C");
    CHECK(boff.size() == (size_t)G::NBUCKETS + 1, "%s: offsets size", what);
    // offsets equal the prefix counts
    std::vector<uint32_t> want(G::NBUCKETS + 1, 0);
    for (uint32_t k : keys) want[k]++;
    want = excl_scan(want);
    CHECK(want == boff, "%s T=%u: offsets differ from prefix counts", what, T);
    // a permutation of the values, grouped by key
    std::vector<uint8_t> seen(total, 0);
    for (uint32_t bkt = 0; bkt < G::NBUCKETS; bkt++) {
        for (uint32_t j = boff[bkt]; j < boff[bkt + 1] && j < total; j++) {
            uint32_t v = c.val[j];
            CHECK(v < total && !seen[v], "%s T=%u: value %u repeated", what, T,
                  v);
            if (v >= total) continue;
            seen[v] = 1;
            CHECK(keys[v] == bkt, "%s T=%u: value %u (key %u) in bucket %u",
                  what, T, v, keys[v], bkt);
        }
    }
    for (uint32_t i = 0; i < total; i++)
        CHECK(seen[i], "%s T=%u: value %u missing", what, T, i);
}

template <typename CFG>
static void check_cfg() {
    using G = fbp_geom<CFG::IB>;
    static_assert(G::NBUCKETS == CFG::NBUCKETS, "geometry");
    const uint32_t n = 5000;
    const int before = g_fail;
    for (uint32_t T : {1u, 7u, 256u}) {
        std::vector<uint32_t> k(n);
        for (auto &x : k) x = (uint32_t)rnd() & CFG::DMASK;
        check_input<G>(k, T, "random");
        std::fill(k.begin(), k.end(), 0x2a5a5u & CFG::DMASK);
        check_input<G>(k, T, "all equal");
        std::fill(k.begin(), k.end(), 0u);
        check_input<G>(k, T, "all zero");
        for (auto &x : k) x = (uint32_t)rnd() & 1023u;
        check_input<G>(k, T, "keys < 1024");
        std::fill(k.begin(), k.end(), CFG::DMASK);
        check_input<G>(k, T, "maximum key");
        check_input<G>(std::vector<uint32_t>(1, 5u), T, "one entry");
    }
    if (g_fail == before) std::printf("c=%d ok\n", CFG::C);
}

int main() {
    check_cfg<CfgFbm20>();
    check_cfg<CfgFbm22>();
    check_cfg<CfgFbm24>();
    if (g_fail) {
        std::fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    std::printf("all cases agree\n");
    return 0;
}
