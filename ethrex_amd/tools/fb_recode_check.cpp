// Host check of the merged fixed-base digit recode (csrc/msm_fb_recode.h).
// For c in {20, 22, 24} the signed digits d_w of every scalar k < r must
// satisfy  sum_w d_w * 2^(c*w) == k  exactly, |d_w| <= 2^(c-1), and the
// top window must not carry out.  10^5 random scalars below r plus the
// edge set (0, 1, r-1, 2^(c-1), 2^(c-1)+1, 2^c-1, every full window
// 2^(c-1), every full window 2^c-1, ...).
//
//   hipcc -x hip --offload-host-only -O2 -std=c++17 -I ../csrc \
//         fb_recode_check.cpp -o fb_recode_check
//
// Exit status 0 = all cases agree; prints one "c=<c> ok" line per geometry.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "msm_fb_recode.h"

using namespace em;
typedef uint64_t u64;

// BN254 scalar field modulus r, little-endian u64 limbs
static const u64 R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull,
                         0xb85045b68181585dull, 0x30644e72e131a029ull};

struct k256 {
    u64 v[4];
};

static u64 rng_s = 0x9e3779b97f4a7c15ull;
static u64 rnd() {
    rng_s ^= rng_s << 13;
    rng_s ^= rng_s >> 7;
    rng_s ^= rng_s << 17;
    return rng_s;
}

static bool lt_r(const k256 &k) {
    for (int i = 3; i >= 0; i--) {
        if (k.v[i] < R[i]) return true;
        if (k.v[i] > R[i]) return false;
    }
    return false;
}

// acc (5 limbs, two's complement) += / -= mag << sh
static void acc_shifted(u64 acc[5], uint32_t mag, int sh, bool sub) {
    u64 t[5] = {0, 0, 0, 0, 0};
    int limb = sh >> 6, off = sh & 63;
    t[limb] = (u64)mag << off;
    if (off != 0 && limb + 1 < 5) t[limb + 1] = (u64)mag >> (64 - off);
    unsigned __int128 c = sub ? 1 : 0;
    for (int i = 0; i < 5; i++) {
        c += (unsigned __int128)acc[i] + (sub ? ~t[i] : t[i]);
        acc[i] = (u64)c;
        c >>= 64;
    }
}

static int g_fail = 0;

template <typename CFG>
static void check_one(const k256 &k, const char *what) {
    u64 acc[5] = {0, 0, 0, 0, 0};
    uint32_t carry = 0;
    for (int w = 0; w < CFG::NWIN_REAL; w++) {
        uint32_t neg = 0;
        uint32_t mag =
            fbm_recode_step<CFG::C>(fbm_digit<CFG::C>(k.v, w), carry, neg);
        if (mag > (1u << (CFG::C - 1))) {
            std::fprintf(stderr, "FAIL c=%d %s: |d| > 2^(c-1) at w=%d\n",
                         CFG::C, what, w);
            g_fail++;
        }
        // raw = 2^c - 1 with a carry in gives t = 2^c: digit 0, carry out
        // (mag 0 with neg set; the digit kernel parks it as a skip)
        acc_shifted(acc, mag, CFG::C * w, neg != 0);
    }
    if (carry) {
        std::fprintf(stderr, "FAIL c=%d %s: top window carried out\n", CFG::C,
                     what);
        g_fail++;
    }
    if (acc[4] != 0 || std::memcmp(acc, k.v, 32) != 0) {
        std::fprintf(stderr, "FAIL c=%d %s: digits do not rebuild the scalar\n",
                     CFG::C, what);
        g_fail++;
    }
    if (g_fail > 20) std::exit(1);
}

static k256 small(u64 x) { return k256{{x, 0, 0, 0}}; }

static void set_bits(k256 &k, int bit, u64 val, int nbits) {
    for (int b = 0; b < nbits; b++)
        if ((val >> b) & 1) k.v[(bit + b) >> 6] |= 1ull << ((bit + b) & 63);
}

template <typename CFG>
static void check_cfg() {
    constexpr int C = CFG::C, NW = CFG::NWIN_REAL;
    std::vector<k256> edge;
    edge.push_back(small(0));
    edge.push_back(small(1));
    k256 rm1{{R[0] - 1, R[1], R[2], R[3]}};
    edge.push_back(rm1);
    edge.push_back(small(1ull << (C - 1)));
    edge.push_back(small((1ull << (C - 1)) + 1));
    edge.push_back(small((1ull << C) - 1));
    // every full window 2^(c-1) / 2^(c-1)+1 / 2^c-1 (carry through every
    // window into the top one); the top window keeps its largest value
    // below r's top bits on the last two
    const u64 pat[3] = {1ull << (C - 1), (1ull << (C - 1)) + 1,
                        (1ull << C) - 1};
    const u64 rtop = R[3] >> ((C * (NW - 1)) - 192);   // r's top window
    for (int t = 0; t < 3; t++) {
        for (u64 top : {(u64)0, rtop - 1}) {
            k256 k = small(0);
            for (int w = 0; w < NW - 1; w++) set_bits(k, C * w, pat[t], C);
            set_bits(k, C * (NW - 1), top, CFG::TOP_BITS);
            edge.push_back(k);
        }
    }
    // single windows at the sign threshold, one at a time
    for (int w = 0; w < NW - 1; w++) {
        k256 k = small(0);
        set_bits(k, C * w, 1ull << (C - 1), C);
        edge.push_back(k);
        k256 k2 = small(0);
        set_bits(k2, C * w, (1ull << (C - 1)) + 1, C);
        edge.push_back(k2);
    }
    for (size_t i = 0; i < edge.size(); i++) {
        if (!lt_r(edge[i])) {
            std::fprintf(stderr, "edge case %zu not below r\n", i);
            std::exit(1);
        }
        check_one<CFG>(edge[i], "edge");
    }
    int done = 0;
    while (done < 100000) {
        k256 k{{rnd(), rnd(), rnd(), rnd() >> 2}};
        if (!lt_r(k)) continue;
        check_one<CFG>(k, "random");
        done++;
    }
    if (!g_fail) std::printf("c=%d ok (%zu edge, %d random)\n", C, edge.size(),
                             done);
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
