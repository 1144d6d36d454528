// Host check of the BN254 Fq2 layer and G2 group operations
// (csrc/gpu_g2_bn254.h).  The fused multiply fq2_mul_f and the square
// fq2_sqr are compared, as canonical values, with the Karatsuba form
// fq2_mul_k and with a schoolbook built from mont_mul9.  Built with
// EM_LAZY9_AUDIT, so every multiply input also passes the limb/value bound
// audit written next to it in the header.
//
//   hipcc -x hip --offload-host-only -O2 -std=c++17 -DEM_LAZY9_AUDIT \
//         -I ../csrc fq2_check.cpp -o fq2_check
//
// Exit status 0 = all cases agree; prints one "<group> ok" line per group.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef EM_LAZY9_AUDIT
#define EM_LAZY9_AUDIT 1
#endif
#include "gpu_g2_bn254.h"

namespace em {
void em_lazy9_audit_fail(const char *what) {
    std::fprintf(stderr, "AUDIT FAIL: bound violated at '%s'\n", what);
    std::exit(2);
}
}  // namespace em

using namespace em;
using C = Bn254G2;
using F = Fq9T;

static u64 rng_s = 0x243f6a8885a308d3ull;
static u64 rnd() {
    rng_s ^= rng_s << 13;
    rng_s ^= rng_s >> 7;
    rng_s ^= rng_s << 17;
    return rng_s;
}

static int g_fail = 0;
static void fail(const char *grp, long i, const char *msg) {
    std::fprintf(stderr, "FAIL [%s] case %ld: %s\n", grp, i, msg);
    if (++g_fail > 20) std::exit(1);
}

// random canonical value < 2^253 < p, raw limbs
static fe9 rnd_raw() {
    u64 w[4] = {rnd(), rnd(), rnd(), rnd() >> 11};
    return fe9_from_u64<F>(w);
}
static fe9 raw_const(u32 x) {
    fe9 r = fe9_zero();
    r.v[0] = x;
    return r;
}
static fe9 raw_p() { return fe9_load<9>(F::P); }
static fe9 raw_p_minus_1() {
    fe9 r = raw_p();
    r.v[0] -= 1;   // p is odd: no borrow
    return r;
}
// stored representative x + p (norm limbs, < 2p for x < p)
static fe9 plus_p(const fe9 &x) {
    return fe9_norm<9>(add9<9>(x, raw_p()));
}
// a norm2p stored value: canonical or its + p form
static fe9 rnd_norm2p() {
    fe9 x = rnd_raw();
    return (rnd() & 1) ? plus_p(x) : x;
}
static fq2 rnd_fq2() { return {rnd_norm2p(), rnd_norm2p()}; }

static bool same(const fq2 &a, const fq2 &b) { return fq2_eq_modp(a, b); }

// schoolbook on four single multiplies
static fq2 mul_school(const fq2 &a, const fq2 &b) {
    fq2 r;
    r.c0 = subm9<F>(mont_mul9<F>(a.c0, b.c0), mont_mul9<F>(a.c1, b.c1));
    r.c1 = add9_n<F>(mont_mul9<F>(a.c0, b.c1), mont_mul9<F>(a.c1, b.c0));
    return r;
}

static void audit_norm2p(const fq2 &a, const char *what) {
    lazy_audit<F>(a.c0, 128, what);
    lazy_audit<F>(a.c1, 128, what);
}

static void check_mul(const char *grp, long i, const fq2 &a, const fq2 &b) {
    fq2 f = fq2_mul_f(a, b), k = fq2_mul_k(a, b), s = mul_school(a, b);
    audit_norm2p(f, "fused out norm2p");
    audit_norm2p(k, "karatsuba out norm2p");
    if (!same(f, k)) fail(grp, i, "fused != karatsuba");
    if (!same(f, s)) fail(grp, i, "fused != schoolbook");
    if (!same(fq2_mul(a, b), s)) fail(grp, i, "fq2_mul != schoolbook");
    fq2 q = fq2_sqr(a);
    audit_norm2p(q, "sqr out norm2p");
    if (!same(q, mul_school(a, a))) fail(grp, i, "sqr != schoolbook");
    if (!same(q, fq2_mul_k(a, a))) fail(grp, i, "sqr != karatsuba");
}

// ---- group helpers ----
static g1jQ2 from_affine(const g1aQ2 &a) {
    g1jQ2 p;
    p.x = a.x;
    p.y = a.y;
    p.zz = fq2_one();
    p.zzz = fq2_one();
    return p;
}
static g1jQ2 smul(const g1aQ2 &p, const u64 *k, int nwords) {
    g1jQ2 acc = g1_inf9<C>();
    for (int i = 64 * nwords - 1; i >= 0; i--) {
        acc = g1_dbl9<C>(acc);
        if ((k[i >> 6] >> (i & 63)) & 1) acc = g1_add_affine9<C>(acc, p);
    }
    return acc;
}
static g1jQ2 smul1(const g1aQ2 &p, u64 k) { return smul(p, &k, 1); }

// canonical 128-byte image (zeros for infinity)
struct img_t {
    uint8_t b[128];
};
static img_t img(const g1jQ2 &p) {
    img_t r;
    g1_to_affine_be9<C>(r.b, p);
    return r;
}
static bool same_pt(const g1jQ2 &a, const g1jQ2 &b) {
    img_t x = img(a), y = img(b);
    return std::memcmp(x.b, y.b, 128) == 0;
}

int main() {
    // ---- field: random inputs ----
    {
        const char *grp = "random";
        for (long i = 0; i < 20000; i++) check_mul(grp, i, rnd_fq2(), rnd_fq2());
        // inverse and negate
        for (long i = 0; i < 200; i++) {
            fq2 a = rnd_fq2();
            if (fq2_is_zero_modp(a)) continue;
            if (!same(fq2_mul(a, fq2_inv(a)), fq2_one())) fail(grp, i, "a * 1/a != 1");
            if (!fq2_is_zero_modp(fq2_add_n(a, fq2_neg(a)))) fail(grp, i, "a + (-a) != 0");
            fq2 b = rnd_fq2();
            if (!same(fq2_add_n(fq2_subn(a, b), b), a)) fail(grp, i, "(a-b)+b != a");
        }
        std::printf("%s ok\n", grp);
    }

    // ---- field: extreme inputs in every slot ----
    {
        const char *grp = "extreme";
        std::vector<fe9> ext;
        ext.push_back(raw_const(0));
        ext.push_back(raw_const(1));
        ext.push_back(raw_p_minus_1());
        ext.push_back(raw_p());                        // p itself (≡ 0)
        ext.push_back(plus_p(raw_const(1)));           // p + 1
        ext.push_back(plus_p(raw_p_minus_1()));        // 2p - 1
        {
            fe9 t = plus_p(raw_p_minus_1());           // 2p - 2
            t.v[0] -= 1;                               // 2p - 1 is odd: no borrow
            ext.push_back(t);
        }
        ext.push_back(plus_p(rnd_raw()));
        ext.push_back(rnd_raw());
        long n = 0;
        for (const fe9 &a0 : ext)
            for (const fe9 &a1 : ext)
                for (const fe9 &b0 : ext)
                    for (const fe9 &b1 : ext) {
                        check_mul(grp, n, fq2{a0, a1}, fq2{b0, b1});
                        n++;
                    }
        // the negation helper at its edges: 2p - 0 = 2p, 2p - (2p-1) = 1
        fe9 z = fq_neg2p_norm(raw_const(0));
        if (!fe9_eq_raw<9>(z, fe9_load<9>(F::TWOP))) fail(grp, n, "2p - 0");
        fe9 o = fq_neg2p_norm(plus_p(raw_p_minus_1()));
        if (!fe9_eq_raw<9>(o, raw_const(1))) fail(grp, n, "2p - (2p-1)");
        std::printf("%s ok (%ld combinations)\n", grp, n);
    }

    // ---- field: chained (outputs fed back) ----
    {
        const char *grp = "chain";
        fq2 xf = rnd_fq2(), y = rnd_fq2();
        fq2 xk = xf;
        for (long i = 0; i < 4000; i++) {
            // alternate multiply / square, feeding outputs back into both slots
            fq2 nf, nk;
            if (i % 3 == 2) {
                nf = fq2_sqr(xf);
                nk = fq2_mul_k(xk, xk);
            } else {
                nf = fq2_mul_f(xf, y);
                nk = fq2_mul_k(xk, y);
            }
            audit_norm2p(nf, "chain out");
            if (!same(nf, nk)) fail(grp, i, "fused chain != karatsuba chain");
            y = (i & 1) ? xf : fq2_add_n(xf, y);
            xf = nf;
            xk = nk;
        }
        std::printf("%s ok\n", grp);
    }

    // ---- group operations on the host ----
    {
        const char *grp = "group";
        g1aQ2 g = bn254_g2_generator();
        if (!bn254_g2_on_curve(g)) fail(grp, 0, "generator off curve");
        // r * G = O, (r-1) * G = -G
        g1jQ2 rg = smul(g, bn254::G2_ORDER, 4);
        if (!g1_is_inf9<C>(rg)) fail(grp, 1, "r*G != O");
        u64 rm1[4];
        for (int i = 0; i < 4; i++) rm1[i] = bn254::G2_ORDER[i];
        rm1[0] -= 1;
        g1jQ2 mg = from_affine(g);
        g1_neg_y9<C>(mg);
        if (!same_pt(smul(g, rm1, 4), mg)) fail(grp, 2, "(r-1)*G != -G");
        // pool of multiples
        const int NP = 64;
        std::vector<g1aQ2> pool(NP);
        std::vector<u64> ks(NP);
        for (int i = 0; i < NP; i++) {
            ks[i] = (rnd() >> 8) | 1;
            pool[i] = g1_to_affine9<C>(smul1(g, ks[i]));
            if (!bn254_g2_on_curve(pool[i])) fail(grp, i, "multiple off curve");
        }
        for (long i = 0; i < 400; i++) {
            int a = rnd() % NP, b = rnd() % NP, c = rnd() % NP;
            g1jQ2 acc = g1_add_affine9<C>(from_affine(pool[a]), pool[b]);
            // mixed add == full add
            g1jQ2 m = g1_add_affine9<C>(acc, pool[c]);
            g1jQ2 f = g1_add9<C>(acc, from_affine(pool[c]));
            if (!same_pt(m, f)) fail(grp, i, "add_affine != add");
            // against the scalar relation (k_a + k_b + k_c) * G
            u64 k3[2];
            unsigned __int128 s = (unsigned __int128)ks[a] + ks[b] + ks[c];
            k3[0] = (u64)s;
            k3[1] = (u64)(s >> 64);
            if (!same_pt(m, smul(g, k3, 2))) fail(grp, i, "sum != (ka+kb+kc)G");
            // doubling branch: acc + acc (affine and full), == dbl
            if (g1_is_inf9<C>(acc)) continue;
            g1aQ2 self = g1_to_affine9<C>(acc);
            g1jQ2 d = g1_dbl9<C>(acc);
            if (!same_pt(g1_add_affine9<C>(acc, self), d)) fail(grp, i, "P+P (affine) != 2P");
            if (!same_pt(g1_add9<C>(acc, from_affine(self)), d)) fail(grp, i, "P+P != 2P");
            // cancel branch
            g1aQ2 neg = self;
            neg.y = fq2_neg(neg.y);
            if (!g1_is_inf9<C>(g1_add_affine9<C>(acc, neg))) fail(grp, i, "P+(-P) (affine) != O");
            if (!g1_is_inf9<C>(g1_add9<C>(acc, from_affine(neg)))) fail(grp, i, "P+(-P) != O");
            // identity operands
            if (!same_pt(g1_add9<C>(acc, g1_inf9<C>()), acc)) fail(grp, i, "P+O != P");
            if (!same_pt(g1_add_affine9<C>(g1_inf9<C>(), self), acc)) fail(grp, i, "O+P != P");
        }
        // Jacobian wire round trip
        for (int i = 0; i < 16; i++) {
            g1jQ2 acc = g1_add_affine9<C>(from_affine(pool[i]), pool[i + 16]);
            uint8_t w[192];
            g1_jac_be9<C>(w, acc);
            g1jQ2 back;
            if (!g1_jac_from_be9<C>(back, w) || !same_pt(back, acc)) fail(grp, i, "jacobian wire");
        }
        std::printf("%s ok\n", grp);
    }

    if (g_fail) {
        std::fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    std::printf("fq2_check: all cases agree\n");
    return 0;
}
