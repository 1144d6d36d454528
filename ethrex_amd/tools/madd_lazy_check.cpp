// Host differential check of the lazy signed mixed add (gpu_g1_9_lazy.h)
// against g1_add_affine9, results compared as canonical affine points.
// Built with EM_LAZY9_AUDIT, so every call also asserts that each value fed
// to a multiply meets the multiply contract and that the accumulator meets
// the loop invariant stated in the header.
//
//   hipcc -x hip --offload-host-only -O2 -std=c++17 -DEM_LAZY9_AUDIT \
//         -I ../csrc madd_lazy_check.cpp -o madd_lazy_check
//
// Exit status 0 = all cases agree; prints one line per case group.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef EM_LAZY9_AUDIT
#define EM_LAZY9_AUDIT 1
#endif
#include "gpu_g1_9_lazy.h"

namespace em {
void em_lazy9_audit_fail(const char *what) {
    std::fprintf(stderr, "AUDIT FAIL: bound violated at '%s'\n", what);
    std::exit(2);
}
}  // namespace em

using namespace em;
using C = Bn254G1;
using F = Fq9T;

static u64 rng_s = 0x9e3779b97f4a7c15ull;
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
static fe9 raw_p_minus_1() {
    fe9 r = fe9_load<9>(F::P);
    r.v[0] -= 1;   // p is odd: no borrow
    return r;
}
// stored representative x + p (norm limbs, < 2p for x < p)
static fe9 plus_p(const fe9 &x) {
    return fe9_norm<9>(add9<9>(x, fe9_load<9>(F::P)));
}

static g1a9 gen() {
    g1a9 g;
    g.x = fe9_load<9>(C::GX);
    g.y = fe9_load<9>(C::GY);
    return g;
}
static g1j9 smul(const g1a9 &p, u64 k) {
    g1j9 acc = g1_inf9<C>();
    for (int i = 63; i >= 0; i--) {
        acc = g1_dbl9(acc);
        if ((k >> i) & 1) acc = g1_add_affine9(acc, p);
    }
    return acc;
}

struct canon_t {
    bool inf;
    fe9 x, y;
};
static canon_t canon(const g1j9 &p) {
    canon_t c;
    c.inf = g1_is_inf9(p);
    c.x = c.y = fe9_zero();
    if (c.inf) return c;
    g1a9 a = g1_to_affine9(p);
    c.x = from_mont9<F>(a.x);
    c.y = from_mont9<F>(a.y);
    return c;
}
static bool same(const canon_t &a, const canon_t &b) {
    if (a.inf || b.inf) return a.inf == b.inf;
    return fe9_eq_raw<9>(a.x, b.x) && fe9_eq_raw<9>(a.y, b.y);
}

// finished lazy accumulator must meet norm2p and equal the reference
static void compare(const char *grp, long i, const g1j9 &lz, bool lz_inf,
                    const g1j9 &ref) {
    // contract: acc holds g1_inf9() while the flag is set
    if (lz_inf && !g1_is_inf9(lz)) fail(grp, i, "flag set but acc != inf");
    g1j9 f = g1_lazy_finish9(lz);
    if (!lz_inf) {
        lazy_audit<F>(f.x, 128, "finish X");
        lazy_audit<F>(f.y, 128, "finish Y");
        lazy_audit<F>(f.zz, 128, "finish ZZ");
        lazy_audit<F>(f.zzz, 128, "finish ZZZ");
    }
    if (g1_is_inf9(f) != lz_inf) fail(grp, i, "flag vs ZZ disagree");
    if (!same(canon(f), canon(ref))) fail(grp, i, "lazy != reference");
}

static g1j9 ref_add(const g1j9 &acc, g1a9 q, bool neg) {
    if (neg) q.y = neg9<F>(q.y);
    return g1_add_affine9(acc, q);
}

static g1j9 from_affine(const g1a9 &a) {
    g1j9 p;
    p.x = a.x;
    p.y = a.y;
    p.zz = fe9_load<9>(F::ONE);
    p.zzz = fe9_load<9>(F::ONE);
    return p;
}

int main() {
    using K = lazy_consts9<F>;
    // ---- field helpers ----
    {
        // fe9_is_kp: exact for k*p, k*p +- 1 and for values that share only
        // the low limb with k*p (drives the cold full compare)
        for (u32 k = 0; k <= 9; k++) {
            lazy_kp9 kp = lazy_kp_plain<F>(k);
            fe9 a;
            for (int i = 0; i < 9; i++) a.v[i] = kp.l[i];
            for (u32 kmax = 0; kmax <= 8; kmax++) {
                if (fe9_is_kp<F>(a, kmax) != (k <= kmax)) fail("is_kp", k, "k*p");
                for (int i = 1; i < 9; i++) {
                    fe9 b = a;
                    b.v[i] ^= 1u << (i % 22);
                    if (fe9_is_kp<F>(b, kmax)) fail("is_kp", k, "limb flip");
                }
                fe9 c = a;
                c.v[0] ^= 1;
                // low limb changed: c = k*p +- 1 is no multiple of p
                if (fe9_is_kp<F>(c, kmax)) fail("is_kp", k, "low flip");
            }
        }
        // two-product multiply == sum of two multiplies (mod p)
        for (int i = 0; i < 2000; i++) {
            fe9 a = plus_p(rnd_raw()), b = plus_p(rnd_raw());
            fe9 c = rnd_raw(), d = plus_p(rnd_raw());
            fe9 one = mont_mul2_9<F>(a, b, c, d);
            fe9 two = add9_n<F>(mont_mul9<F>(a, b), mont_mul9<F>(c, d));
            lazy_audit<F>(one, 128, "mul2 out");
            if (!fe9_eq_raw<9>(fe9_csubp<F>(one), fe9_csubp<F>(two)))
                fail("mul2", i, "A*B + C*D mismatch");
        }
        (void)K::K6;
        std::printf("field helpers ok\n");
    }

    // ---- point pool: multiples of G, affine ----
    const int NP = 1024;
    std::vector<g1a9> pool(NP);
    {
        g1a9 g = gen();
        g1j9 t = smul(g, rnd() | 1);
        g1a9 step = g1_to_affine9(smul(g, rnd() | 1));
        for (int i = 0; i < NP; i++) {
            pool[i] = g1_to_affine9(t);
            // every other point in its non-canonical x + p / y + p form
            if (i & 1) {
                pool[i].x = plus_p(fe9_csubp<F>(pool[i].x));
                pool[i].y = plus_p(fe9_csubp<F>(pool[i].y));
            }
            t = g1_add_affine9(t, step);
        }
    }

    // ---- random cases: random accumulators (non-trivial ZZ) and points ----
    {
        const char *grp = "random";
        for (long i = 0; i < 4000; i++) {
            // accumulator = sum of three pool points through the reference
            g1j9 ref = from_affine(pool[rnd() % NP]);
            ref = g1_add_affine9(ref, pool[rnd() % NP]);
            ref = g1_add_affine9(ref, pool[rnd() % NP]);
            if (g1_is_inf9(ref)) continue;
            g1j9 lz = ref;
            bool inf = false;
            const g1a9 &q = pool[rnd() % NP];
            bool neg = rnd() & 1;
            g1_madd_lazy9<C>(lz, inf, q, neg);
            compare(grp, i, lz, inf, ref_add(ref, q, neg));
        }
        std::printf("%s ok\n", grp);
    }

    // ---- long chains on one accumulator (the loop invariant) ----
    {
        const char *grp = "chain";
        for (int chain = 0; chain < 3; chain++) {
            const long LEN = chain == 0 ? 20000 : 12000;
            g1j9 lz = g1_inf9<C>(), ref = g1_inf9<C>();
            bool inf = true;   // empty start
            for (long i = 0; i < LEN; i++) {
                const g1a9 &q = pool[rnd() % NP];
                bool neg = chain == 1 ? false : (rnd() & 1);
                g1_madd_lazy9<C>(lz, inf, q, neg);
                ref = ref_add(ref, q, neg);
                // chain 0 compares every step; the others every 97th
                if (chain == 0 || i % 97 == 0 || i == LEN - 1)
                    compare(grp, i, lz, inf, ref);
            }
        }
        std::printf("%s ok\n", grp);
    }

    // ---- empty start / doubling / cancellation / doubling via sign ----
    {
        const char *grp = "special";
        int kseen[8] = {0};
        for (long i = 0; i < 600; i++) {
            const g1a9 &a = pool[rnd() % NP];
            const g1a9 &b = pool[rnd() % NP];
            bool na = rnd() & 1;
            // empty start: first add loads +-a
            g1j9 lz = g1_inf9<C>(), ref = g1_inf9<C>();
            bool inf = true;
            g1_madd_lazy9<C>(lz, inf, a, na);
            ref = ref_add(ref, a, na);
            compare(grp, i, lz, inf, ref);
            // doubling: q equals the accumulator (same sign)
            g1_madd_lazy9<C>(lz, inf, a, na);
            ref = ref_add(ref, a, na);
            compare(grp, i, lz, inf, ref);
            // build a non-trivial ZZ, then add the accumulator's own affine
            // value: doubling with P = k*p for varying k
            g1_madd_lazy9<C>(lz, inf, b, false);
            ref = ref_add(ref, b, false);
            if (inf) continue;
            g1a9 self = g1_to_affine9(g1_lazy_finish9(lz));
            if (i & 1) self.x = plus_p(fe9_csubp<F>(self.x));
            {
                // record which multiple of p the zero test sees
                fe9 u2 = mont_mul9<F>(self.x, lz.zz), P;
                for (int j = 0; j < 9; j++)
                    P.v[j] = u2.v[j] + K::K6.l[j] - lz.x.v[j];
                P = fe9_norm<9>(P);
                u32 k = (P.v[0] * K::PINV) & bn254::FQ9_MASK;
                if (k >= 1 && k <= 7) kseen[k]++;
                else fail(grp, i, "P of a doubling is not k*p, 1<=k<=7");
            }
            g1j9 lz2 = lz, ref2 = ref;
            bool inf2 = inf;
            if (i % 3 == 0) {
                // doubling via sign: q = -acc, neg = true
                g1a9 m = self;
                m.y = neg9<F>(m.y);
                g1_madd_lazy9<C>(lz2, inf2, m, true);
                ref2 = ref_add(ref2, m, true);
            } else {
                g1_madd_lazy9<C>(lz2, inf2, self, false);
                ref2 = ref_add(ref2, self, false);
            }
            if (inf2) fail(grp, i, "doubling gave infinity");
            compare(grp, i, lz2, inf2, ref2);
            // cancellation: q = -acc (by sign on even i, by value on odd i)
            if (i & 2) {
                g1_madd_lazy9<C>(lz, inf, self, true);
                ref = ref_add(ref, self, true);
            } else {
                g1a9 m = self;
                m.y = neg9<F>(m.y);
                g1_madd_lazy9<C>(lz, inf, m, false);
                ref = ref_add(ref, m, false);
            }
            if (!inf) fail(grp, i, "cancellation did not give infinity");
            compare(grp, i, lz, inf, ref);
            // ... and the next add reloads
            g1_madd_lazy9<C>(lz, inf, b, na);
            ref = ref_add(ref, b, na);
            if (inf) fail(grp, i, "reload left the flag set");
            compare(grp, i, lz, inf, ref);
            g1_madd_lazy9<C>(lz, inf, a, !na);
            ref = ref_add(ref, a, !na);
            compare(grp, i, lz, inf, ref);
        }
        std::printf("%s ok (doubling P = k*p seen for k=1..7: %d %d %d %d %d %d %d)\n",
                    grp, kseen[1], kseen[2], kseen[3], kseen[4], kseen[5],
                    kseen[6], kseen[7]);
    }

    // ---- extreme coordinates: stored values 1, p-1, x+p, 2p-1 ----
    // (the add formulas are polynomial identities, so lazy == reference
    // holds for any coordinate values, on the curve or not)
    {
        const char *grp = "extreme";
        std::vector<fe9> ext;
        ext.push_back(raw_const(1));
        ext.push_back(raw_const(2));
        ext.push_back(raw_p_minus_1());
        ext.push_back(plus_p(raw_const(1)));          // p + 1
        ext.push_back(plus_p(raw_p_minus_1()));       // 2p - 1
        ext.push_back(plus_p(rnd_raw()));             // x + p
        ext.push_back(rnd_raw());
        // mul-output-sized ZZ/ZZZ values up to just under 1.5p
        std::vector<fe9> zs;
        zs.push_back(fe9_load<9>(F::ONE));
        zs.push_back(raw_const(1));
        zs.push_back(raw_p_minus_1());
        {
            fe9 h = raw_p_minus_1();                  // (p-1)/2 + p < 1.5p
            u32 c = 0;
            for (int i = 8; i >= 0; i--) {
                u32 t = h.v[i] | (c << 29);
                h.v[i] = t >> 1;
                c = t & 1;
            }
            zs.push_back(plus_p(h));
        }
        long n = 0;
        for (const fe9 &X : ext)
            for (const fe9 &Y : ext)
                for (const fe9 &x2 : ext)
                    for (const fe9 &y2 : ext)
                        for (const fe9 &Z : zs)
                            for (int neg = 0; neg < 2; neg++) {
                                g1j9 ref;
                                ref.x = X;
                                ref.y = Y;
                                ref.zz = Z;
                                ref.zzz = zs[(n + 1) % zs.size()];
                                g1a9 q{x2, y2};
                                g1j9 lz = ref;
                                bool inf = false;
                                g1_madd_lazy9<C>(lz, inf, q, neg);
                                g1j9 r1 = ref_add(ref, q, neg);
                                compare(grp, n, lz, inf, r1);
                                // a second add from the lazy state
                                if (!inf) {
                                    const g1a9 &q2 = pool[n % NP];
                                    g1_madd_lazy9<C>(lz, inf, q2, !neg);
                                    compare(grp, n, lz, inf,
                                            ref_add(r1, q2, !neg));
                                }
                                n++;
                            }
        std::printf("%s ok (%ld combinations)\n", grp, n);
    }

    if (g_fail) {
        std::fprintf(stderr, "%d failures\n", g_fail);
        return 1;
    }
    std::printf("madd_lazy_check: all cases agree\n");
    return 0;
}
