// ============================================================================
// Lazy signed mixed add for the L=9 (BN254) field: the bucket walk's
// acc += (neg ? -q : q) with the modular bookkeeping the result does not
// need removed.  Same madd-2008-s formulas as g1_add_affine9, but
//   * the digit sign is folded into R (no negate of q.y first),
//   * P, R and Q-X3 are limb-normalised only (no conditional subtractions:
//     they feed multiplies, which accept values <= 8p at L=9),
//   * X3 is one combined limb expression with one normalise,
//   * Y3 = R*(Q-X3) + (3p-Y1)*PPP is one 162-mad column sum and ONE
//     Montgomery reduction,
//   * infinity rides in a caller-held flag instead of a ZZ test per add.
//
// Loop invariant (holds on entry and exit of g1_madd_lazy9 when !acc_inf;
// "c/64" bounds are in units of p/64 and are what the host audit asserts):
//   acc.x   : limbs < 2^29, value < 333/64 p  (5.21p)   -- NOT norm2p
//   acc.y   : limbs < 2^29, value < 2p                  (norm2p)
//   acc.zz  : limbs < 2^29, value < 1.5p                (mul output)
//   acc.zzz : limbs < 2^29, value < 1.5p                (mul output)
// q is norm2p.  g1_lazy_finish9 tightens acc.x to norm2p once per bucket.
//
// R' = 2^261 and 2^261/p = 169.28, so a product of values a*p and b*p
// reduces to < (a*b/169.28 + 1) p; every bound below uses that.
// ============================================================================
#pragma once
#include "gpu_g1_9.h"

namespace em {

// ---- borrow-safe multiples of p ----
// K*p with J*2^29 added to every limb below the top and J taken from the
// limb above (the sum telescopes to zero): a per-limb expression that
// subtracts up to J normalised values from it never borrows, provided the
// top limb also covers the subtrahends' top limbs (checked at each use).
struct lazy_kp9 {
    u32 l[9];
};

template <typename T>
constexpr lazy_kp9 lazy_kp_plain(u32 k) {   // k*p, normalised limbs
    lazy_kp9 r{};
    u64 c = 0;
    for (int i = 0; i < 9; i++) {
        u64 t = (u64)T::P[i] * k + c;
        r.l[i] = (u32)(t & bn254::FQ9_MASK);
        c = t >> 29;
    }
    r.l[8] += (u32)(c << 29);   // c == 0 for every k used here (asserted)
    return r;
}

template <typename T>
constexpr lazy_kp9 lazy_kp_make(u32 k, u32 j) {
    lazy_kp9 r = lazy_kp_plain<T>(k);
    for (int i = 0; i < 9; i++) {
        if (i < 8) r.l[i] += j << 29;
        if (i > 0) r.l[i] -= j;
    }
    return r;
}

// value(c) == k*p, lower limbs >= j*(2^29-1) and < 2^32 - 2^29 (room for
// one normalised addend), top limb did not wrap
template <typename T>
constexpr bool lazy_kp_ok(const lazy_kp9 &c, u32 k, u32 j) {
    lazy_kp9 pl = lazy_kp_plain<T>(k);
    if (pl.l[8] > bn254::FQ9_MASK || pl.l[8] < j) return false;
    u64 carry = 0;
    for (int i = 0; i < 9; i++) {            // re-normalise and compare
        u64 t = (u64)c.l[i] + carry;
        if ((u32)(t & bn254::FQ9_MASK) != pl.l[i] && i < 8) return false;
        if (i == 8 && t != pl.l[8]) return false;
        carry = t >> 29;
    }
    for (int i = 0; i < 8; i++) {
        if (c.l[i] < j * bn254::FQ9_MASK) return false;
        if (c.l[i] >= 0xe0000000u) return false;
    }
    return true;
}

// upper bound on the top limb of a normalised value < c64/64 * p
template <typename T>
constexpr u32 lazy_top(u32 c64) {
    return (u32)(((u64)c64 * (T::P[8] + 1)) / 64 + 1);
}

// value bounds in p/64 units (derivations at the use sites)
constexpr u32 LZ_X = 333;     // acc.x invariant            5.21p
constexpr u32 LZ_Y = 128;     // acc.y invariant (norm2p)   2p
constexpr u32 LZ_Z = 96;      // acc.zz/zzz, mul outputs    1.5p
constexpr u32 LZ_U = 66;      // u2, s2                     1.04p
constexpr u32 LZ_P = 451;     // P, Q-X3                    7.05p
constexpr u32 LZ_R = 323;     // R                          5.05p
constexpr u32 LZ_PP = 83;     // PP                         1.30p
constexpr u32 LZ_PPP = 68;    // PPP                        1.07p
constexpr u32 LZ_Q = 67;      // Q                          1.05p
constexpr u32 LZ_N = 193;     // 3p - Y1                    3.02p
constexpr u32 LZ_MUL = 512;   // multiply contract          8p

template <typename T>
struct lazy_consts9 {
    // 6p, one subtrahend:  u2 + K6 - X1  and  Q + K6 - X3
    static constexpr lazy_kp9 K6 = lazy_kp_make<T>(6, 1);
    // 4p, two subtrahends: K4 - Y1 -/+ s2
    static constexpr lazy_kp9 K4R = lazy_kp_make<T>(4, 2);
    // 4p, three subtrahends: RR + K4 - PPP - Q - Q
    static constexpr lazy_kp9 K4X = lazy_kp_make<T>(4, 3);
    // 3p, one subtrahend: K3 - Y1
    static constexpr lazy_kp9 K3 = lazy_kp_make<T>(3, 1);
    // p^-1 mod 2^29 (N0INV is -p^-1)
    static constexpr u32 PINV = (0u - T::N0INV) & bn254::FQ9_MASK;

    static_assert(T::L == 9, "lazy headroom exists only at L=9");
    static_assert(lazy_kp_ok<T>(K6, 6, 1), "K6 != 6p / limb borrow");
    static_assert(lazy_kp_ok<T>(K4R, 4, 2), "K4R != 4p / limb borrow");
    static_assert(lazy_kp_ok<T>(K4X, 4, 3), "K4X != 4p / limb borrow");
    static_assert(lazy_kp_ok<T>(K3, 3, 1), "K3 != 3p / limb borrow");
    // top-limb borrow safety against the subtrahends' value bounds
    static_assert(K6.l[8] >= lazy_top<T>(LZ_X), "K6 top vs X");
    static_assert(K4R.l[8] >= lazy_top<T>(LZ_Y) + lazy_top<T>(LZ_U),
                  "K4R top vs Y1 + s2");
    static_assert(K4X.l[8] >= lazy_top<T>(LZ_PPP) + 2 * lazy_top<T>(LZ_Q),
                  "K4X top vs PPP + 2Q");
    static_assert(K3.l[8] >= lazy_top<T>(LZ_Y), "K3 top vs Y1");
    static_assert(((T::P[0] * PINV) & bn254::FQ9_MASK) == 1, "PINV");
};

// ---- host-only audit hooks (tools/madd_lazy_check.cpp defines
// EM_LAZY9_AUDIT and supplies em_lazy9_audit_fail) ----
#if defined(EM_LAZY9_AUDIT) && !defined(__HIP_DEVICE_COMPILE__)
void em_lazy9_audit_fail(const char *what);
// limbs < 2^29 and value < c64/64 * p   <=>   64*a < c64*p
template <typename T>
inline void lazy_audit(const fe9 &a, u32 c64, const char *what) {
    u64 l[10], r[10], cl = 0, cr = 0;
    for (int i = 0; i < 9; i++) {
        if (a.v[i] > bn254::FQ9_MASK) em_lazy9_audit_fail(what);
        u64 x = (u64)a.v[i] * 64 + cl, y = (u64)T::P[i] * c64 + cr;
        l[i] = x & bn254::FQ9_MASK, cl = x >> 29;
        r[i] = y & bn254::FQ9_MASK, cr = y >> 29;
    }
    l[9] = cl, r[9] = cr;
    for (int i = 9; i >= 0; i--) {
        if (l[i] != r[i]) {
            if (l[i] > r[i]) em_lazy9_audit_fail(what);
            return;
        }
    }
    em_lazy9_audit_fail(what);   // equal: bound is strict
}
#define EM_LAZY_AUDIT(F, a, c64, what) lazy_audit<F>(a, c64, what)
#else
#define EM_LAZY_AUDIT(F, a, c64, what) ((void)0)
#endif

// a == k*p for some 0 <= k <= kmax?  (a: limbs < 2^29.)  Exact: k is pinned
// by the low limb (k = a0 * p^-1 mod 2^29), so the hot path is one
// mul_lo + compare and the full limb compare runs only in the cold branch
// (taken falsely with probability (kmax+1)/2^29).
template <typename T>
__device__ __host__ __forceinline__ bool fe9_is_kp(const fe9 &a, u32 kmax) {
    u32 k = (a.v[0] * lazy_consts9<T>::PINV) & bn254::FQ9_MASK;
    if (__builtin_expect(k > kmax, 1)) return false;
    u32 c = 0, d = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        u32 t = T::P[i] * k + c;          // k <= 7: < 2^32
        d |= (t & bn254::FQ9_MASK) ^ a.v[i];
        c = t >> 29;
    }
    return d == 0;
}

// Montgomery reduction of 17 product columns: the tail of mont_mul9 at
// L=9, kept here as its own copy so that gpu_field9.h -- and with it every
// kernel of every field that does not use the lazy add -- compiles from
// unchanged source.  t[k] < 2^63 on entry; t is consumed.  Output limbs
// < 2^29, value < (sum of products)/R' + p.
template <typename T>
__device__ __host__ __forceinline__ fe9 lazy_redc9(u64 (&t)[17]) {
    static_assert(T::L == 9, "L=9 only");
#pragma unroll
    for (int k = 0; k < 9; k++) {
        u32 m = ((u32)t[k] * T::N0INV) & bn254::FQ9_MASK;
#pragma unroll
        for (int j = 0; j < 9; j++) t[k + j] += (u64)m * T::P[j];
        t[k + 1] += t[k] >> 29;        // t[k] ≡ 0 mod 2^29 now
    }
    fe9 r;
    u64 c = 0;
#pragma unroll
    for (int k = 9; k < 17; k++) {
        c += t[k];
        r.v[k - 9] = (u32)c & bn254::FQ9_MASK;
        c >>= 29;
    }
    r.v[8] = (u32)c;
    return r;
}

// A*B + C*D in one column accumulation and ONE reduction.
// Inputs: limbs < 2^29 (27 * 2^58 + carries < 2^63 per column),
// value(A)*value(B) + value(C)*value(D) <= 64 p^2.
template <typename T>
__device__ __host__ __forceinline__ fe9 mont_mul2_9(const fe9 &A, const fe9 &B,
                                                    const fe9 &C, const fe9 &D) {
    u64 t[17];
#pragma unroll
    for (int k = 0; k < 17; k++) t[k] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
#pragma unroll
        for (int j = 0; j < 9; j++) {
            t[i + j] += (u64)A.v[i] * B.v[j];
            t[i + j] += (u64)C.v[i] * D.v[j];
        }
    }
    return lazy_redc9<T>(t);
}

// acc += (neg ? -q : q); acc_inf is the caller-held infinity flag (acc's
// coordinates are meaningless while it is set).  q: affine, norm2p, not
// infinity.  See the header comment for the invariant on acc.
template <typename C>
__device__ __host__ __forceinline__ void g1_madd_lazy9(g1jT<C> &acc, bool &acc_inf,
                                                       const g1aT<C> &q, bool neg) {
    using F = typename C::F;
    static_assert(F::L == 9, "g1_madd_lazy9 is L=9 only");
    using K = lazy_consts9<F>;
    if (__builtin_expect(acc_inf, 0)) {
        // first add of a run, or first after a P + (-P) cancellation
        acc.x = q.x;
        acc.y = neg ? neg9<F>(q.y) : q.y;
        acc.zz = fe9_load<9>(F::ONE);
        acc.zzz = fe9_load<9>(F::ONE);
        acc_inf = false;
        return;
    }
    EM_LAZY_AUDIT(F, acc.x, LZ_X, "in X1");
    EM_LAZY_AUDIT(F, acc.y, LZ_Y, "in Y1");
    EM_LAZY_AUDIT(F, acc.zz, LZ_Z, "in ZZ");
    EM_LAZY_AUDIT(F, acc.zzz, LZ_Z, "in ZZZ");
    EM_LAZY_AUDIT(F, q.x, 128, "in x2");
    EM_LAZY_AUDIT(F, q.y, 128, "in y2");
    // u2, s2 < (2 * 1.5 / 169.28 + 1) p = 1.018p
    fe9 u2 = mont_mul9<F>(q.x, acc.zz);
    fe9 s2 = mont_mul9<F>(q.y, acc.zzz);
    EM_LAZY_AUDIT(F, u2, LZ_U, "u2");
    EM_LAZY_AUDIT(F, s2, LZ_U, "s2");
    // P = u2 + 6p - X1: X1 < 5.21p => 0.79p < P < 7.03p, normalised only.
    // Feeds PP, PPP (multiplies: <= 8p ok) and the zero test.
    // R = +-s2 + 4p - Y1: the sign is a two's-complement conditional negate
    // of each s2 limb (limb expression stays in [0, 2^31): K4R limbs >=
    // 2*(2^29-1)).  neg: R > 4p - 1.02p - 2p > 0;  pos: 2p < R < 5.02p.
    fe9 P, R;
    u32 sg = neg ? 0xffffffffu : 0u;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        P.v[i] = u2.v[i] + K::K6.l[i] - acc.x.v[i];
        R.v[i] = (K::K4R.l[i] - acc.y.v[i]) + ((s2.v[i] ^ sg) - sg);
    }
    P = fe9_norm<9>(P);
    R = fe9_norm<9>(R);
    EM_LAZY_AUDIT(F, P, LZ_P, "P");
    EM_LAZY_AUDIT(F, R, LZ_R, "R");
    // exceptional cases, exact: 0 < P < 8p so P ≡ 0 iff P in {p..7p};
    // 0 < R < 6p so R ≡ 0 iff R in {p..5p}
    if (fe9_is_kp<F>(P, 7)) {
        if (fe9_is_kp<F>(R, 5)) {
            // +-q == acc: g1_dbl9 takes X1 only into multiplies (< 8p ok),
            // Y1 norm2p; its output is norm2p
            acc = g1_dbl9(acc);
        } else {
            acc = g1_inf9<C>();
            acc_inf = true;
        }
        return;
    }
    fe9 PP = mont_sqr9<F>(P);             // < 7.05^2/169.28 + 1 = 1.294p
    fe9 PPP = mont_mul9<F>(P, PP);        // < 7.05*1.30/169.28 + 1 = 1.054p
    fe9 Q = mont_mul9<F>(acc.x, PP);      // < 5.21*1.30/169.28 + 1 = 1.040p
    fe9 RR = mont_sqr9<F>(R);             // < 5.05^2/169.28 + 1 = 1.151p
    EM_LAZY_AUDIT(F, PP, LZ_PP, "PP");
    EM_LAZY_AUDIT(F, PPP, LZ_PPP, "PPP");
    EM_LAZY_AUDIT(F, Q, LZ_Q, "Q");
    // X3 = RR + 4p - PPP - 2Q: PPP + 2Q < 3.14p so X3 > 0.86p, and
    // X3 < 1.151p + 4p = 5.151p < 333/64 p: the invariant, no csub.
    // D = Q + 6p - X3: 0.79p < D < 7.04p, normalised only (feeds the Y3 sum)
    // N = 3p - Y1:     p < N <= 3p
    fe9 X3, D, N;
#pragma unroll
    for (int i = 0; i < 9; i++)
        X3.v[i] = RR.v[i] + K::K4X.l[i] - PPP.v[i] - Q.v[i] - Q.v[i];
    X3 = fe9_norm<9>(X3);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        D.v[i] = Q.v[i] + K::K6.l[i] - X3.v[i];
        N.v[i] = K::K3.l[i] - acc.y.v[i];
    }
    D = fe9_norm<9>(D);
    N = fe9_norm<9>(N);
    EM_LAZY_AUDIT(F, D, LZ_P, "D");
    EM_LAZY_AUDIT(F, N, LZ_N, "N");
    // Y3 = R*D + N*PPP ≡ R(Q - X3) - Y1*PPP, one reduction:
    // < ((5.05*7.05 + 3.02*1.07)/169.28 + 1) p = 1.23p  (norm2p)
    acc.y = mont_mul2_9<F>(R, D, N, PPP);
    acc.x = X3;
    acc.zz = mont_mul9<F>(acc.zz, PP);    // < 1.5*1.30/169.28 + 1 = 1.012p
    acc.zzz = mont_mul9<F>(acc.zzz, PPP);
    EM_LAZY_AUDIT(F, acc.x, LZ_X, "out X3");
    EM_LAZY_AUDIT(F, acc.y, LZ_Y, "out Y3");
    EM_LAZY_AUDIT(F, acc.zz, LZ_Z, "out ZZ");
    EM_LAZY_AUDIT(F, acc.zzz, LZ_Z, "out ZZZ");
}

// end of a run: hand the accumulator back under the norm2p contract the
// reduce kernels expect (acc.x < 5.21p -> two conditional 2p subtractions;
// the other coordinates already are norm2p).  Once per bucket.  While the
// infinity flag is set acc holds g1_inf9() (the caller starts it there and
// the cancellation branch puts it back), which passes through unchanged --
// so no flag here, and no select between two whole points.
template <typename C>
__device__ __host__ __forceinline__ g1jT<C> g1_lazy_finish9(const g1jT<C> &acc) {
    using F = typename C::F;
    g1jT<C> o = acc;
    o.x = fe9_csub2p<F>(fe9_csub2p<F>(acc.x));
    return o;
}

}  // namespace em
