// ============================================================================
// BN254 G2 on gfx950: Fq2 = Fq[u]/(u^2 + 1) over the 9x29-limb base field,
// twist y^2 = x^3 + 3/(9+u).  This is the Groth16 B-query group.
//
// Byte semantics (EIP-197; normative, repeated in include/ethrex_mi355.h
// and DESIGN.md):
//   affine point, 128 B: x.c1 || x.c0 || y.c1 || y.c0, each 32-B big-endian
//     -- IMAGINARY part first, the opposite of the BLS c0||c1 order.
//     All-zero bytes are the identity on input and output.  Coordinates
//     must be canonical (< p), else EM_ERR_INPUT (stricter than the G1
//     from_be_bytes_mod_order convention, deliberately); off-curve points
//     give EM_ERR_POINT.
//   subgroup: the cofactor is 2p - r.  mul, msm and upload_points enforce
//     r*P = O (else EM_ERR_POINT) because scalars are reduced mod r; add
//     checks on-curve only.
//   Jacobian partial, 192 B: X || Y || Z, each element c1||c0 canonical;
//     Z = 0 is the identity.
//
// The Pippenger machinery is curve-templated on g1aT<C>/g1jT<C> and the
// group-op overload set; BN254 G2 plugs in by SPECIALISING those for the
// Bn254G2 tag, as gpu_g2.h does for BLS.  The group formulas below are a
// second copy of the gpu_g2.h bodies (same EFD add-2008-s / madd-2008-s /
// dbl-2008-s) over fq2: gpu_g2.h is hard-wired to fe14 and stays untouched,
// so the bodies could not be shared through a template without editing it.
//
// Bound discipline (gpu_field9.h contracts): every fq2 component is norm2p
// (limbs < 2^29, value < 2p) between operations.
//
// The multiply.  L=9 has what L=14 lacks: a column of TWO 9-term products
// still fits a u64 (27 * 2^58 < 2^63).  So
//   c1 = a0*b1 + a1*b0          one mont_mul2_9
//   c0 = a0*b0 + a1*(2p - b1)   one mont_mul2_9, 2p - b1 limb-normalised
// is 4 products and 2 Montgomery reductions with no subtraction chain after
// them; Karatsuba (fq2_mul_k, the gpu_g2.h algorithm) is 3 products, 3
// reductions and 3 subm9.  Both are 486 mads; the fused form has one serial
// reduce chain fewer and no carry-normalise/conditional-subtract tail.
// Bounds of the fused form, for norm2p inputs:
//   limbs of a0, a1, b0, b1 and of nb1 = 2p - b1 are < 2^29
//     => column <= 18 * (2^29-1)^2 products + 9 * (2^29-1)^2 reduction
//        + carries < 2^63                                  (static_assert)
//   value(nb1) <= 2p  =>  sum of products <= 8 p^2 <= 64 p^2  (contract)
//   output < 8p^2/R' + p = (8/169.28 + 1) p < 1.05p  =>  norm2p.
// -DEM_FQ2_KARATSUBA makes fq2_mul the Karatsuba form everywhere (A/B).
// ============================================================================
#pragma once
#include "gpu_g1_9_lazy.h"   // mont_mul2_9, EM_LAZY_AUDIT
#include "bn254_g2_constants_dev.h"

namespace em {

struct fq2 {
    fe9 c0, c1;   // c0 + c1*u
};

using FQ = Fq9T;

// ---- bounds the fused multiply rests on, asserted on the constants ----
namespace fq2_bounds {
constexpr u64 LMAX = bn254::FQ9_MASK;          // normalised limb
// two 9-term product rows + the 9-term reduction row + carry-in
static_assert(27 * (LMAX * LMAX) + (1ull << 36) < (1ull << 63),
              "fused fq2 column sum must stay below 2^63");
// lazy one-level add feeding mont_mul9 (fq2_sqr): limbs < 2^30 times
// limbs < 2^29, 9 terms, + reduction row
static_assert(9 * ((2 * LMAX) * LMAX) + 9 * (LMAX * LMAX) + (1ull << 36) <
                  (1ull << 63),
              "lazy-add operand column sum must stay below 2^63");
// C2P is 2p with 2^29 lent to every limb below the top: C2P - b never
// borrows in a lower limb for normalised b, and re-normalises to 2p
constexpr bool c2p_ok() {
    u64 c = 0;
    for (int i = 0; i < 9; i++) {
        if (i < 8 && FQ::C2P[i] < LMAX) return false;
        u64 t = (u64)FQ::C2P[i] + c;
        if ((t & LMAX) != FQ::TWOP[i]) return false;
        c = t >> 29;
    }
    return c == 0;
}
static_assert(c2p_ok(), "C2P must be a borrow-safe form of 2p");
static_assert(FQ::TWOP[8] <= LMAX, "2p must fit 9 normalised limbs");
// 4p + 2p (fq2_sqr: a0 + 4p - a1 < 6p) fits the limbs as well
static_assert(3 * (u64)FQ::TWOP[8] + 3 <= LMAX, "6p must fit 9 limbs");
// value bounds, in p^2: fused products 2p*2p + 2p*2p = 8 <= 64;
// sqr c0 (4p)(6p) = 24 <= 64; sqr c1 (2p)(4p) = 8 <= 64.  Output bound
// (S/169.28 + 1) p with R'/p > 169: 24/169 + 1 < 2 => norm2p.
static_assert((FQ::P[8] + 1ull) * 169 < (1ull << 29),
              "R'/p > 169: mul outputs of <= 64p^2 stay below 1.38p");
}  // namespace fq2_bounds

__device__ __host__ __forceinline__ fq2 fq2_zero() {
    return {fe9_zero(), fe9_zero()};
}
__device__ __host__ __forceinline__ fq2 fq2_one() {
    return {fe9_load<9>(FQ::ONE), fe9_zero()};
}
__device__ __host__ __forceinline__ fq2 fq2_add_n(const fq2 &a, const fq2 &b) {
    return {add9_n<FQ>(a.c0, b.c0), add9_n<FQ>(a.c1, b.c1)};
}
// a - b, b a MUL-OUTPUT pair (< 1.5p per component)
__device__ __host__ __forceinline__ fq2 fq2_subm(const fq2 &a, const fq2 &b) {
    return {subm9<FQ>(a.c0, b.c0), subm9<FQ>(a.c1, b.c1)};
}
// a - b, b norm2p
__device__ __host__ __forceinline__ fq2 fq2_subn(const fq2 &a, const fq2 &b) {
    return {subn9<FQ>(a.c0, b.c0), subn9<FQ>(a.c1, b.c1)};
}
__device__ __host__ __forceinline__ fq2 fq2_neg(const fq2 &a) {
    return {neg9<FQ>(a.c0), neg9<FQ>(a.c1)};
}
__device__ __host__ __forceinline__ bool fq2_is_zero_modp(const fq2 &a) {
    return fe9_is_zero_modp<FQ>(a.c0) && fe9_is_zero_modp<FQ>(a.c1);
}
__device__ __host__ __forceinline__ bool fq2_eq_modp(const fq2 &a,
                                                     const fq2 &b) {
    return fe9_eq_raw<9>(fe9_csubp<FQ>(a.c0), fe9_csubp<FQ>(b.c0)) &&
           fe9_eq_raw<9>(fe9_csubp<FQ>(a.c1), fe9_csubp<FQ>(b.c1));
}

// 2p - b, limbs normalised (< 2^29), value in (0, 2p]; b norm2p.  The top
// limb may pass through a wrapped intermediate when b's top limb equals
// 2p's; the true value is non-negative, so the mod-2^32 limb arithmetic of
// fe9_norm lands on it.
__device__ __host__ __forceinline__ fe9 fq_neg2p_norm(const fe9 &b) {
    fe9 t;
#pragma unroll
    for (int i = 0; i < 9; i++) t.v[i] = FQ::C2P[i] - b.v[i];
    return fe9_norm<9>(t);
}

// Karatsuba, 3 base multiplies (the gpu_g2.h algorithm over fe9): the A/B
// baseline and the differential partner of the host check
__device__ __host__ __forceinline__ fq2 fq2_mul_k(const fq2 &a, const fq2 &b) {
    EM_LAZY_AUDIT(FQ, a.c0, 128, "mul_k a0");
    EM_LAZY_AUDIT(FQ, a.c1, 128, "mul_k a1");
    EM_LAZY_AUDIT(FQ, b.c0, 128, "mul_k b0");
    EM_LAZY_AUDIT(FQ, b.c1, 128, "mul_k b1");
    fe9 sa = add9_n<FQ>(a.c0, a.c1), sb = add9_n<FQ>(b.c0, b.c1);
    EM_LAZY_AUDIT(FQ, sa, 128, "mul_k a0+a1");
    EM_LAZY_AUDIT(FQ, sb, 128, "mul_k b0+b1");
    fe9 m0 = mont_mul9<FQ>(a.c0, b.c0);
    fe9 m1 = mont_mul9<FQ>(a.c1, b.c1);
    fe9 m2 = mont_mul9<FQ>(sa, sb);
    fq2 r;
    r.c0 = subm9<FQ>(m0, m1);
    r.c1 = subm9<FQ>(subm9<FQ>(m2, m0), m1);
    return r;
}

// fused: 4 products, 2 reductions, no subtraction after the multiplies
__device__ __host__ __forceinline__ fq2 fq2_mul_f(const fq2 &a, const fq2 &b) {
    fe9 nb1 = fq_neg2p_norm(b.c1);
    EM_LAZY_AUDIT(FQ, a.c0, 128, "mul a0");
    EM_LAZY_AUDIT(FQ, a.c1, 128, "mul a1");
    EM_LAZY_AUDIT(FQ, b.c0, 128, "mul b0");
    EM_LAZY_AUDIT(FQ, b.c1, 128, "mul b1");
    EM_LAZY_AUDIT(FQ, nb1, 129, "mul 2p-b1");   // <= 2p, strictly < 129/64 p
    fq2 r;
    r.c0 = mont_mul2_9<FQ>(a.c0, b.c0, a.c1, nb1);
    r.c1 = mont_mul2_9<FQ>(a.c0, b.c1, a.c1, b.c0);
    EM_LAZY_AUDIT(FQ, r.c0, 68, "mul out c0");  // < 1.05p
    EM_LAZY_AUDIT(FQ, r.c1, 68, "mul out c1");
    return r;
}

__device__ __host__ __forceinline__ fq2 fq2_mul(const fq2 &a, const fq2 &b) {
#ifdef EM_FQ2_KARATSUBA
    return fq2_mul_k(a, b);
#else
    return fq2_mul_f(a, b);
#endif
}

// c0 = (a0+a1)(a0-a1), c1 = a0 * 2a1: two single multiplies.  Chosen over
// c1 = mont_mul2_9(a0,a1,a0,a1) by instruction count: that form spends 162
// product mads on the same value 81 give here (the doubling is 9 shifts).
// a0+a1 and 2a1 are one-level lazy adds (limbs < 2^30, allowed as an L=9
// multiply input); a0-a1 is a0 + 4p - a1, limb-normalised only (< 6p).
__device__ __host__ __forceinline__ fq2 fq2_sqr(const fq2 &a) {
    EM_LAZY_AUDIT(FQ, a.c0, 128, "sqr a0");
    EM_LAZY_AUDIT(FQ, a.c1, 128, "sqr a1");
    fe9 s = add9<9>(a.c0, a.c1);       // < 4p, limbs < 2^30
    fe9 d;
#pragma unroll
    for (int i = 0; i < 9; i++) d.v[i] = a.c0.v[i] + FQ::C4P[i] - a.c1.v[i];
    d = fe9_norm<9>(d);                // 2p < d < 6p
    EM_LAZY_AUDIT(FQ, d, 384, "sqr a0-a1");
    fq2 r;
    r.c0 = mont_mul9<FQ>(s, d);                          // < 1.15p
    r.c1 = mont_mul9<FQ>(a.c0, add9<9>(a.c1, a.c1));     // < 1.05p
    EM_LAZY_AUDIT(FQ, r.c0, 74, "sqr out c0");
    EM_LAZY_AUDIT(FQ, r.c1, 68, "sqr out c1");
    return r;
}

// 1/(a0 + a1 u) = (a0 - a1 u) / (a0^2 + a1^2)
__device__ __host__ __forceinline__ fq2 fq2_inv(const fq2 &a) {
    fe9 n = add9_n<FQ>(mont_sqr9<FQ>(a.c0), mont_sqr9<FQ>(a.c1));
    fe9 t = mont_inv9<FQ>(n);
    fq2 r;
    r.c0 = mont_mul9<FQ>(a.c0, t);
    r.c1 = neg9<FQ>(mont_mul9<FQ>(a.c1, t));
    return r;
}

// canonical byte IO, EIP-197 order: c1 || c0, 32-B BE each
__device__ __host__ __forceinline__ void fq2_to_be(uint8_t *b, const fq2 &m) {
    feT_to_be<FQ>(b, from_mont9<FQ>(m.c1));
    feT_to_be<FQ>(b + 32, from_mont9<FQ>(m.c0));
}
__device__ __host__ __forceinline__ fq2 fq2_from_be_mont(const uint8_t *b) {
    fq2 r;
    r.c1 = to_mont9<FQ>(feT_from_be<FQ>(b));
    r.c0 = to_mont9<FQ>(feT_from_be<FQ>(b + 32));
    return r;
}

// curve tag; F = the base field trait (scalar machinery uses F::W64)
struct Bn254G2 {
    using F = Fq9T;
};

template <>
struct g1aT<Bn254G2> {
    fq2 x, y;
};
template <>
struct g1jT<Bn254G2> {
    fq2 x, y, zz, zzz;  // XYZZ over Fq2
};

using g1aQ2 = g1aT<Bn254G2>;
using g1jQ2 = g1jT<Bn254G2>;

template <>
__device__ __host__ __forceinline__ g1jQ2 g1_inf9<Bn254G2>() {
    g1jQ2 p;
    p.x = fq2_one();
    p.y = fq2_one();
    p.zz = fq2_zero();
    p.zzz = fq2_zero();
    return p;
}

template <>
__device__ __host__ __forceinline__ bool g1_is_inf9<Bn254G2>(const g1jQ2 &p) {
    return fq2_is_zero_modp(p.zz);
}

// dbl-2008-s over fq2 (a = 0)
template <>
__device__ __host__ __forceinline__ g1jQ2 g1_dbl9<Bn254G2>(const g1jQ2 &p) {
    if (g1_is_inf9<Bn254G2>(p)) return p;
    fq2 U = fq2_add_n(p.y, p.y);
    fq2 V = fq2_sqr(U);
    fq2 W = fq2_mul(U, V);
    fq2 S = fq2_mul(p.x, V);
    fq2 A = fq2_sqr(p.x);
    fq2 M = fq2_add_n(fq2_add_n(A, A), A);
    g1jQ2 o;
    o.x = fq2_subm(fq2_subm(fq2_sqr(M), S), S);
    o.y = fq2_subm(fq2_mul(M, fq2_subn(S, o.x)), fq2_mul(W, p.y));
    o.zz = fq2_mul(V, p.zz);
    o.zzz = fq2_mul(W, p.zzz);
    return o;
}

// add-2008-s over fq2
template <>
__device__ __host__ __forceinline__ g1jQ2 g1_add9<Bn254G2>(const g1jQ2 &p,
                                                           const g1jQ2 &q) {
    if (g1_is_inf9<Bn254G2>(p)) return q;
    if (g1_is_inf9<Bn254G2>(q)) return p;
    fq2 u1 = fq2_mul(p.x, q.zz);
    fq2 u2 = fq2_mul(q.x, p.zz);
    fq2 s1 = fq2_mul(p.y, q.zzz);
    fq2 s2 = fq2_mul(q.y, p.zzz);
    fq2 P = fq2_subm(u2, u1);
    fq2 R = fq2_subm(s2, s1);
    if (__builtin_expect(fq2_is_zero_modp(P), 0)) {
        if (fq2_is_zero_modp(R)) return g1_dbl9<Bn254G2>(p);
        return g1_inf9<Bn254G2>();
    }
    fq2 PP = fq2_sqr(P);
    fq2 PPP = fq2_mul(P, PP);
    fq2 Q = fq2_mul(u1, PP);
    g1jQ2 o;
    o.x = fq2_subm(fq2_subm(fq2_subm(fq2_sqr(R), PPP), Q), Q);
    o.y = fq2_subm(fq2_mul(R, fq2_subn(Q, o.x)), fq2_mul(s1, PPP));
    o.zz = fq2_mul(fq2_mul(p.zz, q.zz), PP);
    o.zzz = fq2_mul(fq2_mul(p.zzz, q.zzz), PPP);
    return o;
}

// madd-2008-s over fq2
template <>
__device__ __host__ __forceinline__ g1jQ2 g1_add_affine9<Bn254G2>(
    const g1jQ2 &p, const g1aQ2 &q) {
    if (__builtin_expect(g1_is_inf9<Bn254G2>(p), 0)) {
        g1jQ2 o;
        o.x = q.x;
        o.y = q.y;
        o.zz = fq2_one();
        o.zzz = fq2_one();
        return o;
    }
    fq2 u2 = fq2_mul(q.x, p.zz);
    fq2 s2 = fq2_mul(q.y, p.zzz);
    fq2 P = fq2_subn(u2, p.x);
    fq2 R = fq2_subn(s2, p.y);
    if (__builtin_expect(fq2_is_zero_modp(P), 0)) {
        if (fq2_is_zero_modp(R)) return g1_dbl9<Bn254G2>(p);
        return g1_inf9<Bn254G2>();
    }
    fq2 PP = fq2_sqr(P);
    fq2 PPP = fq2_mul(P, PP);
    fq2 Q = fq2_mul(p.x, PP);
    g1jQ2 o;
    o.x = fq2_subm(fq2_subm(fq2_subm(fq2_sqr(R), PPP), Q), Q);
    o.y = fq2_subm(fq2_mul(R, fq2_subn(Q, o.x)), fq2_mul(p.y, PPP));
    o.zz = fq2_mul(p.zz, PP);
    o.zzz = fq2_mul(p.zzz, PPP);
    return o;
}

// y^2 == x^3 + b'   (host + device body; the g1a9_on_curve specialisation
// below is the device entry the shared kernels call)
__device__ __host__ __forceinline__ bool bn254_g2_on_curve(const g1aQ2 &p) {
    fq2 l = fq2_sqr(p.y);
    fq2 r = fq2_mul(fq2_sqr(p.x), p.x);
    fq2 b2{fe9_load<9>(bn254::FQ9_G2_B0), fe9_load<9>(bn254::FQ9_G2_B1)};
    r = fq2_add_n(r, b2);
    return fq2_eq_modp(l, r);
}
template <>
__device__ __forceinline__ bool g1a9_on_curve<Bn254G2>(const g1aQ2 &p) {
    return bn254_g2_on_curve(p);
}

// the EIP-197 generator
__device__ __host__ __forceinline__ g1aQ2 bn254_g2_generator() {
    g1aQ2 g;
    g.x = {fe9_load<9>(bn254::FQ9_G2_GX0), fe9_load<9>(bn254::FQ9_G2_GX1)};
    g.y = {fe9_load<9>(bn254::FQ9_G2_GY0), fe9_load<9>(bn254::FQ9_G2_GY1)};
    return g;
}
template <>
__device__ __forceinline__ g1aQ2 g1_generator9<Bn254G2>() {
    return bn254_g2_generator();
}

// XYZZ -> affine (one fq2 inversion)
template <>
__device__ __host__ __forceinline__ g1aQ2 g1_to_affine9<Bn254G2>(
    const g1jQ2 &p) {
    fq2 t = fq2_inv(fq2_mul(p.zz, p.zzz));
    g1aQ2 a;
    a.x = fq2_mul(p.x, fq2_mul(t, p.zzz));
    a.y = fq2_mul(p.y, fq2_mul(t, p.zz));
    return a;
}

// XYZZ -> affine BE bytes (128 B); infinity -> zeros
template <>
__device__ __host__ __forceinline__ void g1_to_affine_be9<Bn254G2>(
    uint8_t *out, const g1jQ2 &p) {
    if (g1_is_inf9<Bn254G2>(p)) {
        for (int i = 0; i < 16; i++) ((u64 *)out)[i] = 0;
        return;
    }
    g1aQ2 a = g1_to_affine9<Bn254G2>(p);
    fq2_to_be(out, a.x);
    fq2_to_be(out + 64, a.y);
}

template <>
__device__ __host__ __forceinline__ void g1_neg_y9<Bn254G2>(g1jQ2 &p) {
    p.y = fq2_neg(p.y);
}

template <>
struct pt_bytes<Bn254G2> {
    static constexpr int NB = 32;
    static constexpr int AFF = 128;  // x.c1||x.c0||y.c1||y.c0
    static constexpr int JAC = 192;  // X||Y||Z, each c1||c0
};

// Jacobian wire IO over Fq2 (192 B)
template <>
__device__ __host__ __forceinline__ void g1_jac_be9<Bn254G2>(uint8_t *out,
                                                             const g1jQ2 &p) {
    if (g1_is_inf9<Bn254G2>(p)) {
        for (int j = 0; j < 24; j++) ((u64 *)out)[j] = 0;
        return;
    }
    fq2 zzz2 = fq2_sqr(p.zzz);
    fq2 X = fq2_mul(fq2_mul(p.x, p.zz), zzz2);
    fq2 Y = fq2_mul(fq2_mul(p.y, fq2_mul(fq2_sqr(p.zz), p.zz)), zzz2);
    fq2 Z = fq2_mul(p.zz, p.zzz);
    fq2_to_be(out, X);
    fq2_to_be(out + 64, Y);
    fq2_to_be(out + 128, Z);
}

template <>
__device__ __host__ __forceinline__ bool g1_jac_from_be9<Bn254G2>(
    g1jQ2 &o, const uint8_t *in) {
    fq2 X = fq2_from_be_mont(in);
    fq2 Y = fq2_from_be_mont(in + 64);
    fq2 Z = fq2_from_be_mont(in + 128);
    if (fq2_is_zero_modp(Z)) return false;
    o.x = X;
    o.y = Y;
    o.zz = fq2_sqr(Z);
    o.zzz = fq2_mul(o.zz, Z);
    return true;
}

}  // namespace em
