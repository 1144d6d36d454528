// ============================================================================
// BN254 G2 hooks into the shared Pippenger machinery: the msm_curve traits,
// the affine negate of the signed walk, and the input kernels (EIP-197
// bytes; see gpu_g2_bn254.h for the normative byte semantics).  Included by
// api_msm_bn254_g2.hip only, AFTER msm_api_impl.h, so that an edit here or in
// gpu_g2_bn254.h rebuilds no other curve's translation unit.
// ============================================================================
#pragma once
#include "msm_kernels.h"
#include "gpu_g2_bn254.h"

namespace em {

template <>
__device__ __forceinline__ void g1a_neg_y9<Bn254G2>(g1aQ2 &p) {
    p.y = fq2_neg(p.y);
}

// parse one 128-B point: 0 ok, 1 off-curve, 2 non-canonical coordinate
__device__ __forceinline__ int bn254_g2_parse_one(const uint8_t *b, g1aQ2 &p,
                                                  bool &is_inf) {
    fe9 c[4];   // x.c1, x.c0, y.c1, y.c0
    bool allz = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        c[k] = feT_from_be<Fq9T>(b + 32 * k);
        // 9x29 limbs hold all 256 input bits, so the raw compare is exact
        if (fe9_geq_raw<9>(c[k], bn254::FQ9_P)) return 2;
        if (!fe9_is_zero_raw<9>(c[k])) allz = false;
    }
    if (allz) {
        is_inf = true;
        return 0;
    }
    p.x = {to_mont9<Fq9T>(c[1]), to_mont9<Fq9T>(c[0])};
    p.y = {to_mont9<Fq9T>(c[3]), to_mont9<Fq9T>(c[2])};
    is_inf = false;
    if (!bn254_g2_on_curve(p)) return 1;
    return 0;
}

// r*P == O ?
__device__ __forceinline__ bool bn254_g2_in_subgroup(const g1aQ2 &p) {
    g1jQ2 t = g1_scalar_mul9<Bn254G2>(p, bn254::G2_ORDER, 4);
    return g1_is_inf9<Bn254G2>(t);
}

// err bits: 1 off-curve, 2 non-canonical, 4 not in the r-subgroup
static __global__ void k_bn254_g2_parse_points(const uint8_t *__restrict__ in,
                                               g1aQ2 *__restrict__ pts,
                                               uint8_t *__restrict__ inf,
                                               size_t n,
                                               uint32_t *__restrict__ err) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    g1aQ2 p;
    bool is_inf;
    int rc = bn254_g2_parse_one(in + 128 * i, p, is_inf);
    if (rc) {
        atomicOr(err, rc == 2 ? 2u : 1u);
        return;
    }
    if (is_inf) {
        inf[i] = 1;
        pts[i].x = fq2_zero();
        pts[i].y = fq2_zero();
        return;
    }
    inf[i] = 0;
    if (!bn254_g2_in_subgroup(p)) atomicOr(err, 4u);
    pts[i] = p;
}

// P_i = (start+i+1) * G2
static __global__ void k_bn254_g2_gen_points(g1aQ2 *__restrict__ pts,
                                             uint8_t *__restrict__ inf,
                                             size_t n, uint64_t start) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 k = start + i + 1;
    g1aQ2 g = bn254_g2_generator();
    g1jQ2 acc = g1_inf9<Bn254G2>();
    for (int b = 63; b >= 0; b--) {
        acc = g1_dbl9<Bn254G2>(acc);
        if ((k >> b) & 1) acc = g1_add_affine9<Bn254G2>(acc, g);
    }
    if (g1_is_inf9<Bn254G2>(acc)) {   // start + i + 1 wrapped to 0
        inf[i] = 1;
        pts[i].x = fq2_zero();
        pts[i].y = fq2_zero();
        return;
    }
    pts[i] = g1_to_affine9<Bn254G2>(acc);
    inf[i] = 0;
}

static __global__ void k_bn254_g2_points_to_be(const g1aQ2 *__restrict__ pts,
                                               const uint8_t *__restrict__ inf,
                                               uint8_t *__restrict__ out,
                                               size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (inf[i]) {
        for (int j = 0; j < 16; j++) ((u64 *)(out + 128 * i))[j] = 0;
        return;
    }
    fq2_to_be(out + 128 * i, pts[i].x);
    fq2_to_be(out + 128 * i + 64, pts[i].y);
}

// single ops.  add: on-curve only; mul: subgroup-checked, scalar mod r
static __global__ void k_bn254_g2_add_single(const uint8_t *in /* 256 B */,
                                             uint8_t *out, uint32_t *err) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    g1jQ2 acc = g1_inf9<Bn254G2>();
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        g1aQ2 p;
        bool is_inf;
        int rc = bn254_g2_parse_one(in + 128 * k, p, is_inf);
        if (rc) {
            atomicOr(err, rc == 2 ? 2u : 1u);
            return;
        }
        if (!is_inf) acc = g1_add_affine9<Bn254G2>(acc, p);
    }
    g1_to_affine_be9<Bn254G2>(out, acc);
}

static __global__ void k_bn254_g2_mul_single(const uint8_t *in /* 128+32 B */,
                                             uint8_t *out, uint32_t *err) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    g1aQ2 p;
    bool is_inf;
    int rc = bn254_g2_parse_one(in, p, is_inf);
    if (rc) {
        atomicOr(err, rc == 2 ? 2u : 1u);
        return;
    }
    if (is_inf) {
        for (int j = 0; j < 16; j++) ((u64 *)out)[j] = 0;
        return;
    }
    if (!bn254_g2_in_subgroup(p)) {
        atomicOr(err, 4u);
        return;
    }
    fe4 k = from_mont<Fr>(to_mont<Fr>(fe_from_be(in + 128)));
    g1_to_affine_be9<Bn254G2>(out, g1_scalar_mul9<Bn254G2>(p, k.v, 4));
}

// NTT/quotient handoff: packed fe4m Montgomery -> canonical (< r) packed
// u64x4, the value layout k_parse_scalars produces (same kernel as the G1
// handoff in api_msm_bn254.hip)
static __global__ void k_bn254_g2_scalars_from_fe4m(
    const fe4 *__restrict__ src, fe4 *__restrict__ dst, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe9 c = from_mont9<Fr9T>(fe9_from_u64x4(src[i].v));
    fe4 out;
    fe9_to_u64x4(out.v, c);
    dst[i] = out;
}

template <>
struct msm_curve<Bn254G2> {
    static constexpr bool BN_SCALARS = true;    // mod-r scalars, 254 bits
    static constexpr bool LAZY_WALK = false;    // no lazy Fq2 mixed add yet
    static constexpr bool SIGNED_ONLY = true;   // c=8 or signed c=17 only
    static constexpr bool OWN_IO = true;
    static constexpr bool FB_MERGED = false;    // G1 only (msm_fb_recode.h)
    static constexpr const char *SUBGROUP_ERR = "G2 point not in subgroup";
    static void launch_parse_points(const uint8_t *in, g1aQ2 *pts,
                                    uint8_t *inf, size_t n, uint32_t *err) {
        hipLaunchKernelGGL(k_bn254_g2_parse_points,
                           dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0,
                           in, pts, inf, n, err);
    }
    static void launch_gen_points(g1aQ2 *pts, uint8_t *inf, size_t n,
                                  uint64_t start) {
        hipLaunchKernelGGL(k_bn254_g2_gen_points,
                           dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0,
                           pts, inf, n, start);
    }
    static void launch_points_to_be(const g1aQ2 *pts, const uint8_t *inf,
                                    uint8_t *out, size_t n) {
        hipLaunchKernelGGL(k_bn254_g2_points_to_be,
                           dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0,
                           pts, inf, out, n);
    }
};

}  // namespace em
