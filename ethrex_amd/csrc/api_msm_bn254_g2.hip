// ============================================================================
// ethrex_mi355 C-ABI implementation — MI355X-native BN254 MSM/NTT core.
//
// See include/ethrex_mi355.h for the boundary contract and DESIGN.md for the
// kernel design.  Threading: plans are not internally locked.
//
// NO CPU FALLBACK: every compute entry point requires a visible GPU and
// returns EM_ERR_HIP otherwise.
// ============================================================================
// api_msm_bn254_g2.hip — BN254 G2 MSM ABI (the Groth16 B-query over Fq2;
// EIP-197 128-byte points, scalars reduced mod r).
#include "msm_api_impl.h"
#include "msm_kernels_g2_bn254.h"

struct em_bn254_g2_msm_plan : msm_plan_t<Bn254G2> {};
using g2plan = msm_plan_t<Bn254G2>;

extern "C" int ethrex_mi355_bn254_g2_msm_plan_create(
    size_t n, em_bn254_g2_msm_plan **plan) {
    return msm_create_t(n, (g2plan **)plan);
}
extern "C" int ethrex_mi355_bn254_g2_msm_plan_destroy(em_bn254_g2_msm_plan *p) {
    return msm_destroy_t((g2plan *)p);
}
extern "C" int ethrex_mi355_bn254_g2_msm_upload_points(em_bn254_g2_msm_plan *p,
                                                       const uint8_t *pts128) {
    return msm_upload_points_t((g2plan *)p, pts128);
}
extern "C" int ethrex_mi355_bn254_g2_msm_gen_points(em_bn254_g2_msm_plan *p,
                                                    uint64_t start) {
    return msm_gen_points_t((g2plan *)p, start);
}
extern "C" int ethrex_mi355_bn254_g2_msm_download_points(
    em_bn254_g2_msm_plan *p, uint8_t *out128) {
    return msm_download_points_t((g2plan *)p, out128);
}
extern "C" int ethrex_mi355_bn254_g2_msm_upload_scalars(
    em_bn254_g2_msm_plan *p, const uint8_t *s32) {
    return msm_upload_scalars_t((g2plan *)p, s32);
}
extern "C" int ethrex_mi355_bn254_g2_msm_run(em_bn254_g2_msm_plan *p,
                                             uint8_t out[128]) {
    return msm_run_inner_t((g2plan *)p, out, 0);
}
extern "C" int ethrex_mi355_bn254_g2_msm_run_partial(em_bn254_g2_msm_plan *p,
                                                     uint8_t out[192]) {
    return msm_run_inner_t((g2plan *)p, out, 1);
}
extern "C" int ethrex_mi355_bn254_g2_msm_run_async(em_bn254_g2_msm_plan *p,
                                                   uint8_t out[128]) {
    return msm_run_async_t((g2plan *)p, out);
}
extern "C" int ethrex_mi355_bn254_g2_msm_sync(em_bn254_g2_msm_plan *p) {
    return msm_sync_t((g2plan *)p);
}
extern "C" int ethrex_mi355_bn254_g2_msm_last_times(em_bn254_g2_msm_plan *p,
                                                    double times_ms[5]) {
    if (!p || !times_ms) return EM_ERR_INPUT;
    memcpy(times_ms, p->last_ms, sizeof p->last_ms);
    return EM_OK;
}

// the witness vector of an NTT / quotient plan feeds B2 without PCIe
extern "C" int ethrex_mi355_bn254_g2_msm_scalars_from_ntt(
    em_bn254_g2_msm_plan *plan, const void *ntt_data, uint64_t offset) {
    auto *p = (g2plan *)plan;
    if (!p || !ntt_data) return EM_ERR_INPUT;
    int rc0 = msm_sync_t(p);
    if (rc0) return rc0;
    hipLaunchKernelGGL(k_bn254_g2_scalars_from_fe4m,
                       dim3(blocks_for(p->n, 256)), dim3(256), 0, 0,
                       (const fe4 *)ntt_data + offset, p->d_scalars, p->n);
    HIP_TRY(hipDeviceSynchronize());
    p->have_scalars = true;
    return EM_OK;
}

extern "C" int ethrex_mi355_bn254_g2_msm(const uint8_t *points128,
                                         const uint8_t *scalars32, size_t n,
                                         uint8_t out[128]) {
    if (!points128 || !scalars32 || !out || n == 0) return EM_ERR_INPUT;
    em_bn254_g2_msm_plan *p = nullptr;
    int rc = ethrex_mi355_bn254_g2_msm_plan_create(n, &p);
    if (rc) return rc;
    rc = ethrex_mi355_bn254_g2_msm_upload_points(p, points128);
    if (!rc) rc = ethrex_mi355_bn254_g2_msm_upload_scalars(p, scalars32);
    if (!rc) rc = ethrex_mi355_bn254_g2_msm_run(p, out);
    ethrex_mi355_bn254_g2_msm_plan_destroy(p);
    return rc;
}

// run_single maps kernel err bits 1/4 to EM_ERR_POINT and 2 to EM_ERR_INPUT
extern "C" int ethrex_mi355_bn254_g2_add(const uint8_t p1[128],
                                         const uint8_t p2[128],
                                         uint8_t out[128]) {
    if (!p1 || !p2 || !out) return EM_ERR_INPUT;
    return run_single(k_bn254_g2_add_single, p1, 128, p2, 128, out, 128);
}
extern "C" int ethrex_mi355_bn254_g2_mul(const uint8_t point[128],
                                         const uint8_t scalar[32],
                                         uint8_t out[128]) {
    if (!point || !scalar || !out) return EM_ERR_INPUT;
    return run_single(k_bn254_g2_mul_single, point, 128, scalar, 32, out, 128);
}
