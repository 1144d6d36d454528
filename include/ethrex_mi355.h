/* ============================================================================
 * ethrex_mi355 — C-ABI boundary of the MI355X-native BN254 MSM/NTT prover
 * core.
 *
 * This is the drop-in seam a Rust host binds behind ethrex's `ProverBackend`
 * trait (reference: crates/prover/src/backend/mod.rs:87-153; the backend's
 * `prove` drives these entry points).  The FFI convention mirrors the
 * in-repo ZisK accelerator ABI (crates/guest-program/src/crypto/zisk.rs:71-137):
 *   - `int` status returns (0 = OK, nonzero = error),
 *   - fixed-size byte structs, 8-byte aligned,
 *   - caller-allocated out-parameters.
 * The Rust-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Byte encodings (reference semantics, crates/common/crypto/provider.rs:247-318):
 *   - G1 affine point: 64 bytes big-endian x||y; (0,0) encodes the identity
 *     on input and output (EIP-197; crates/vm/levm/src/precompiles.rs:792-795).
 *     Coordinates are parsed `from_be_bytes_mod_order` (reduced mod p) and
 *     validated on-curve (off-curve => EM_ERR_POINT).
 *   - Scalar / Fr element: 32 bytes big-endian; scalars are reduced mod r
 *     exactly as ark's `from_be_bytes_mod_order` does.  NTT elements must be
 *     canonical (< r) => EM_ERR_INPUT otherwise.
 *   - G1 Jacobian partial (multi-GPU exchange payload): 96 bytes big-endian
 *     X||Y||Z canonical form; Z = 0 encodes the identity.
 *
 * Every compute entry point REQUIRES the MI355X GPU path: there is no CPU
 * fallback anywhere behind this ABI (EM_ERR_HIP if no device).
 * ==========================================================================*/
#ifndef ETHREX_MI355_H
#define ETHREX_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    EM_OK = 0,
    EM_ERR_POINT = 1,   /* G1 point not on curve (provider.rs InvalidPoint) */
    EM_ERR_INPUT = 2,   /* bad size / non-canonical Fr element / null ptr   */
    EM_ERR_HIP = 3,     /* HIP runtime failure or no gfx950 device          */
};

/* library identification / device selection */
const char *ethrex_mi355_version(void);
int ethrex_mi355_device_count(int *count);
int ethrex_mi355_set_device(int device);
/* last HIP error string (for diagnostics after EM_ERR_HIP) */
const char *ethrex_mi355_last_error(void);

/* ---- single-op entry points (zisk.rs:100-102 zkvm_bn254_g1_add/mul
 *      mirror; run on the GPU; used for on-device semantics parity) ---- */
int ethrex_mi355_bn254_g1_add(const uint8_t p1[64], const uint8_t p2[64],
                              uint8_t out[64]);
int ethrex_mi355_bn254_g1_mul(const uint8_t point[64], const uint8_t scalar[32],
                              uint8_t out[64]);

/* ---- one-shot hot-path entry points (host buffers in, host buffer out;
 *      the drop-in calls a Rust `ProverBackend::prove` makes) ---- */
int ethrex_mi355_bn254_g1_msm(const uint8_t *points64, const uint8_t *scalars32,
                              size_t n, uint8_t out[64]);
int ethrex_mi355_bn254_fr_ntt(uint8_t *elems32, size_t n, int inverse);

/* ---- planned API: device-resident buffers for repeated runs (bench /
 *      pipeline use; inputs stay in HBM between runs) ---- */
typedef struct em_msm_plan em_msm_plan;
typedef struct em_ntt_plan em_ntt_plan;

int ethrex_mi355_msm_plan_create(size_t n, em_msm_plan **plan);
int ethrex_mi355_msm_plan_destroy(em_msm_plan *plan);
/* upload host-side affine points (64 B BE each); validates on device */
int ethrex_mi355_msm_upload_points(em_msm_plan *plan, const uint8_t *points64);
/* generate P_i = (start+i+1)*G directly in HBM (deterministic inputs) */
int ethrex_mi355_msm_gen_points(em_msm_plan *plan, uint64_t start);
/* download the plan's points back as 64 B BE affine (parity checks) */
int ethrex_mi355_msm_download_points(em_msm_plan *plan, uint8_t *out64);
int ethrex_mi355_msm_upload_scalars(em_msm_plan *plan, const uint8_t *scalars32);
/* full MSM -> affine result */
int ethrex_mi355_msm_run(em_msm_plan *plan, uint8_t out[64]);
/* shard partial -> Jacobian 96 B (multi-GPU: AllGather these, then combine) */
int ethrex_mi355_msm_run_partial(em_msm_plan *plan, uint8_t out[96]);
/* pipelined MSM step: enqueues the step and returns; the sort chain of the
 * NEXT run_async overlaps this step's bucket/reduction chain on a second
 * HIP stream (the proving loop runs many MSMs back-to-back).  `out` is
 * filled by the time ethrex_mi355_msm_sync — or the depth-2 backpressure of
 * a later run_async — returns; keep it valid until then. */
int ethrex_mi355_msm_run_async(em_msm_plan *plan, uint8_t out[64]);
/* drain all pipelined steps and deliver their results */
int ethrex_mi355_msm_sync(em_msm_plan *plan);
/* pipelined shard step: run_async delivering the 96-B Jacobian partial
 * (the multi-GPU exchange payload) instead of the affine result */
int ethrex_mi355_msm_run_partial_async(em_msm_plan *plan, uint8_t out[96]);
/* deliver the OLDEST pending pipelined step only (blocks on its compute
 * chain; later enqueued steps keep running).  The N>1 exchange loop calls
 * this to AllGather+combine step k while the GPU computes step k+1. */
int ethrex_mi355_msm_wait_one(em_msm_plan *plan);
/* combine Jacobian partials on the GPU -> affine result */
int ethrex_mi355_bn254_g1_combine(const uint8_t *jacobians96, size_t count,
                                  uint8_t out[64]);
/* combine the N>1 exchange payload (world-size 96-B Jacobian partials) on
 * the HOST — boundary glue; avoids touching GPU streams mid-pipeline */
int ethrex_mi355_bn254_g1_combine_cpu(const uint8_t *jacobians96,
                                      size_t count, uint8_t out[64]);
/* wrap-pipeline handoff (sp1.rs:122-134 flow): take this plan's n scalars
 * from an NTT plan's device-resident output (ethrex_mi355_ntt_device_data)
 * at element `offset` — the composed MSM+NTT step stays on-device */
int ethrex_mi355_msm_scalars_from_ntt(em_msm_plan *plan, const void *ntt_data,
                                      uint64_t offset);
/* per-phase HIP-event timings of the last run, milliseconds:
 * [0]=digits+sort, [1]=bucket accumulation, [2]=bucket reduction,
 * [3]=window combine + affine, [4]=total */
int ethrex_mi355_msm_last_times(em_msm_plan *plan, double times_ms[5]);
/* merged fixed-base mode (large plans, bases fixed across runs): when the
 * table T[w*n + i] = 2^(c*w) * P_i fits, upload_points / gen_points build
 * it and every run uses one bucket space for all windows.  *c = window
 * bits (0: the separate-window path runs), *precompute_ms = time of the
 * last table build (setup, outside any run), *table_bytes = table size.
 * EM_MSM_FB=0 forces the mode off, EM_MSM_FB=20|22|24 forces it on. */
int ethrex_mi355_msm_fb_info(em_msm_plan *plan, int *c, double *precompute_ms,
                             uint64_t *table_bytes);
/* rows [start, start+count) of table window w as 64 B BE affine points */
int ethrex_mi355_msm_download_fb_rows(em_msm_plan *plan, int w, size_t start,
                                      size_t count, uint8_t *out64);
/* combine partials reusing the plan's device buffers (per-step exchange) */
int ethrex_mi355_msm_combine(em_msm_plan *plan, const uint8_t *jacobians96,
                             size_t count, uint8_t out[64]);

/* ---- native MPT structure builder (host; §8f row 4 witness-generation
 * speedup).  Fixed 32-byte sorted distinct keys (the hashed-key state /
 * storage trie shape); per-level >= 32-B node encodings come out in the
 * batched-keccak layout, are hashed on the GPU by the caller, and the
 * hashes patch back before the next (shallower) level encodes.  Levels
 * run from mpt_max_depth down to 0; the root is always hashed. ---- */
typedef struct em_mpt em_mpt;
int ethrex_mi355_mpt_create(const uint8_t *keys32, const uint8_t *vals,
                            const uint64_t *val_offs, size_t n, em_mpt **out);
int ethrex_mi355_mpt_destroy(em_mpt *t);
int ethrex_mi355_mpt_max_depth(em_mpt *t, int *depth);
int ethrex_mi355_mpt_level_encode(em_mpt *t, int depth, uint8_t *buf,
                                  uint64_t *offs, size_t buf_cap,
                                  size_t max_n, size_t *n_hash);
int ethrex_mi355_mpt_level_set_hashes(em_mpt *t, int depth,
                                      const uint8_t *h32, size_t n_hash);
int ethrex_mi355_mpt_root(em_mpt *t, uint8_t out[32]);

/* ---- batched Keccak-256 (witness/statement hashing; original Keccak
 * padding, Ethereum keccak256).  offsets[n+1] delimits message i as
 * [offsets[i], offsets[i+1]); out32 receives 32 bytes per message. ---- */
typedef struct em_keccak_plan em_keccak_plan;
int ethrex_mi355_keccak256_batch(const uint8_t *msgs, const uint64_t *offsets,
                                 size_t n, uint8_t *out32);
int ethrex_mi355_keccak_plan_create(size_t max_bytes, size_t max_n,
                                    em_keccak_plan **plan);
int ethrex_mi355_keccak_plan_destroy(em_keccak_plan *plan);
int ethrex_mi355_keccak_upload(em_keccak_plan *plan, const uint8_t *msgs,
                               const uint64_t *offsets, size_t n);
int ethrex_mi355_keccak_run(em_keccak_plan *plan);
int ethrex_mi355_keccak_download(em_keccak_plan *plan, uint8_t *out32);
int ethrex_mi355_keccak_last_ms(em_keccak_plan *plan, double *ms);
/* device pointer to the n 32-B digests of the last keccak_run; valid until
 * the next upload/destroy.  EM_ERR_INPUT if the plan has not run. */
int ethrex_mi355_keccak_device_digests(em_keccak_plan *plan,
                                       const void **ptr, size_t *n);

int ethrex_mi355_ntt_plan_create(size_t n, em_ntt_plan **plan);
int ethrex_mi355_ntt_plan_destroy(em_ntt_plan *plan);
int ethrex_mi355_ntt_upload(em_ntt_plan *plan, const uint8_t *elems32);
int ethrex_mi355_ntt_run(em_ntt_plan *plan, int inverse);
int ethrex_mi355_ntt_download(em_ntt_plan *plan, uint8_t *elems32);
/* [0]=bit-reverse, [1]=butterfly stages total, [2]=total */
int ethrex_mi355_ntt_last_times(em_ntt_plan *plan, double times_ms[3]);
/* device pointer to the current transform output (packed 4x64 Montgomery)
 * for the on-device MSM handoff (ethrex_mi355_msm_scalars_from_ntt) */
int ethrex_mi355_ntt_device_data(em_ntt_plan *plan, const void **ptr,
                                 size_t *n);
/* fill the plan's n resident elements with wrap vector v1 from m device
 * digests; synchronous; leaves the data in the input buffer (cur = 0).
 * Wrap vector v1 (DESIGN.md "Wrap vector v1"): R = pairwise keccak256 tree
 * root of the m digests (odd tail promoted unchanged); block j =
 * keccak-f1600 of the single padded rate block
 * domain || R || le64(m) || le64(j) || digest[j mod m]; element 4j+t = the
 * big-endian integer of state bytes [32t, 32t+32) reduced mod r.
 * EM_ERR_INPUT for null pointers or m == 0.  d_digests32 is a DEVICE
 * pointer (ethrex_mi355_keccak_device_digests); domain is a host pointer. */
int ethrex_mi355_ntt_fill_from_digests(em_ntt_plan *plan,
                                       const void *d_digests32, size_t m,
                                       const uint8_t domain[32]);
/* HIP-event time of the last fill (tree levels + expansion), milliseconds */
int ethrex_mi355_ntt_last_fill_ms(em_ntt_plan *plan, double *ms);

/* ---- coset transforms and the Groth16 quotient polynomial H (DESIGN.md
 * "Quotient polynomial").  Coset generator g = 5 (the gnark-crypto /
 * arkworks generator of BN254 Fr); w as for the plain transform.
 *   coset forward:  A_j = sum_i a_i g^i w^(ij)
 *   coset inverse:  a_i = g^-i n^-1 sum_j A_j w^(-ij)
 * Same buffer rules as ethrex_mi355_ntt_run; the plain transforms of the
 * plan are unaffected.  EM_NTT_COSET_UNFUSED=1 (read once per process)
 * forces the standalone scaling pass on every path (A/B measurement). ---- */
int ethrex_mi355_ntt_run_coset(em_ntt_plan *plan, int inverse);
int ethrex_mi355_bn254_fr_coset_ntt(uint8_t *elems32, size_t n, int inverse);

/* Quotient of three evaluation vectors a, b, c (values on the n-point
 * domain, natural order): with x~ = coset_fwd(intt(x)),
 *   e_j = (a~_j * b~_j - c~_j) * (g^n - 1)^-1,   h = coset_inv(e)
 * — n coefficients, natural order; for c = a (.) b the exact quotient of
 * A*B - C by X^n - 1.  The plan owns one twiddle set, three resident
 * vectors and one work buffer; n a power of two <= 2^28.
 * EM_ERR_INPUT: null pointer, `which` outside 0..2, bad n, non-canonical
 * element on upload, mul_ab_into_c without a and b loaded, quot_run
 * unless all three slots were loaded since the last run, download /
 * device_data before any run (or after slot a was reloaded). */
typedef struct em_quot_plan em_quot_plan;
int ethrex_mi355_quot_plan_create(size_t n, em_quot_plan **plan);
int ethrex_mi355_quot_plan_destroy(em_quot_plan *plan);
/* which: 0 = a, 1 = b, 2 = c */
int ethrex_mi355_quot_upload(em_quot_plan *plan, int which,
                             const uint8_t *elems32);
/* copy n resident fe4m elements device-to-device, e.g. from
 * ethrex_mi355_ntt_device_data (after a fill or a run) */
int ethrex_mi355_quot_load_device(em_quot_plan *plan, int which,
                                  const void *d_fe4m);
/* c = a (.) b, element-wise; marks slot c loaded */
int ethrex_mi355_quot_mul_ab_into_c(em_quot_plan *plan);
/* h = quotient(a, b, c); consumes the three slots */
int ethrex_mi355_quot_run(em_quot_plan *plan);
int ethrex_mi355_quot_download(em_quot_plan *plan, uint8_t *elems32);
/* device pointer to h (fe4m), valid until the next load/run/destroy;
 * feeds ethrex_mi355_msm_scalars_from_ntt unchanged */
int ethrex_mi355_quot_device_data(em_quot_plan *plan, const void **ptr,
                                  size_t *n);
/* [0]=3 iNTT, [1]=3 coset NTT, [2]=pointwise, [3]=coset iNTT, [4]=total (ms) */
int ethrex_mi355_quot_last_times(em_quot_plan *plan, double times_ms[5]);

/* ---- R1CS evaluation: y = M z for the three sparse constraint matrices
 * A, B, C of a Groth16 circuit and the witness vector z (DESIGN.md "R1CS
 * evaluation").  The matrices are uploaded once in CSR form and repacked
 * on the host; the results are resident fe4m vectors that feed
 * ethrex_mi355_quot_load_device without leaving the device.
 *   y_i = sum_k coeff_k * z[col_k] mod r over the entries of row i; a
 *   column may repeat in a row (its terms add), a zero coefficient is
 *   legal, an empty row gives 0, n_rows = 0 gives the zero vector.
 * EM_ERR_INPUT: null pointer, bad n, n_vars == 0 or >= 2^32, `which`
 * outside 0..2, n_rows > n, row_offs[0] != 0 or a decreasing offset,
 * nnz >= 2^32, a column >= n_vars, a non-canonical coefficient or witness
 * element, eval before both that matrix and a witness are loaded, download
 * / device_data before an eval of that matrix since its last upload (or
 * since the last witness change).  A failed upload leaves that matrix (or
 * the witness) unloaded.  EM_R1CS_T (short/long row threshold) and
 * EM_R1CS_CHUNK (long-row chunk, a multiple of 64) override the packing
 * constants; both are read once per process. ---- */
typedef struct em_r1cs_plan em_r1cs_plan;
/* n: evaluation-domain size (power of two <= 2^28, the QuotPlan rule);
 * n_vars: length m of the witness vector z, 1 <= m < 2^32 */
int ethrex_mi355_r1cs_plan_create(size_t n, size_t n_vars, em_r1cs_plan **plan);
int ethrex_mi355_r1cs_plan_destroy(em_r1cs_plan *plan);
/* which: 0 = A, 1 = B, 2 = C.  CSR: row_offs[n_rows+1] (u64, row_offs[0] = 0,
 * non-decreasing), cols[nnz] (u32, < n_vars), coeffs32[nnz] 32-B big-endian
 * canonical Fr.  n_rows <= n; rows [n_rows, n) of the result are zero. */
int ethrex_mi355_r1cs_upload_matrix(em_r1cs_plan *plan, int which,
        const uint64_t *row_offs, const uint32_t *cols,
        const uint8_t *coeffs32, size_t n_rows);
int ethrex_mi355_r1cs_upload_witness(em_r1cs_plan *plan, const uint8_t *z32);
/* take z from n_vars resident fe4m elements at element `offset` of a device
 * vector (ethrex_mi355_ntt_device_data / quot_device_data) */
int ethrex_mi355_r1cs_witness_from_device(em_r1cs_plan *plan,
        const void *d_fe4m, uint64_t offset);
/* y_which = M_which * z; synchronous */
int ethrex_mi355_r1cs_eval(em_r1cs_plan *plan, int which);
int ethrex_mi355_r1cs_download(em_r1cs_plan *plan, int which, uint8_t *elems32);
/* device pointer to the n fe4m results, valid until the next eval of that
 * matrix, upload_matrix(which) or destroy; feeds ethrex_mi355_quot_load_device */
int ethrex_mi355_r1cs_device_data(em_r1cs_plan *plan, int which,
        const void **ptr, size_t *n);
/* HIP-event time of the last eval of A, B, C (ms; 0 if never run) */
int ethrex_mi355_r1cs_last_times(em_r1cs_plan *plan, double times_ms[3]);

/* ---- deterministic input generation (host-side; the product restatement
 *      of BASELINE.md's xoshiro256++/splitmix64 scheme; parity-tested
 *      against the oracle's independent restatement) ---- */
void ethrex_mi355_gen_fr(uint64_t seed, size_t n, uint8_t *out32);

/* ==== BLS12-381 G1 (the blob-KZG commitment MSM
 *      of crates/common/crypto/kzg.rs:208-230 and the EIP-2537 G1 MSM of
 *      provider.rs:620-634 / bls_blst.rs).  Semantics = the in-tree blst
 *      path: 48-byte big-endian CANONICAL coordinates (non-canonical =>
 *      EM_ERR_INPUT), (0,0) identity, on-curve check, r-subgroup check on
 *      MSM inputs (=> EM_ERR_POINT), scalars = full 256-bit integers (no
 *      reduction).  Affine point = 96 B x||y; Jacobian partial = 144 B
 *      X||Y||Z canonical, Z=0 identity. ==== */

int ethrex_mi355_bls12381_g1_add(const uint8_t p1[96], const uint8_t p2[96],
                                 uint8_t out[96]);
int ethrex_mi355_bls12381_g1_mul(const uint8_t point[96],
                                 const uint8_t scalar[32], uint8_t out[96]);
int ethrex_mi355_bls12381_g1_msm(const uint8_t *points96,
                                 const uint8_t *scalars32, size_t n,
                                 uint8_t out[96]);
int ethrex_mi355_bls12381_g1_combine(const uint8_t *jacobians144, size_t count,
                                     uint8_t out[96]);

typedef struct em_bls_msm_plan em_bls_msm_plan;
int ethrex_mi355_bls_msm_plan_create(size_t n, em_bls_msm_plan **plan);
int ethrex_mi355_bls_msm_plan_destroy(em_bls_msm_plan *plan);
int ethrex_mi355_bls_msm_upload_points(em_bls_msm_plan *plan,
                                       const uint8_t *points96);
int ethrex_mi355_bls_msm_gen_points(em_bls_msm_plan *plan, uint64_t start);
int ethrex_mi355_bls_msm_download_points(em_bls_msm_plan *plan, uint8_t *out96);
int ethrex_mi355_bls_msm_upload_scalars(em_bls_msm_plan *plan,
                                        const uint8_t *scalars32);
/* build the fixed-base table (2^(12w)*P_i, c-kzg KZG_PRECOMPUTE-style):
 * the setup points are fixed across blobs, so subsequent runs collapse the
 * window dimension.  Requires n <= 65536; invalidated by new points. */
int ethrex_mi355_bls_msm_precompute(em_bls_msm_plan *plan);
int ethrex_mi355_bls_msm_run(em_bls_msm_plan *plan, uint8_t out[96]);
int ethrex_mi355_bls_msm_run_partial(em_bls_msm_plan *plan, uint8_t out[144]);
int ethrex_mi355_bls_msm_run_async(em_bls_msm_plan *plan, uint8_t out[96]);
int ethrex_mi355_bls_msm_sync(em_bls_msm_plan *plan);

/* ---- BLS12-381 G2 (EIP-2537 / blst semantics, bls_blst.rs:338-441):
 * 192-byte points x.c0||x.c1||y.c0||y.c1 (canonical 48-B BE coords over
 * Fp2 = Fp[u]/(u^2+1)), (0,0,0,0) = identity; add checks on-curve only,
 * MSM additionally enforces the r-subgroup check per point.  Jacobian
 * exchange payload: 288 B (X||Y||Z, each c0||c1). ---- */
typedef struct em_bls_g2_msm_plan em_bls_g2_msm_plan;
int ethrex_mi355_bls12381_g2_add(const uint8_t p1[192], const uint8_t p2[192],
                                 uint8_t out[192]);
int ethrex_mi355_bls12381_g2_mul(const uint8_t point[192],
                                 const uint8_t scalar[32], uint8_t out[192]);
int ethrex_mi355_bls12381_g2_msm(const uint8_t *points192,
                                 const uint8_t *scalars32, size_t n,
                                 uint8_t out[192]);
int ethrex_mi355_bls_g2_msm_plan_create(size_t n, em_bls_g2_msm_plan **plan);
int ethrex_mi355_bls_g2_msm_plan_destroy(em_bls_g2_msm_plan *plan);
int ethrex_mi355_bls_g2_msm_upload_points(em_bls_g2_msm_plan *plan,
                                          const uint8_t *points192);
int ethrex_mi355_bls_g2_msm_gen_points(em_bls_g2_msm_plan *plan,
                                       uint64_t start);
int ethrex_mi355_bls_g2_msm_download_points(em_bls_g2_msm_plan *plan,
                                            uint8_t *out192);
int ethrex_mi355_bls_g2_msm_upload_scalars(em_bls_g2_msm_plan *plan,
                                           const uint8_t *scalars32);
int ethrex_mi355_bls_g2_msm_run(em_bls_g2_msm_plan *plan, uint8_t out[192]);
int ethrex_mi355_bls_g2_msm_run_async(em_bls_g2_msm_plan *plan,
                                      uint8_t out[192]);
int ethrex_mi355_bls_g2_msm_sync(em_bls_g2_msm_plan *plan);
int ethrex_mi355_bls_g2_msm_run_partial(em_bls_g2_msm_plan *plan,
                                        uint8_t out[288]);
int ethrex_mi355_bls_g2_msm_last_times(em_bls_g2_msm_plan *plan,
                                       double times_ms[5]);
int ethrex_mi355_bls_msm_last_times(em_bls_msm_plan *plan, double times_ms[5]);

/* n elements uniform in [0, r_bls) (canonical blob field elements) */
void ethrex_mi355_bls_gen_fr(uint64_t seed, size_t n, uint8_t *out32);

/* ---- BN254 G2 (the Groth16 B-query; EIP-197 byte semantics) over
 * Fq2 = Fq[u]/(u^2+1), twist y^2 = x^3 + 3/(9+u).
 *   affine point, 128 B: x.c1||x.c0||y.c1||y.c0, each 32-B big-endian --
 *     IMAGINARY part first (the opposite of the BLS c0||c1 order).
 *     All-zero bytes are the identity, on input and output.  Coordinates
 *     must be canonical (< p), else EM_ERR_INPUT (stricter than the G1
 *     mod-order convention, as EIP-197 requires); off-curve: EM_ERR_POINT.
 *   subgroup: G2 has cofactor 2p - r; mul, msm and upload_points enforce
 *     r*P = O (else EM_ERR_POINT, last_error "G2 point not in subgroup");
 *     add checks on-curve only.
 *   scalars: 32-B big-endian, reduced mod r.
 *   Jacobian partial, 192 B: X||Y||Z, each element c1||c0 canonical;
 *     Z = 0 is the identity.
 * Geometry: c=8 for n <= 65536, signed c=17 for every larger n
 * (n < 2^30); EM_MSM_TREE does not apply. ---- */
typedef struct em_bn254_g2_msm_plan em_bn254_g2_msm_plan;
int ethrex_mi355_bn254_g2_add(const uint8_t p1[128], const uint8_t p2[128],
                              uint8_t out[128]);
int ethrex_mi355_bn254_g2_mul(const uint8_t point[128],
                              const uint8_t scalar[32], uint8_t out[128]);
int ethrex_mi355_bn254_g2_msm(const uint8_t *points128,
                              const uint8_t *scalars32, size_t n,
                              uint8_t out[128]);
int ethrex_mi355_bn254_g2_msm_plan_create(size_t n,
                                          em_bn254_g2_msm_plan **plan);
int ethrex_mi355_bn254_g2_msm_plan_destroy(em_bn254_g2_msm_plan *plan);
int ethrex_mi355_bn254_g2_msm_upload_points(em_bn254_g2_msm_plan *plan,
                                            const uint8_t *points128);
int ethrex_mi355_bn254_g2_msm_gen_points(em_bn254_g2_msm_plan *plan,
                                         uint64_t start);
int ethrex_mi355_bn254_g2_msm_download_points(em_bn254_g2_msm_plan *plan,
                                              uint8_t *out128);
int ethrex_mi355_bn254_g2_msm_upload_scalars(em_bn254_g2_msm_plan *plan,
                                             const uint8_t *scalars32);
int ethrex_mi355_bn254_g2_msm_run(em_bn254_g2_msm_plan *plan,
                                  uint8_t out[128]);
int ethrex_mi355_bn254_g2_msm_run_partial(em_bn254_g2_msm_plan *plan,
                                          uint8_t out[192]);
int ethrex_mi355_bn254_g2_msm_run_async(em_bn254_g2_msm_plan *plan,
                                        uint8_t out[128]);
int ethrex_mi355_bn254_g2_msm_sync(em_bn254_g2_msm_plan *plan);
int ethrex_mi355_bn254_g2_msm_last_times(em_bn254_g2_msm_plan *plan,
                                         double times_ms[5]);
/* take the plan's n scalars from an NTT/quotient plan's device-resident
 * vector (fe4m) at element `offset`: the witness vector feeds B2 on device */
int ethrex_mi355_bn254_g2_msm_scalars_from_ntt(em_bn254_g2_msm_plan *plan,
                                               const void *ntt_data,
                                               uint64_t offset);

#ifdef __cplusplus
}
#endif

#endif /* ETHREX_MI355_H */
