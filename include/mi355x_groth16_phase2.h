/* mi355x_groth16_phase2.h -- the circuit's keys from a powers-of-tau SRS, on the device (BN254): gnark's mpcsetup phase 2.
 *
 * mi_groth16_setup needs tau, alpha, beta, gamma, delta in the clear: whoever ran it can forge proofs.  This header is the other way a
 * key comes to be: nobody knows tau, alpha, beta (a public SRS holds their powers as points; mi355x_groth16_phase1.h makes one by a
 * ceremony of its own and hands its rows over on the device: mi_phase2_init_from_phase1), the circuit's key is DERIVED from the SRS
 * with gamma = 1 and delta = 1, and contributors then re-randomise delta one after the other.  It replaces
 *     mpcsetup.InitPhase2(r1cs, &srs) / (*Phase2).Contribute() / ExtractKeys
 * All of it is Setup's arithmetic "in the exponent" (csrc/phase2.hip): the Lagrange basis is an inverse NTT over curve points
 * (csrc/point_ntt.cuh), the transposed sparse products are sparse sums of points with scalar multiplications by the coefficients
 * (csrc/sparse_points.cuh).
 *
 * Same library and conventions as mi355x_groth16_setup.h: status codes, Montgomery mi_fr, affine points with (0, 0) = infinity,
 * mi_last_error names the field, the R1CS and the SRS are HOST pointers and the library keeps none of them after return, nothing stays
 * allocated after a refusal.
 *
 * Definitions.  N, w, the wire classes and the order of every array are exactly mi355x_groth16_setup.h's.
 *     [L_i]1 = (1 / N) sum_k w^(-i k) [tau^k]1           likewise [alpha L_i]1, [beta L_i]1 and [L_i]2 from their SRS rows
 *     [A_j]1 = sum_i A[i][j] [L_i]1                      likewise [B_j]1 and [B_j]2 (rows >= n_constraints do not exist)
 *     [t_j]1 = sum_i (A[i][j] [beta L_i]1 + B[i][j] [alpha L_i]1 + C[i][j] [L_i]1)
 *     infinity_a[j] / infinity_b[j]                      [A_j]1 / [B_j]1 is the point at infinity
 *     pk.G1.A / G1.B / G2.B / G1.K                       those points for the wires Setup keeps, in wire order; K = [t_j]1 (delta = 1)
 *     pk.G1.Z                                            Z_i = [tau^(i + N)]1 - [tau^i]1, i < N, stored bit-reversed
 *     vk                                                 alpha1 = alpha_tau_g1[0], beta1 = beta_tau_g1[0], beta2 = beta_g2,
 *                                                        gamma2 = delta2 = g2, delta1 = g1, K = [t_j]1 (gamma = 1)
 *     commitment k                                       Basis[i] = [t_j]1 for j = committed[k][i]; BasisExpSigma[i] = sigma_k Basis[i];
 *                                                        the verifying half is mi_pedersen_vk_make(sigma)
 * So an SRS built from known (tau, alpha, beta) gives, byte for byte, the key mi_groth16_setup gives for (tau, alpha, beta, 1, 1, sigma),
 * and after contributions d_1 .. d_m the key for delta = d_1 ... d_m (an affine point has one encoding).
 *
 * NOT DONE HERE (each of them is needed before a ceremony can be trusted).  The first two are in mi355x_groth16_phase2_check.h, which a
 * ceremony runs beside the entry points below; the third is in this library nowhere:
 *   - the pairing check that the SRS rows are consistent powers (e([tau^(k+1)]1, g2) = e([tau^k]1, [tau]2), and the same for the alpha
 *     and beta rows): mi_phase2_init checks the rows point by point only -- on the curve, in the r-torsion, not at infinity -- and
 *     derives a key from whatever passes that.  mi_srs_check_powers makes the pairing check over the same rows: call it first;
 *   - the contributions' proofs of knowledge of delta and the verification of a transcript of contributions: mi_phase2_contribute
 *     below moves delta and leaves no record.  mi_phase2_contribute_proved writes a Schnorr record per contribution, and
 *     mi_phase2_verify_adopt checks a contributor's claimed Z, K and delta points against one's own state and takes them over
 *     (mi_phase2_get_array exports what it takes back).  The commitment keys' sigma has the same there, over the state's points
 *     [-sigma_k]2: mi_phase2_contribute_sigma_proved, mi_phase2_verify_adopt_sigma, and mi_phase2_get_pedersen_vk for the sealed key's
 *     verifying half, so that a ceremony starts from sigma = 1 and nobody holds the scalar;
 *   - gnark's mpcsetup file formats (Phase1 / Phase2 WriteTo): their layout is NOT AVAILABLE to this project (no gnark on the machines
 *     this was written on), so the SRS, the state and the records cross this interface as plain arrays in this project's own layout.
 *     The keys leave as the streams of mi355x_groth16_keyfile.h and mi355x_groth16_vkfile.h, with those headers' caveats.
 * Whether a key -- a sealed state's or a file's -- IS the key of this circuit under this SRS can be checked without deriving it again:
 * mi355x_groth16_keyaudit.h.
 */
#ifndef MI355X_GROTH16_PHASE2_H
#define MI355X_GROTH16_PHASE2_H
#include "mi355x_groth16.h"
#include "mi355x_groth16_setup.h"
#include "mi355x_groth16_keyfile.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_srs_desc {          /* HOST pointers; affine, as mi_batch_scalar_mul_g1 / _g2 write them */
    const mi_g1_affine *tau_g1;       /* [tau^k]1, k = 0 .. n_tau_g1 - 1; needs n_tau_g1 >= 2 N */
    const mi_g1_affine *alpha_tau_g1; /* [alpha tau^k]1, k < N */
    const mi_g1_affine *beta_tau_g1;  /* [beta tau^k]1, k < N */
    const mi_g2_affine *tau_g2;       /* [tau^k]2, k < N */
    mi_g2_affine beta_g2;             /* [beta]2 */
    uint64_t n_tau_g1, n_alpha_tau_g1, n_beta_tau_g1, n_tau_g2;
} mi_srs_desc;

typedef struct mi_phase2 mi_phase2;   /* device-resident ceremony state: the plain arrays of both keys */

/* Device times of the last mi_phase2_init on ctx, by phase (HIP events on the context's stream; the phases run one after the other).
 * upload: SRS and R1CS to the device; check: the point checks of the SRS; point_ntt_g1 / _g2: the three G1 transforms / the G2 one,
 * without their conversion to affine; sparse_g1 / _g2: the column sort and the sums of points; z: the Z differences; affine: every
 * batched conversion to affine.  entries = nnz(A) + nnz(B) + nnz(C); long_columns / chunks: per matrix, the columns whose entry lists
 * were split over waves and the pieces they were split into (mi_setup_stats counts the same).  peak_bytes: the most device memory the
 * call's own allocations held at once (SRS rows, XYZZ working arrays, sorted matrices and the state's arrays; the context's workspaces
 * are mi_get_mem_ledger's). */
typedef struct mi_phase2_stats {
    float upload_ms, check_ms, point_ntt_g1_ms, point_ntt_g2_ms, sparse_g1_ms, sparse_g2_ms, z_ms, affine_ms, total_ms;
    uint64_t entries, long_columns, chunks, peak_bytes;
} mi_phase2_stats;

/* InitPhase2: the state for this circuit from this SRS, with delta = 1.  sigma: n_commitments values (may be NULL when there are none).
 * flags: 0, or MI_KEYFILE_NO_SUBGROUP_CHECK (the G2 points are not tested for membership of the r-torsion).
 * MI_EINVAL, with nothing left allocated: everything mi_groth16_setup refuses about the R1CS; a null SRS row or one shorter than
 * needed (tau_g1: 2 N; the others: N); a sigma of 0; an unknown flag; an SRS point off its curve, a G2 point outside the r-torsion,
 * an SRS point at infinity -- mi_last_error names the row (srs.tau_g1, srs.alpha_tau_g1, srs.beta_tau_g1, srs.tau_g2, srs.beta_g2) and
 * the lowest bad index in it.  Only the first 2 N / N points of a row are read and checked. */
int32_t mi_phase2_init(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_srs_desc *srs, const mi_fr *sigma, uint32_t flags, mi_phase2 **out);
/* Contribute: Z and the private wires' K are multiplied by 1 / delta, delta1 and delta2 by delta, BasisExpSigma[k] by sigma_factor[k]
 * (NULL = all 1), and the state's point [-sigma_k]2 -- which the verifying key's stream and mi_phase2_get_pedersen_vk are written
 * from -- by sigma_factor[k] as well.  Nothing else changes.  delta = 0 or a sigma_factor of 0:
 * MI_EINVAL and the state is as it was. */
int32_t mi_phase2_contribute(mi_ctx *ctx, mi_phase2 *st, const mi_fr *delta, const mi_fr *sigma_factor);
/* ExtractKeys: the state's arrays are COPIED into an ordinary mi_pk (fixed-base tables and all, as any adopted key), the commitments'
 * Pedersen keys (ped_out: room for n_commitments handles; may be NULL when there are none) and the verifying key's points (vk_out as
 * for mi_groth16_setup).  The Pedersen pairs for mi_vk_desc.ped come from the state's points: mi_phase2_get_pedersen_vk
 * (mi355x_groth16_phase2_check.h), so no caller needs sigma.  Sealing does not end the ceremony: one state can be sealed after every
 * contribution. */
int32_t mi_phase2_seal(mi_ctx *ctx, const mi_phase2 *st, mi_pk **pk_out, mi_pedersen_pk **ped_out, mi_vk_out *vk_out);
/* Both keys as gnark's streams, written from the state's arrays: the out / cap / len triples of mi_groth16_setup_to_streams (cap too
 * small: MI_EINVAL with both *len and *vk_len set). */
int32_t mi_phase2_to_streams(mi_ctx *ctx, const mi_phase2 *st, uint32_t encoding, uint8_t *out_host, size_t cap, size_t *len,
                             uint8_t *vk_out_host, size_t vk_cap, size_t *vk_len);
int32_t mi_phase2_free(mi_ctx *ctx, mi_phase2 *st);
int32_t mi_phase2_get_stats(mi_ctx *ctx, mi_phase2_stats *out);

/* What a maintainer dumps when a key is in doubt: one array of the state to host memory.  which: */
#define MI_PHASE2_G1_A 0u
#define MI_PHASE2_G1_B 1u
#define MI_PHASE2_G2_B 2u
#define MI_PHASE2_G1_K 3u
#define MI_PHASE2_G1_Z 4u
#define MI_PHASE2_VK_K 5u
#define MI_PHASE2_BASIS 6u              /* + 2 k: Basis of commitment k; + 2 k + 1: its BasisExpSigma */
/* *n (never NULL) = the array's points; out_host (may be NULL: the count alone) has room for cap of them.  cap too small: MI_EINVAL. */
int32_t mi_phase2_get_array(mi_ctx *ctx, const mi_phase2 *st, uint32_t which, void *out_host, uint64_t cap, uint64_t *n);

#ifdef __cplusplus
}
#endif
#endif
