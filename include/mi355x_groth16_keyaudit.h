/* mi355x_groth16_keyaudit.h -- is this the key of this circuit under this SRS?  The audit of a proving and verifying key that came
 * from someone else -- a key file, a sealed ceremony state, plain arrays -- against the compiled R1CS and a powers-of-tau SRS, WITHOUT
 * deriving the key again (BN254).
 *
 * mi_phase2_init derives a key from an SRS with a point transform and sparse sums of points (mi355x_groth16_phase2.h); the stream
 * loaders of mi355x_groth16_keyfile.h / _vkfile.h check a key's points one by one and nothing about what they are.  The derivation is
 * LINEAR in the key's points, so it is checked here by one random linear combination per array, the same-ratio idea of
 * mi355x_groth16_phase2_check.h applied to the key instead of the SRS.  For coefficients r_j per wire and u = A r (a product by rows):
 *     sum_j r_j [A_j]1  =  sum_i u_i [L_i(tau)]1  =  sum_k p_k [tau^k]1      with p = iNTT_N(u)
 * where index i of the transform means w^i, w the domain generator of fft.NewDomain (mi355x_groth16_setup.h): one sparse product, one
 * Fr transform and two MSMs in place of a point transform and a sparse sum of points.  No step multiplies a point by a scalar one
 * lane at a time.
 *
 * COEFFICIENTS.  The stream r_k of mi355x_groth16_phase2_check.h under one seed: r_k is the little-endian integer of the first 16 bytes
 * of SHA-256("mi355x-ceremony-coeff" | seed (32 bytes) | le64(k)), computed on the device.  Wire j takes r_j = stream[j]; Z takes
 * q_i = stream[nb_wires + i].  One stream serves every relation of a call; each relation is judged on its own, so each keeps its own
 * bound.  seed == NULL: the library draws the 32 bytes from the operating system (getrandom); if that fails the call returns MI_ENODEV
 * and no verdict.
 * THE SOUNDNESS CLAIM BELOW HOLDS ONLY FOR A SEED THE MAKER OF THE DATA CANNOT PREDICT: whoever knows the seed before choosing the points
 * knows every r_k and can make defects cancel.  A fixed seed is for tests and for reproducing a verdict, never for judging a key from
 * someone else.
 *
 * SOUNDNESS.  A mask of 0 means: every group element listed in the table below is the one mi_groth16_setup would produce for the
 * (tau, alpha, beta) of the SRS and the gamma, delta, sigma_k implied by gamma2, delta2, g_sigma_neg_k -- with error at most about
 * 2^-128 per relation over an unpredictable seed.  (After the point checks every point lies in a group of prime order r; a relation
 * reads sum_j r_j d_j = 0 mod r with d_j the defects in the exponent, and a non-zero d_j leaves one value of r_j, of 2^128, that
 * satisfies it.  The coefficients are hashed PER INDEX so that two defects that cancel under equal coefficients do not cancel here.)
 * A key that is what it should be passes every relation for every seed.
 * The audit presumes the rows are consistent powers: run mi_srs_check_powers or mi_phase1_check first.  Against rows that are not,
 * a mask of 0 says nothing.
 *
 * NOT COVERED:
 *   - who knows delta or sigma: that is what the records of contributions say (mi355x_groth16_phase2_check.h: the delta chain and the
 *     sigma chain).  The audit says that BasisExpSigma is sigma Basis for the sigma of g_sigma_neg, not that nobody kept sigma;
 *   - encodings and mask canonicity: the audit judges group elements.  A wire flagged finite whose point is (0, 0) in the arrays, or
 *     two encodings of one stream, are the loaders' business (a stream is decoded by exactly their code, refusals included);
 *   - gnark's formats: the stream layouts carry the "recalled, not pinned to gnark" caveat of the loaders this header shares them
 *     with (mi355x_groth16_keyfile.h, mi355x_groth16_vkfile.h);
 *   - the SRS itself (see above), and the lists of public committed wires of a verifying key's stream, which are not group elements.
 *
 * Same library and conventions as mi355x_groth16_phase2_check.h: status codes, Montgomery mi_fr, affine points with (0, 0) = infinity,
 * mi_last_error names the field, nothing left allocated after a refusal, every relation evaluated whatever the others say.
 */
#ifndef MI355X_GROTH16_KEYAUDIT_H
#define MI355X_GROTH16_KEYAUDIT_H
#include "mi355x_groth16_phase2_check.h"
#include "mi355x_groth16_phase1.h"
#include "mi355x_groth16_verify.h"
#include "mi355x_groth16_vkfile.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- the claim
 * Device-resident: the five arrays of a proving key in mi_pk_desc's layout and order with the two infinity masks, the Pedersen pairs
 * Basis[k] / BasisExpSigma[k], the proving key's small points (alpha1, beta1, delta1, beta2, delta2), and the verifying key (alpha1,
 * beta2, gamma2, delta2, K, the mi_pedersen_vk pairs).  Three ways in, one way out (mi_key_claim_free). */
typedef struct mi_key_claim mi_key_claim;

/* Both of gnark's streams in either encoding (each stream its own), through the decoders, point checks, refusals and texts of
 * mi_pk_load_stream / mi_vk_load_stream -- the same code -- stopping before the handover: no mi_pk, no fixed-base tables.
 * flags: those of the loaders (MI_KEYFILE_NO_SUBGROUP_CHECK, MI_KEYFILE_SUBGROUP_BY_R). */
int32_t mi_key_claim_from_streams(mi_ctx *ctx, const uint8_t *pk_buf, size_t pk_len, const uint8_t *vk_buf, size_t vk_len, uint32_t flags,
                                  mi_key_claim **out);
/* Borrows a phase-2 state's arrays where they are: nothing is copied, the state must outlive the claim, and the claim follows the state
 * through later contributions.  The verifying key's Pedersen pairs are made from the state's sigma (mi_pedersen_vk_make). */
int32_t mi_key_claim_from_phase2(mi_ctx *ctx, const mi_phase2 *st, mi_key_claim **out);
/* desc: a mi_pk_desc with DEVICE arrays as mi_pk_write_dev takes it (masks on the host; committed_wires is not read); ped: n_ped pairs
 * of device arrays; vk_desc: host memory.  Everything is copied.  The points are checked as mi_phase2_verify_adopt checks a claim:
 * reduced words on the curve, the G2 points in the r-torsion; (0, 0) is allowed inside K, vk.K, Z and the bases, and not for the small
 * points or inside A, B, G2.B.  MI_EINVAL names the array and the lowest bad index. */
int32_t mi_key_claim_from_arrays(mi_ctx *ctx, const mi_pk_desc *desc, const mi_pedersen_arrays *ped, uint32_t n_ped, const mi_vk_desc *vk_desc,
                                 mi_key_claim **out);
int32_t mi_key_claim_free(mi_ctx *ctx, mi_key_claim *claim);

/* ---------------------------------------------------------------- the audit
 * Wire classes: V = public wires and commitment wires; C = committed wires; P = the remaining private wires.  r^X = r with every wire
 * outside class X set to 0.  S(v; row) = MSM(iNTT_N(v), row[0 .. N)) with v padded by zeros from n_constraints to N.
 * T(v) = S(A v; beta_tau_g1) + S(B v; alpha_tau_g1) + S(C v; tau_g1).  slot_x(j): where wire j's point lies in the compacted array.
 * The bits of *failed: the relation that does NOT hold (g1, g2: the generators). */
#define MI_KEY_BAD_SMALL       1u   /* as affine words pk.alpha1 = vk.alpha1 = alpha_tau_g1[0], pk.beta1 = beta_tau_g1[0], pk.beta2 = vk.beta2 = beta_g2,
                                       pk.delta2 = vk.delta2; and e(pk.delta1, g2) = e(g1, pk.delta2) */
#define MI_KEY_BAD_A           2u   /* sum_{j: !inf_a[j]} r_j pk.A[slot_a(j)] = S(A r; tau_g1), compared as points.  r runs over ALL wires, so a
                                       wire wrongly flagged infinite fails */
#define MI_KEY_BAD_B1          4u   /* the same with B over pk.G1.B / tau_g1 */
#define MI_KEY_BAD_B2          8u   /* the same with B over pk.G2.B / tau_g2 (G2 MSMs) */
#define MI_KEY_BAD_K_PRIVATE  16u   /* e(sum_{j in P} r_j pk.K[slot_k(j)], pk.delta2) = e(T(r^P), g2) */
#define MI_KEY_BAD_K_PUBLIC   32u   /* e(sum_{j in V} r_j vk.K[.], vk.gamma2) = e(T(r^V), g2) */
#define MI_KEY_BAD_BASIS      64u   /* e(sum_k sum_i r_{committed[k][i]} Basis_k[i], vk.gamma2) = e(T(r^C), g2) */
#define MI_KEY_BAD_SIGMA     128u   /* for every k: e(sum_i r_{committed[k][i]} Basis_k[i], g_sigma_neg_k) e(sum_i r_{..} BasisExpSigma_k[i], g_k) = 1 */
#define MI_KEY_BAD_Z         256u   /* e(sum_i q_i Z[bitrev(i)], pk.delta2) = e(MSM(q, tau_g1[N .. 2N)) - MSM(q, tau_g1[0 .. N)), g2) */

/* Exactly one of srs (HOST rows, brought up row by row as mi_srs_check_powers does, with mi_phase2_init's point checks and refusal
 * texts; the call holds one row at a time) and p1 (rows already on the device, checked when the state took them).
 * flags: 0 or MI_KEYFILE_NO_SUBGROUP_CHECK (the G2 points of a host SRS are not tested for membership of the r-torsion; WITHOUT the test
 * the soundness claim does not cover MI_KEY_BAD_B2).
 * MI_EINVAL before any relation is evaluated, with nothing left allocated: a null ctx, r1cs, claim or failed; an unknown flag;
 * everything mi_groth16_setup refuses about the R1CS; both or neither SRS source; a null or short row, or a domain above the phase-1
 * state's; an SRS point off its curve, outside the r-torsion or at infinity; a claim whose SHAPE is not the circuit's, mi_last_error
 * naming the count: n_z != N, nb_wires differs, n_a or n_b (= n of G2.B) is not the number of clear mask bytes, n_k != the number of
 * private wires that are neither committed nor a commitment wire, vk.n_k != nb_public + n_commitments, the number of Pedersen keys
 * (of either key) or a basis length differs from n_committed[k].  MI_ENODEV: seed == NULL and no randomness.
 * Otherwise MI_OK and *failed = the mask of relations that do not hold.  Every relation is evaluated whatever the others say. */
int32_t mi_key_audit(mi_ctx *ctx, const mi_r1cs_desc *r1cs, const mi_srs_desc *srs /* or NULL */, const mi_phase1 *p1 /* or NULL */,
                     const mi_key_claim *claim, const uint8_t seed[32] /* may be NULL */, uint32_t flags, uint32_t *failed);

/* Times of the last mi_key_audit on ctx by phase, in milliseconds of the host's clock around work that is waited for (the phases run one
 * after the other): upload: the R1CS, the wire lists and the SRS rows to the device; point_check: the point checks of a host SRS;
 * coeff: the coefficient kernel, the class masks and the gathers; sparse: the nine masked products (mi_r1cs_eval_dev); transform: the
 * nine inverse transforms and the sums; srs_msm_g1 / srs_msm_g2: the thirteen G1 MSMs / the G2 one over SRS rows; key_msm_g1 /
 * key_msm_g2: the MSMs over the claimed arrays (A, B, K, vk.K, Z, two per commitment / G2.B); pairing: the Miller loops, the final
 * exponentiations and the verdicts.  peak_bytes: the most device memory the call's own allocations held at once (the vectors, one SRS
 * row, the resident R1CS; the MSM's and the transform's workspaces belong to the context and are mi_get_mem_ledger's). */
typedef struct mi_key_audit_stats {
    float upload_ms, point_check_ms, coeff_ms, sparse_ms, transform_ms, srs_msm_g1_ms, srs_msm_g2_ms, key_msm_g1_ms, key_msm_g2_ms, pairing_ms, total_ms;
    uint32_t relations;     /* pairing relations judged */
    uint64_t peak_bytes;
} mi_key_audit_stats;
int32_t mi_key_audit_get_stats(mi_ctx *ctx, mi_key_audit_stats *out);

#ifdef __cplusplus
}
#endif
#endif
